"""Pure-PyTorch (fp32, eager) reference implementations of every fused HIP op.

These are the numerics oracles the HIP kernels (distributed_rl_amd/ops/hip/*)
are unit-tested against, and the CPU execution path (no GPU present).
Each function documents the reference code whose math it reproduces
(file:line into /root/reference/).
"""

from __future__ import annotations

from typing import Tuple

import torch

# ---------------------------------------------------------------------------
# K1 — uint8 -> float /255 dequant (APE_X/Learner.py:61-67 does
#      torch.tensor(u8).float()/255 on the GPU synchronously)
# ---------------------------------------------------------------------------


def dequant_frames(x_u8: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    return x_u8.to(dtype) / 255.0


# ---------------------------------------------------------------------------
# K2b — 3x3 stride-1 pad-1 conv with the IMPALA-ResNet block fusions:
#       relu on the input, + bias, + residual, relu on the output
#       (models/base_agent.py ResidualBlock: x + c2(relu(c1(relu(x)))))
# ---------------------------------------------------------------------------


def conv3x3_res(x, weight, bias=None, relu_in: bool = False,
                relu_out: bool = False, residual=None) -> torch.Tensor:
    y = torch.nn.functional.conv2d(
        torch.nn.functional.relu(x) if relu_in else x, weight, bias, padding=1)
    if residual is not None:
        y = y + residual
    return torch.nn.functional.relu(y) if relu_out else y


# ---------------------------------------------------------------------------
# K2c — max-pool 3x3 stride 2 pad 1 of the IMPALA-ResNet torso
#       (models/base_agent.py ImpalaResNet: nn.MaxPool2d(3, 2, 1)); the
#       winning tap kh*3 + kw per output element, and the input gradient as
#       an ordered fp32 gather over that tap plane
# ---------------------------------------------------------------------------


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.max_pool2d(x, 3, 2, 1)


def maxpool3x3s2_taps(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, taps): taps is uint8 of out's shape, the winner's position in its
    window as kh*3 + kw, from the library's flat h*W + w index."""
    W = x.shape[-1]
    out, i = torch.nn.functional.max_pool2d(x, 3, 2, 1, return_indices=True)
    P, Q = out.shape[-2:]
    p = torch.arange(P, device=x.device).view(P, 1)
    q = torch.arange(Q, device=x.device).view(1, Q)
    tap = (i // W - (2 * p - 1)) * 3 + (i % W - (2 * q - 1))
    return out, tap.to(torch.uint8)


def maxpool3x3s2_bwd(gout: torch.Tensor, taps: torch.Tensor, H: int,
                     W: int) -> torch.Tensor:
    """fp32 input gradient: each input pixel sums gout over the windows whose
    tap names it, in ascending (po, qo) order. Pixel h = 2*po - 1 + kh, so
    per pixel a larger kh is the earlier window: taps run (kh, kw) from
    (2, 2) down to (0, 0)."""
    N, C, P, Q = gout.shape
    g = gout.float()
    zero = torch.zeros((), dtype=torch.float32, device=gout.device)
    gx = torch.zeros(N, C, H, W, dtype=torch.float32, device=gout.device)

    def span(k, size, n_win):
        # windows [lo, hi) whose tap k lies inside [0, size)
        lo = 1 if k == 0 else 0
        hi = min(n_win, (size - k) // 2 + 1)
        return lo, hi

    for kh in (2, 1, 0):
        p0, p1 = span(kh, H, P)
        for kw in (2, 1, 0):
            q0, q1 = span(kw, W, Q)
            if p1 <= p0 or q1 <= q0:
                continue
            hit = taps[:, :, p0:p1, q0:q1] == kh * 3 + kw
            h0, w0 = 2 * p0 - 1 + kh, 2 * q0 - 1 + kw
            gx[:, :, h0:h0 + 2 * (p1 - p0):2, w0:w0 + 2 * (q1 - q0):2] += \
                torch.where(hit, g[:, :, p0:p1, q0:q1], zero)
    return gx


# ---------------------------------------------------------------------------
# K4 — n-step double-DQN TD loss + new priority + IS-weighted loss
#      (APE_X/Learner.py:83-114; gamma**n with done mask; TD clip to [-1,1];
#      priority (|clip(td)|+1e-7)**alpha; loss 0.5*mean(w*td^2))
# ---------------------------------------------------------------------------


def nstep_dqn_loss(
    q_online_s: torch.Tensor,  # (B, A) differentiable
    q_online_sp: torch.Tensor,  # (B, A) no-grad
    q_target_sp: torch.Tensor,  # (B, A) no-grad
    actions: torch.Tensor,  # (B,) int64
    rewards: torch.Tensor,  # (B,) discounted n-step return
    dones: torch.Tensor,  # (B,) float 1.0 where terminal
    weights: torch.Tensor,  # (B,) PER importance weights
    gamma: float,
    n_step: int,
    alpha: float,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (loss, new_priorities).

    Note the reference hardcodes gamma=0.99 in the bootstrap term
    (APE_X/Learner.py:103) regardless of cfg GAMMA — a defect per SURVEY §7;
    we use the configured gamma.
    """
    B = q_online_s.shape[0]
    a_star = q_online_sp.argmax(dim=1)  # double-DQN action selection
    next_q = q_target_sp.gather(1, a_star.unsqueeze(1)).squeeze(1)
    target = rewards + (gamma ** n_step) * next_q * (1.0 - dones)
    q_sa = q_online_s.gather(1, actions.long().unsqueeze(1)).squeeze(1)
    td = (target.detach() - q_sa).clamp(-1.0, 1.0)
    new_priority = (td.detach().abs() + 1e-7) ** alpha
    loss = 0.5 * (weights * td.pow(2)).mean()
    return loss, new_priority


# ---------------------------------------------------------------------------
# K6 — R2D2 value rescaling h / h^-1 (R2D2/Learner.py:22-35)
# ---------------------------------------------------------------------------

_RESCALE_EPS = 1e-3


def value_rescale(x: torch.Tensor, eps: float = _RESCALE_EPS) -> torch.Tensor:
    return torch.sign(x) * ((x.abs() + 1.0).sqrt() - 1.0) + eps * x


def inv_value_rescale(x: torch.Tensor, eps: float = _RESCALE_EPS) -> torch.Tensor:
    # closed-form inverse (R2D2/Learner.py:29-35)
    return torch.sign(x) * (
        ((1.0 + 4.0 * eps * (x.abs() + 1.0 + eps)).sqrt() - 1.0).pow(2)
        / (4.0 * eps ** 2)
        - 1.0
    )


# ---------------------------------------------------------------------------
# K7 — R2D2 sequence priority: eta-mix 0.9*max + 0.1*mean over per-step |td|
#      then **alpha (R2D2/Learner.py:175-181, R2D2/Player.py:209-211)
# ---------------------------------------------------------------------------


def sequence_priority(
    td_abs: torch.Tensor, alpha: float, eta: float = 0.9
) -> torch.Tensor:
    """td_abs: (T, B) -> (B,) priorities."""
    mix = eta * td_abs.max(dim=0).values + (1.0 - eta) * td_abs.mean(dim=0)
    return mix ** alpha


# ---------------------------------------------------------------------------
# K8 — IMPALA V-trace (IMPALA/Learner.py:121-226)
# ---------------------------------------------------------------------------


def vtrace(
    behavior_log_prob: torch.Tensor,  # (T, B) log mu(a|s)
    target_log_prob: torch.Tensor,  # (T, B) log pi(a|s)
    rewards: torch.Tensor,  # (T, B)
    values: torch.Tensor,  # (T, B) V(s_t) under target net
    bootstrap_value: torch.Tensor,  # (B,) V(s_T)
    not_done: torch.Tensor,  # (B,) 1.0 if trajectory did NOT terminate
    gamma: float,
    rho_bar: float = 1.0,
    c_bar: float = 1.0,
    lam: float = 1.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (vs, pg_advantage, rho_clipped).

    Terminal handling matches the reference: the bootstrap value is masked
    by not_done (IMPALA/Player.py:183-186 emits not_done; Learner applies it
    to the bootstrap), and the scan runs reversed in time with
    c_i = lam * min(c_bar, rho_i) (IMPALA/Learner.py:176-200).

    DELIBERATE DIVERGENCE (also recorded in docs/PARITY.md): the reference
    omits the clipped-rho factor on the delta of the LAST unrolled step
    (IMPALA/Learner.py:176-185 applies rho only inside the loop body, not on
    the step that seeds the reversed scan); we apply rho_clipped to EVERY
    step's delta — the V-trace paper's form. Values differ from the
    reference whenever pi != mu on the final step of an unroll.
    """
    T, B = rewards.shape
    rho = (target_log_prob - behavior_log_prob).exp()
    rho_c = rho.clamp(max=rho_bar)
    c = lam * rho.clamp(max=c_bar)

    values_tp1 = torch.cat(
        [values[1:], (bootstrap_value * not_done).unsqueeze(0)], dim=0
    )
    deltas = rho_c * (rewards + gamma * values_tp1 - values)

    acc = torch.zeros(B, dtype=values.dtype, device=values.device)
    vs_minus_v = torch.empty_like(values)
    for t in reversed(range(T)):
        acc = deltas[t] + gamma * c[t] * acc
        vs_minus_v[t] = acc
    vs = values + vs_minus_v

    vs_tp1 = torch.cat([vs[1:], (bootstrap_value * not_done).unsqueeze(0)], dim=0)
    pg_adv = rho_c * (rewards + gamma * vs_tp1 - values)
    return vs, pg_adv, rho_c


# ---------------------------------------------------------------------------
# K9 — IMPALA policy/critic losses (IMPALA/Learner.py:95-119, 224)
# ---------------------------------------------------------------------------


def impala_loss(
    logits: torch.Tensor,  # (T*B, A) differentiable (learner policy head)
    values_pred: torch.Tensor,  # (T*B,) differentiable critic
    actions: torch.Tensor,  # (T*B,) int64
    pg_adv: torch.Tensor,  # (T*B,) no-grad
    vs: torch.Tensor,  # (T*B,) no-grad V-trace targets
    entropy_coef: float,
    critic_coef: float = 1.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    log_pi = torch.log_softmax(logits, dim=-1)
    pi = log_pi.exp()
    entropy = -(pi * log_pi).sum(-1).mean()
    log_pi_a = log_pi.gather(1, actions.unsqueeze(1)).squeeze(1)
    obj_actor = (log_pi_a * pg_adv.detach()).mean() + entropy_coef * entropy
    critic_loss = 0.5 * torch.nn.functional.mse_loss(values_pred, vs.detach())
    total = -obj_actor + critic_coef * critic_loss
    return total, obj_actor, critic_loss, entropy


# ---------------------------------------------------------------------------
# K10 host oracle — proportional PER semantics (contract from SURVEY §2.8):
#   P(i) = p_i / sum(p)   (alpha applied producer-side),
#   IS weight w_i = (1/(n*P_i))^beta / max_j w_j   (APE_X/ReplayMemory.py:64-67)
# ---------------------------------------------------------------------------


def per_probabilities(priorities: torch.Tensor) -> torch.Tensor:
    return priorities / priorities.sum()


def per_is_weights(
    probs: torch.Tensor, n: int, beta: float
) -> torch.Tensor:
    w = (1.0 / (n * probs)) ** beta
    return w / w.max()


# ---------------------------------------------------------------------------
# K10 kernel oracles — the sum-tree itself, operation by operation. Every step
# of the device kernels is one correctly rounded fp32 operation (or 64-bit
# integer arithmetic), so these reproduce them bit for bit: numpy float32
# arrays round once per operation, uint64 arrays wrap mod 2^64.
# ---------------------------------------------------------------------------

_U64 = (1 << 64) - 1


def sumtree_build(leaves, P: int):
    """float32[2P] tree: leaves at tree[P + i] (zeros behind them), every
    inner node n the fp32 sum tree[2n] + tree[2n+1], built bottom-up;
    tree[1] is the root, tree[0] stays 0."""
    import numpy as np

    leaves = np.asarray(leaves, dtype=np.float32).reshape(-1)
    assert P >= 1 and P & (P - 1) == 0 and leaves.size <= P
    tree = np.zeros(2 * P, dtype=np.float32)
    tree[P : P + leaves.size] = leaves
    n = P
    while n > 1:
        half = n >> 1
        tree[half:n] = tree[n : 2 * n : 2] + tree[n + 1 : 2 * n : 2]
        n = half
    return tree


def sumtree_hash01(seed_u64: int, i):
    """splitmix64 counter hash of (seed, i) -> float32 in [0, 1): the top 24
    bits of the mixed word times 2^-24. seed is the device seed word as an
    unsigned 64-bit value (an int64 tensor's value reduced mod 2^64)."""
    import numpy as np

    shape = np.shape(i)
    i = np.asarray(i).astype(np.uint64).reshape(-1)
    seed = np.full(1, int(seed_u64) & _U64, dtype=np.uint64)
    z = seed + np.uint64(0x9E3779B97F4A7C15) * (i + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    h = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return h.reshape(shape)


def sumtree_bump_seed(seed: int) -> int:
    """The LCG step of the device seed word, mod 2^64 (unsigned result)."""
    return ((int(seed) & _U64) * 6364136223846793005
            + 1442695040888963407) & _U64


def sumtree_sample(tree, P: int, n_valid: int, k: int, seed: int):
    """Stratified inverse-CDF descent, draw i of k:
    u = (float32(i) + hash01(seed, i)) * (tree[1] / float32(k)); at each
    level u < tree[2*node] goes left, else u -= tree[2*node] and goes right;
    the leaf is clamped to n_valid - 1; prob = tree[P + leaf] / tree[1].
    Returns (idx int64[k], prob float32[k])."""
    import numpy as np

    tree = np.asarray(tree, dtype=np.float32)
    assert tree.size == 2 * P and 1 <= n_valid <= P and k >= 1
    i = np.arange(k, dtype=np.int64)
    total = tree[1]
    u = (i.astype(np.float32) + sumtree_hash01(seed, i)) * (total / np.float32(k))
    node = np.ones(k, dtype=np.int64)
    level = 1
    while level < P:
        left_child = node << 1
        lv = tree[left_child]
        left = u < lv
        u = np.where(left, u, u - lv)
        node = np.where(left, left_child, left_child + 1)
        level <<= 1
    idx = np.minimum(node - P, n_valid - 1)
    prob = tree[P + idx] / total
    return idx, prob


# ---------------------------------------------------------------------------
# n-step return folding (actor side; APE_X/Player.py:38-51)
# ---------------------------------------------------------------------------


def fold_nstep_reward(rewards: torch.Tensor, gamma: float) -> torch.Tensor:
    """rewards: (..., n) -> (...) discounted sum_t gamma^t r_t."""
    n = rewards.shape[-1]
    disc = gamma ** torch.arange(n, dtype=rewards.dtype, device=rewards.device)
    return (rewards * disc).sum(-1)
