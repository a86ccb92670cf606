"""Pure-PyTorch (eager) reference implementations of every fused HIP op:
fp32 by default, fp64 when fed fp64 (the loss / target oracles are).

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
# fp64 oracles of the fused sequence / head losses. Written from the
# formulas, not from the kernels: plain loops and autograd, no ops.* calls.
# ---------------------------------------------------------------------------


def r2d2_sequence_loss_ref(q_train, q_tgt, actions, rewards, done, weights,
                           burn_in: int, n_step: int, gamma: float,
                           alpha: float, eta: float, use_rescaling: bool):
    """R2D2 target / loss / priority over one batch of sequences, in fp64.

    q_train (T-m, B, A) online rows from the burn-in m on, q_tgt (T, B, A),
    actions / rewards (T, B), done / weights (B,). For every window step
    t in [m, T-1): n = min(n_step, T-1-t), a* = argmax_a q_online[t+n],
    G = sum_{k<n} gamma^k r_{t+k} + gamma^n h^-1(q_tgt[t+n, a*]), the
    bootstrap masked by (1 - done) only where t+n == T-1, and
    td = h(G) - q_online[t, a_t].

    Returns dict(td (W, B), loss, prio (B,), value, td_abs, dq_train), with
    dq_train = d loss / d q_train in closed form (the target is constant).
    """
    import math

    T, B, A = q_tgt.shape
    m = int(burn_in)
    W = T - 1 - m
    qo = q_train.double().tolist()
    qt = q_tgt.double().tolist()
    act = actions.long().tolist()
    rew = rewards.double().tolist()
    dn = done.double().tolist()
    wt = weights.double().tolist()
    eps = _RESCALE_EPS

    def h(x):
        return math.copysign(math.sqrt(abs(x) + 1.0) - 1.0, x) + eps * x

    def h_inv(x):
        r = (math.sqrt(1.0 + 4.0 * eps * (abs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps)
        return math.copysign(r * r - 1.0, x)

    td = torch.zeros(W, B, dtype=torch.float64)
    dq = torch.zeros(T - m, B, A, dtype=torch.float64)
    loss = value = 0.0
    for ti in range(W):
        t = m + ti
        n = min(n_step, T - 1 - t)
        tn = t + n
        for b in range(B):
            ret = sum(gamma ** k * rew[t + k][b] for k in range(n))
            row = qo[tn - m][b]
            a_star = max(range(A), key=lambda a: (row[a], -a))  # earliest max
            boot = qt[tn][b][a_star]
            if use_rescaling:
                boot = h_inv(boot)
            if tn == T - 1:
                boot *= 1.0 - dn[b]
            G = ret + gamma ** n * boot
            if use_rescaling:
                G = h(G)
            q_taken = qo[ti][b][act[t][b]]
            d = G - q_taken
            td[ti, b] = d
            loss += 0.5 * wt[b] * d * d
            value += q_taken
            dq[ti, b, act[t][b]] = -wt[b] * d / (B * W)
    td_abs = td.abs()
    prio = (eta * td_abs.max(dim=0).values
            + (1.0 - eta) * td_abs.mean(dim=0)) ** alpha
    return dict(td=td, loss=torch.tensor(loss / (B * W), dtype=torch.float64),
                prio=prio,
                value=torch.tensor(value / (B * W), dtype=torch.float64),
                td_abs=td_abs.mean(), dq_train=dq)


def dueling_q_head_loss_ref(h_s, wa, ba, wv, bv, h_on, h_tg, wa_t, ba_t, wv_t,
                            bv_t, actions, rewards, dones, weights,
                            gamma: float, n_step: int, alpha: float,
                            pre_act: bool = False, gout: float = 1.0,
                            dtype: torch.dtype = torch.float64):
    """Heads on the [adv | val] halves of the hidden rows, optional ReLU,
    dueling, n-step double-DQN loss, all in fp64; gradients of gout * loss
    for (h_s, wa, ba, wv, bv) by autograd. ``dtype`` = fp32 runs the same
    formula in fp32 (a scale for a kernel's error, not a reference).

    Returns dict(loss, prio, qmean, a_star, raw, td, q_on, dh, dwa, dba, dwv,
    dbv); raw is the unclipped TD error and q_on the online Q(s', .) rows
    (what decides a*)."""
    HH = wa.shape[1]
    leaves = [t.detach().to(dtype).clone().requires_grad_(True)
              for t in (h_s, wa, ba, wv.reshape(1, -1), bv.reshape(1))]
    hs, wa_, ba_, wv_, bv_ = leaves
    c = [t.detach().to(dtype) for t in (h_on, h_tg, wa_t, ba_t,
                                        wv_t.reshape(1, -1), bv_t.reshape(1))]
    rewards, dones, weights = (t.to(dtype) for t in (rewards, dones, weights))
    hon, htg, wat, bat, wvt, bvt = c

    def q_of(h, w_a, b_a, w_v, b_v):
        if pre_act:
            h = torch.relu(h)
        adv = h[:, :HH] @ w_a.t() + b_a
        val = h[:, HH:] @ w_v.t() + b_v
        return adv - adv.mean(dim=1, keepdim=True) + val

    q_s = q_of(hs, wa_, ba_, wv_, bv_)
    with torch.no_grad():
        q_on = q_of(hon, wa_, ba_, wv_, bv_)
        q_tg = q_of(htg, wat, bat, wvt, bvt)
        a_star = q_on.argmax(dim=1)
        target = rewards + gamma ** n_step * q_tg.gather(
            1, a_star.unsqueeze(1)).squeeze(1) * (1.0 - dones)
    q_sa = q_s.gather(1, actions.long().unsqueeze(1)).squeeze(1)
    raw = target - q_sa
    td = raw.clamp(-1.0, 1.0)
    loss = 0.5 * (weights * td.pow(2)).mean()
    grads = torch.autograd.grad(loss * gout, leaves)
    return dict(loss=loss.detach(), prio=(td.detach().abs() + 1e-7) ** alpha,
                qmean=q_s.detach().max(dim=1).values.mean(), a_star=a_star,
                raw=raw.detach(), td=td.detach(), q_on=q_on,
                dh=grads[0], dwa=grads[1], dba=grads[2],
                dwv=grads[3].reshape(wv.shape), dbv=grads[4].reshape(bv.shape))


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


# ---------------------------------------------------------------------------
# ordered fold of the weight-gradient partial planes (conv_mfma.hip,
# wrw_reduce_block) — the same fp32 additions in the same order
# ---------------------------------------------------------------------------


def wrw_fold_ordered(part: torch.Tensor, n_elem: int, b_part=None,
                     out_dtype: torch.dtype = torch.float32):
    """part: (planes, >= n_elem) fp32, columns past n_elem are padding.
    Element e: 16 plane groups, group g adds planes g, g+16, g+32, ... in
    that order onto 0, then t = ((s_0 + s_1) + ...) + s_15. b_part: optional
    (b_planes, cout) fp32 with cout dividing 256; column c: G = 256 // cout
    groups, group g adds rows g, g+G, ... onto 0, then the group sums are
    added onto 0 in group order. Returns (gw, gb or None), rounded to
    out_dtype (round-to-nearest-even) at the very end."""
    p = part.detach().to("cpu", torch.float32)[:, :n_elem]
    planes = p.shape[0]
    sums = []
    for g in range(16):
        s = torch.zeros(n_elem, dtype=torch.float32)
        for k in range(g, planes, 16):
            s = s + p[k]
        sums.append(s)
    t = sums[0]
    for g in range(1, 16):
        t = t + sums[g]
    gw = t.to(out_dtype)
    gb = None
    if b_part is not None:
        b = b_part.detach().to("cpu", torch.float32)
        b_planes, cout = b.shape
        assert 256 % cout == 0
        G = 256 // cout
        tb = torch.zeros(cout, dtype=torch.float32)
        for g in range(G):
            s = torch.zeros(cout, dtype=torch.float32)
            for k in range(g, b_planes, G):
                s = s + b[k]
            tb = tb + s
        gb = tb.to(out_dtype)
    return gw, gb
