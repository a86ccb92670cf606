"""CPU checks of the fp64 loss references and of the shared case generator
(tests/loss_cases.py) that test_gpu_losses.py feeds to the HIP kernels."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as LC  # noqa: E402

from distributed_rl_amd.ops import torch_ref  # noqa: E402


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("shape", LC.R2D2_SHAPES)
def test_r2d2_ref_matches_recurrent_targets(shape, rescale):
    """The loop reference against algos/r2d2.nstep_recurrent_targets (CPU
    path, fp32 inside) to fp32 accuracy, and its closed-form dq_train
    against autograd through that function."""
    from distributed_rl_amd.algos.r2d2 import nstep_recurrent_targets

    T, m, n, B, A = shape
    c = LC.r2d2_case(*shape)
    # R2D2's own discount, not the grid's 1/2: nstep_recurrent_targets forms
    # the n-step return as a difference of gamma^t-weighted prefix sums,
    # which cancels to nothing once gamma^T drops below 1e-16 (0.5^76)
    c.gamma = 0.997
    ref = torch_ref.r2d2_sequence_loss_ref(
        c.q_train, c.q_tgt, c.act, c.rew, c.done, c.w, m, n, c.gamma,
        LC.ALPHA, 0.9, rescale)
    q_train = c.q_train.float().requires_grad_(True)
    q_online = torch.cat([c.q_tgt[:m].float(), q_train])
    td, q_taken, _ = nstep_recurrent_targets(
        q_online, c.q_tgt.float(), c.act, c.rew.float(), c.done.float(), m, n,
        c.gamma, rescale)
    W = T - 1 - m
    assert ref["td"].shape == (W, B) and ref["dq_train"].shape == (T - m, B, A)
    # fp32 accuracy: without rescaling a few ulps of values below 8 (4e-6);
    # with it the fp32 h^-1 is off by up to 1.8e-4 on |x| <= 2 (its
    # sqrt(t) - 1 cancels, see test_rescale_grid_and_inverse_error_pinned),
    # times gamma^n <= 1 and h' <= 0.501
    tol = 1e-4 if rescale else 4e-6
    assert torch.allclose(td.double(), ref["td"], atol=tol, rtol=0)
    loss = 0.5 * (c.w.float() * td.pow(2)).mean()
    loss.backward()
    # |d loss| <= mean(w |td|) * tol, w <= 1, |td| < 8
    assert abs(float(loss.detach()) - float(ref["loss"])) < 8 * tol
    assert abs(float(q_taken.detach().mean()) - float(ref["value"])) < 1e-6
    gmax = float(ref["dq_train"].abs().max())
    # dq = -w td / (B W): the same tol, scaled like the gradient
    assert gmax > 0
    assert torch.allclose(q_train.grad.double(), ref["dq_train"],
                          atol=tol / (B * W), rtol=0)
    assert bool((ref["dq_train"][W:] == 0).all())
    prio = torch_ref.sequence_priority(ref["td"].abs(), LC.ALPHA, 0.9)
    assert torch.equal(prio, ref["prio"])


def test_r2d2_ref_done_mask_only_at_last_step():
    """done must change td only where t + n == T - 1."""
    T, m, n, B, A = 16, 4, 5, 8, 6
    c = LC.r2d2_case(T, m, n, B, A)
    args = (c.q_train, c.q_tgt, c.act, c.rew)
    a = torch_ref.r2d2_sequence_loss_ref(*args, torch.zeros(B).double(), c.w,
                                         m, n, c.gamma, LC.ALPHA, 0.9, True)
    b = torch_ref.r2d2_sequence_loss_ref(*args, torch.ones(B).double(), c.w,
                                         m, n, c.gamma, LC.ALPHA, 0.9, True)
    W = T - 1 - m
    reach = torch.tensor([(m + ti) + min(n, T - 1 - m - ti) == T - 1
                          for ti in range(W)])
    assert torch.equal(a["td"][~reach], b["td"][~reach])
    assert bool((a["td"][reach] != b["td"][reach]).any())


def test_r2d2_zero_td_case():
    c = LC.r2d2_zero_td_case(16, 4, 5, 8, 6)
    ref = torch_ref.r2d2_sequence_loss_ref(
        c.q_train, c.q_tgt, c.act, c.rew, c.done, c.w, 4, 5, c.gamma,
        LC.ALPHA, 0.9, False)
    assert bool((ref["td"][:, 0] == 0).all()) and float(ref["prio"][0]) == 0.0
    assert bool((ref["td"][:, 1:] != 0).any())
    # exact in fp32: every input is a multiple of 2^-8 below 2^6
    for t in (c.q_train, c.q_tgt, c.rew):
        assert torch.equal(t.float().double(), t)
        assert torch.equal((t * 256).round(), t * 256)


@pytest.mark.parametrize("pre_act", [False, True])
@pytest.mark.parametrize("B", LC.QHEAD_B)
def test_qhead_ref_equals_composition(B, pre_act):
    """dueling_q_head_loss_ref against F.linear + dueling + the existing
    torch_ref.nstep_dqn_loss, all in fp64, gradients by autograd."""
    for c in (LC.qhead_grid(B, pre_act), LC.qhead_random(B, pre_act, 0)):
        ref = LC.qhead_ref(c)
        leaves = [t.clone().requires_grad_(True) for t in (c.h[0], *c.online)]

        def q_of(h, wa, ba, wv, bv):
            h = F.relu(h) if pre_act else h
            adv = F.linear(h[:, :LC.HH], wa, ba)
            val = F.linear(h[:, LC.HH:], wv, bv)
            return (adv + val) - adv.mean(dim=-1, keepdim=True)

        q_s = q_of(*leaves)
        q_on = q_of(c.h[1], *c.online)
        q_tg = q_of(c.h[2], *c.target)
        loss, prio = torch_ref.nstep_dqn_loss(
            q_s, q_on, q_tg, c.act, c.rew, c.done, c.w, c.gamma, c.n_step,
            LC.ALPHA)
        grads = torch.autograd.grad(loss * LC.GOUT, leaves)
        assert loss.dtype == torch.float64
        assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-13 * max(
            1, float(ref["loss"]))
        assert torch.allclose(prio, ref["prio"], rtol=1e-12, atol=0)
        for g, k in zip(grads, ("dh", "dwa", "dba", "dwv", "dbv")):
            assert torch.allclose(g, ref[k], rtol=1e-10, atol=1e-15), k


# ---------------------------------------------------------------------------
# generator properties
# ---------------------------------------------------------------------------


def _fp32_exact(t):
    return torch.equal(t.float().double(), t)


def _check_planted(raw, raw_want, done, w, big):
    assert torch.equal(raw, raw_want)
    if not big:
        return
    assert bool((raw == 1.0).any()) and bool((raw == -1.0).any())
    inside = (raw.abs() < 1) & (raw.abs() > 1 - 2e-3)
    assert bool(inside.any()) and bool((raw.abs() > 2).any())
    assert bool((done == 1).any()) and bool((w == 0).any())
    # both clip bounds on done rows and on live rows
    assert bool(((raw.abs() == 1) & (done == 1)).any())
    assert bool(((raw.abs() == 1) & (done == 0)).any())


@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("A", LC.DQN_A)
@pytest.mark.parametrize("B", LC.DQN_B)
def test_dqn_grid_properties(B, A, dueling):
    c = LC.dqn_grid(B, A, dueling)
    a_star, raw, gap = LC.dqn_details(*c.q, c.act, c.rew, c.done, c.gamma_n)
    tie = c.tie_lo >= 0
    assert bool(tie.any()) and bool((gap[tie] == 0).all())
    assert torch.equal(a_star[tie], c.tie_lo[tie])        # earliest index
    _check_planted(raw, c.raw_want, c.done, c.w, B >= 63)
    # a wrong a* moves the target by >= 1/8
    tg = c.q[2]
    d = (tg[:, :, None] - tg[:, None, :]).abs() + torch.eye(A) * 1e9
    assert float(d.min()) * c.gamma_n >= 0.125
    tables = [t for pair in c.heads for t in pair] if dueling else list(c.q)
    for t in tables + [c.rew, c.w]:
        assert _fp32_exact(t)
    for t in tables:                                      # and in bf16
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    if dueling:     # the kernel's fp32 row mean is exact
        for adv in (c.heads[0][0], c.heads[2][0]):
            m32 = adv.float().sum(dim=1) / A
            assert torch.equal(m32.double(), adv.mean(dim=1))
    if B >= 257:
        assert bool((c.w[64:128] == 0).all())


@pytest.mark.parametrize("pre_act", [False, True])
@pytest.mark.parametrize("B", LC.QHEAD_B)
def test_qhead_grid_properties(B, pre_act):
    c = LC.qhead_grid(B, pre_act)
    ref = LC.qhead_ref(c)
    top2 = ref["q_on"].topk(2, dim=1).values
    assert bool((top2[c.tie, 0] == top2[c.tie, 1]).all())
    assert bool((ref["a_star"][c.tie] == 1).all())        # earliest of (1, 2)
    _check_planted(ref["raw"], c.raw_want, c.done, c.w, B >= 31)
    q_tg = LC._qhead_q(c.h[2], *c.target, pre_act)
    d = (q_tg[:, :, None] - q_tg[:, None, :]).abs() + torch.eye(LC.QA) * 1e9
    assert float(d.min()) * c.gamma ** c.n_step >= 0.125
    for t in (*c.h, *c.online, *c.target):
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    assert _fp32_exact(c.rew)
    wa, ba = c.online[0], c.online[1]
    assert float(wa.abs().max()) <= 0.25
    assert torch.equal((wa * 64).round(), wa * 64)
    assert torch.equal((ba * 64).round(), ba * 64)
    # the 512-term dots: fp32 in two orders == fp64
    h = torch.relu(c.h[0]) if pre_act else c.h[0]
    d64 = h[:, :LC.HH] @ wa.t()
    h32, w32 = h[:, :LC.HH].float(), wa.float()
    fwd = torch.zeros(B, LC.QA)
    for k in range(LC.HH):
        fwd += h32[:, k:k + 1] * w32[:, k]
    lanes = (h32[:, None, :] * w32[None]).view(B, LC.QA, 64, 8).sum(-1).sum(-1)
    assert torch.equal(fwd.double(), d64) and torch.equal(lanes.double(), d64)
    if pre_act:
        hs = c.h[0]
        assert bool((hs < 0).any())
        assert bool(((hs == 0) & torch.signbit(hs)).any())
        assert bool(((hs == 0) & ~torch.signbit(hs)).any())


# ---------------------------------------------------------------------------
# exclusion caps of the random-valued cases, from the reference alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("A", LC.DQN_A)
@pytest.mark.parametrize("B", LC.DQN_B)
def test_dqn_random_exclusion_cap(B, A):
    for make in (LC.dqn_random, LC.dueling_random):
        for c in (make(B, A, 0), LC.to_bf16_exact(make(B, A, 0))):
            _, raw, gap = LC.dqn_details(*c.q, c.act, c.rew, c.done, c.gamma_n)
            # one row of a tiny batch is more than 5 %: none may fall out
            assert int(LC.excluded(raw, gap).sum()) <= int(LC.EXCL_CAP * B)


@pytest.mark.parametrize("pre_act", [False, True])
@pytest.mark.parametrize("seed", LC.QHEAD_SEEDS)
@pytest.mark.parametrize("B", LC.QHEAD_B)
def test_qhead_random_exclusion_cap(B, seed, pre_act):
    ref = LC.qhead_ref(LC.qhead_random(B, pre_act, seed))
    n_out = int(LC.qhead_excluded(ref).sum())
    assert n_out <= int(LC.EXCL_CAP * B)
    if seed == 0:   # the case whose loss and weight gradients are compared
        assert n_out == 0


# ---------------------------------------------------------------------------
# V-trace, policy and element-wise inputs
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(20, 32), (80, 300)])
def test_vtrace_case_bands(shape):
    c = LC.vtrace_case(*shape)
    above, below, between = LC.band_shares(c, 1.3, 0.7)
    assert min(above, below, between) >= 0.2
    assert float((c.not_done == 0).double().mean()) >= 0.2
    for t in (c.b_logp, c.t_logp, c.rew, c.val, c.boot):
        assert _fp32_exact(t)


def test_vtrace_ref_distinguishes_the_two_clips():
    """Swapping rho_bar and c_bar moves vs and pg_adv far above any fp32
    tolerance, so a kernel that confuses them cannot pass."""
    c = LC.vtrace_case(20, 32)
    a = torch_ref.vtrace(c.b_logp, c.t_logp, c.rew, c.val, c.boot, c.not_done,
                         c.gamma, 1.3, 0.7, 0.9)
    b = torch_ref.vtrace(c.b_logp, c.t_logp, c.rew, c.val, c.boot, c.not_done,
                         c.gamma, 0.7, 1.3, 0.9)
    assert a[0].dtype == torch.float64
    assert float((a[0] - b[0]).abs().max()) > 1e-2
    assert float((a[1] - b[1]).abs().max()) > 1e-2


@pytest.mark.parametrize("N", LC.POLICY_N)
def test_policy_case_properties(N):
    c = LC.policy_case(N, 6)
    lp = torch.log_softmax(c.logits, -1)
    assert bool(torch.isfinite(lp).all())
    assert float(lp[0].exp().float().min()) == 0.0        # underflows in fp32
    am = c.logits.argmax(1)
    assert bool((c.act[0::2] == am[0::2]).all())
    if N > 1:
        assert bool((c.act[1::2] != am[1::2]).all())
    assert _fp32_exact(c.logits) and _fp32_exact(c.adv)


def test_rescale_grid_and_inverse_error_pinned():
    """The grid holds both zeros and both signs over 1e-6 .. 1e4; on it the
    present fp32 h^-1 formula (its sqrt(t) - 1 cancels) is pinned against
    fp64: absolute error between 1e-6 and 2e-4 on |x| <= 1, relative
    error below 2e-4 above. A form without the cancellation changes R2D2's
    numerics and is left to a follow-up with its own A/B run."""
    x = LC.rescale_grid(4099)
    assert bool(((x == 0) & torch.signbit(x)).any())
    assert bool(((x == 0) & ~torch.signbit(x)).any())
    assert float(x.max()) == pytest.approx(1e4, rel=1e-6)
    assert float(x[x > 0].min()) == pytest.approx(1e-6, rel=1e-6)
    ref = torch_ref.inv_value_rescale(x)
    got = torch_ref.inv_value_rescale(x.float()).double()
    err = (got - ref).abs()
    small = x.abs() <= 1.0
    assert 1e-6 < float(err[small].max()) < 2e-4
    big = x.abs() > 1.0
    assert float((err[big] / ref[big].abs()).max()) < 2e-4


@pytest.mark.parametrize("shape", LC.SEQPRIO_SHAPES)
def test_seqprio_case(shape):
    td = LC.seqprio_case(*shape)
    p = torch_ref.sequence_priority(td, LC.ALPHA, 0.9)
    assert float(p[0]) == 0.0
    if shape[1] > 2:
        assert int(td[:, 1].argmax()) == 0 and int(td[:, 2].argmax()) == shape[0] - 1
