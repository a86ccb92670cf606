"""The fused loss / target kernels against fp64 CPU references at their
edge shapes (inputs from tests/loss_cases.py, shared with test_loss_ref.py).

Rules for every family:
* the reference is fp64 on the CPU;
* every backward gets the upstream gradient GOUT = 0.375, never 1;
* where the reference gradient is zero the kernel's is exactly zero (the
  sign of a zero is not held: autograd itself yields -0 for -coef * gout);
* outputs written once per element, without atomics, are bit-identical
  across two calls on the same inputs;
* atomic sums (DQN loss / q-mean, r2d2 stats, obj / ent of policy_loss_fwd)
  are compared with the reference only.

Tolerances: every compared quantity X is held to
    max |X_gpu - X_64| / max(|X_64|, floor) <= TOL[name]
with floor the quantity's natural scale (1 for values and sums, 1e-3 for
priorities, the largest reference gradient for gradients). TOL[name] is
4 x the error measured on an MI355X over all cases of the family; e_32 is
the same distance for the torch_ref formula run in fp32 on the CPU. bf16
outputs get half a bf16 ulp of the reference (2^-9 |ref|) on top.
docs/KERNELS.md has the table.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as LC  # noqa: E402

from distributed_rl_amd.ops import torch_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
I64, I32 = torch.int64, torch.int32

# name: 4 x e_gpu               e_gpu measured on an MI355X | e_32 (CPU fp32)
# (bf16 outputs: after half a bf16 ulp of the reference is taken off)
TOL = {
    "dqn.loss": 2.8e-07,        # 6.81e-08 | 3.30e-08
    "dqn.qmean": 7.2e-07,       # 1.80e-07 | 1.26e-07
    "dqn.prio": 5.5e-04,        # 1.37e-04 | 1.37e-04
    "dqn.grad": 2.1e-06,        # 5.01e-07 | 4.64e-07
    "dueling.out": 7.2e-07,     # 1.79e-07 | 1.79e-07
    "dueling.grad": 5.5e-07,    # 1.37e-07 | 1.22e-07
    "qhead.loss": 5.0e-07,      # 1.24e-07 | 8.22e-08
    "qhead.qmean": 1.2e-06,     # 2.80e-07 | 1.48e-07
    "qhead.prio": 6.8e-05,      # 1.70e-05 | 1.70e-05
    "qhead.dh": 3.4e-07,        # 8.25e-08 | 1.79e-06
    "qhead.dw": 1.7e-07,        # 4.19e-08 | 1.74e-06
    "r2d2.td": 0.0e+00,         # 0.00e+00 | 0.00e+00
    "r2d2.loss": 3.4e-07,       # 8.50e-08 | 5.42e-08
    "r2d2.prio": 4.0e-07,       # 9.85e-08 | 8.42e-08
    "r2d2.value": 9.8e-08,      # 2.44e-08 | -
    "r2d2.td_abs": 4.9e-07,     # 1.22e-07 | 3.42e-08
    "r2d2.dq": 1.6e-07,         # 3.80e-08 | 3.74e-08
    "r2d2.h.td": 1.3e-04,       # 3.11e-05 | 2.54e-05
    "r2d2.h.loss": 2.0e-05,     # 4.93e-06 | 4.93e-06
    "r2d2.h.prio": 1.2e-05,     # 2.82e-06 | 2.81e-06
    "r2d2.h.td_abs": 8.6e-06,   # 2.14e-06 | 2.14e-06
    "r2d2.h.dq": 3.5e-05,       # 8.54e-06 | 8.54e-06
    "vtrace.vs": 3.6e-06,       # 8.95e-07 | 9.19e-07
    "vtrace.pg": 5.5e-06,       # 1.35e-06 | 1.44e-06
    "vtrace.rho": 3.1e-07,      # 7.61e-08 | 5.99e-08
    "policy.logpa": 7.5e-06,    # 1.85e-06 | 1.77e-07
    "policy.pi": 7.4e-06,       # 1.84e-06 | 1.81e-07
    "policy.H": 7.4e-06,        # 1.84e-06 | 1.70e-07
    "policy.ent": 7.4e-06,      # 1.84e-06 | 7.73e-08
    "policy.obj": 2.8e-07,      # 6.80e-08 | 6.80e-08
    "policy.dlogits": 2.5e-06,  # 6.05e-07 | 1.54e-07
    "impala.loss": 2.8e-07,     # 6.90e-08 | 6.90e-08
    "impala.obj": 3.5e-07,      # 8.66e-08 | 4.67e-08
    "impala.critic": 3.0e-07,   # 7.48e-08 | 6.12e-08
    "impala.dout": 2.0e-06,     # 4.84e-07 | 1.83e-07
    "rescale.h": 3.5e-07,       # 8.73e-08 | 8.73e-08
    "rescale.h_inv": 3.1e-04,   # 7.52e-05 | 8.27e-05
    "seqprio": 3.0e-07,         # 7.48e-08 | 7.48e-08
    "clip": 2.3e-06,            # 5.66e-07 | 9.27e-05
}
# policy.*: e_gpu is 10..24 x e_32 because the kernel uses __expf / __logf:
# __expf(x) = exp2(x * log2 e), and the rounding of that product is worth
# |x| * 2^-24 in the result, 1.8e-6 at the |x| ~ 30 that logits * 8 reach; the
# entropy mean inherits it (it is a bias, it does not average out as e_32 does).


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def ops(ext):
    from distributed_rl_amd import ops as _ops

    return _ops


def D(t, dtype=F32):
    return t.detach().to(dtype).to(DEV)


def G(t, dtype=F32):
    return D(t, dtype).requires_grad_(True)


def gout():
    return torch.tensor(LC.GOUT, dtype=F32, device=DEV)


def hold(name, got, ref, floor, ref32=None, bf16=False, cap=None):
    """Print e_gpu (and e_32) for ``name``, then hold e_gpu to TOL[name].
    With bf16, half a bf16 ulp of the reference is taken off first. ``cap``
    is an absolute bound on top, where an older test holds one."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().reshape(-1)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    if bf16:
        err = (err - LC.ulp_bf16(ref)).clamp_min(0.0)
    e = float((err / ref.abs().clamp_min(floor)).max())
    e32 = LC.rel_err(ref32, ref, floor) if ref32 is not None else float("nan")
    print(f"ERR {name} e_gpu={e:.3e} e_32={e32:.3e} floor={floor:.3e} "
          f"abs={float(err.max()):.3e}")
    assert e <= TOL[name], (name, e, TOL[name])
    assert cap is None or float(err.max()) <= cap, (name, float(err.max()))


def exactly_zero(t):
    return bool((t == 0).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.detach().reshape(-1).contiguous().view(torch.uint8),
        b.detach().reshape(-1).contiguous().view(torch.uint8))


def gfloor(ref):
    m = float(ref.abs().max())
    assert m > 0
    return m


# ---------------------------------------------------------------------------
# n-step double-DQN loss, with and without the dueling heads
# ---------------------------------------------------------------------------


def _dqn_case(B, A, kind, dt, dueling):
    if kind == "grid":
        c = LC.dqn_grid(B, A, dueling)
    else:
        c = (LC.dueling_random if dueling else LC.dqn_random)(B, A, 0)
    return LC.to_bf16_exact(c) if dt is BF16 else c


def _dqn_ref(c, dtype, dueling):
    """loss, prio, qmean and the gradients of GOUT * loss from
    torch_ref.nstep_dqn_loss in ``dtype`` (fp64: the reference; fp32: e_32)."""
    if dueling:
        leaves = [t.to(dtype).requires_grad_(True) for t in c.heads[0]]
        adv, val = leaves
        q_s = adv - adv.mean(dim=1, keepdim=True) + val[:, None]
    else:
        leaves = [c.q[0].to(dtype).requires_grad_(True)]
        q_s = leaves[0]
    loss, prio = torch_ref.nstep_dqn_loss(
        q_s, c.q[1].to(dtype), c.q[2].to(dtype), c.act, c.rew.to(dtype),
        c.done.to(dtype), c.w.to(dtype), c.gamma, c.n_step, LC.ALPHA)
    grads = torch.autograd.grad(loss * LC.GOUT, leaves)
    return loss.detach(), prio, q_s.detach().max(dim=1).values.mean(), grads


def _dqn_run(ops, c, dt, dueling):
    common = (D(c.act, I64), D(c.rew), D(c.done), D(c.w), c.gamma, c.n_step,
              LC.ALPHA)
    if dueling:
        (a_s, v_s), (a_on, v_on), (a_tg, v_tg) = c.heads
        leaves = [G(a_s, dt), G(v_s[:, None], dt)]
        loss, prio, qmean = ops.dueling_nstep_dqn_loss(
            leaves[0], leaves[1], D(a_on, dt), D(v_on[:, None], dt),
            D(a_tg, dt), D(v_tg[:, None], dt), *common)
    else:
        leaves = [G(c.q[0], dt)]
        loss, prio, qmean = ops.nstep_dqn_loss(
            leaves[0], D(c.q[1], dt), D(c.q[2], dt), *common,
            with_value_stat=True)
    loss.backward(gout())
    torch.cuda.synchronize()
    return loss.detach(), prio, qmean, [t.grad for t in leaves]


def _check_dqn(ops, B, A, kind, dt, dueling):
    c = _dqn_case(B, A, kind, dt, dueling)
    loss64, prio64, qm64, g64 = _dqn_ref(c, F64, dueling)
    loss32, prio32, qm32, g32 = _dqn_ref(c, F32, dueling)
    a_star, raw, gap = LC.dqn_details(*c.q, c.act, c.rew, c.done, c.gamma_n)
    # a* is taken on the inputs as they are, so only the clip band matters;
    # the grid rows sit exactly where planted and none is left out
    out = (torch.zeros(B, dtype=torch.bool) if kind == "grid"
           else ((raw.abs() - 1.0).abs() < LC.EXCL))
    keep = ~out
    assert int(out.sum()) <= int(LC.EXCL_CAP * B)

    loss, prio, qmean, grads = _dqn_run(ops, c, dt, dueling)
    loss2, prio2, qmean2, grads2 = _dqn_run(ops, c, dt, dueling)
    assert same_bits(prio, prio2)
    for a, b in zip(grads, grads2):
        assert same_bits(a, b)

    hold("dqn.loss", loss, loss64, 1.0, loss32)
    hold("dqn.qmean", qmean, qm64, 1.0, qm32)
    # relative to max(|prio|, 1e-3) the error peaks where |td| is near 0 (the
    # subtraction target - q cancels); test_dqn_loss_matches_ref holds
    # atol = 1e-5, which stays on top
    hold("dqn.prio", prio, prio64, 1e-3, prio32, cap=1e-5)
    floor = gfloor(g64[0]) if float(g64[0].abs().max()) > 0 else 1.0
    for g, r64, r32 in zip(grads, g64, g32):
        assert g.dtype == dt
        g = g.reshape(r64.shape).cpu()
        hold("dqn.grad", g[keep], r64[keep], floor, r32[keep], bf16=dt is BF16)
    # zeros of the reference gradient: clipped rows, and without the dueling
    # mean every action that was not taken
    clipped = keep & (raw.abs() > 1.0)
    if kind == "grid" and B >= 63:
        assert bool(clipped.any()) and bool((raw.abs() == 1.0).any())
    for g, r64 in zip(grads, g64):
        g = g.reshape(r64.shape).cpu()
        assert exactly_zero(r64[clipped]) and exactly_zero(g[clipped])
    if not dueling:
        taken = torch.zeros(B, A, dtype=torch.bool)
        taken[torch.arange(B), c.act] = True
        assert exactly_zero(grads[0].cpu()[~taken])
    # the clip bounds themselves pass gradient (torch.clamp's convention)
    on_bound = (raw.abs() == 1.0) & (c.w > 0)
    if bool(on_bound.any()):
        g0 = grads[0].cpu().double()
        sa = g0[torch.arange(B), c.act]
        assert bool((sa[on_bound] != 0).all())
        assert bool((g64[0][torch.arange(B), c.act][on_bound] != 0).all())


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["grid", "random"])
@pytest.mark.parametrize("A", LC.DQN_A)
@pytest.mark.parametrize("B", LC.DQN_B)
def test_nstep_dqn_loss(ops, B, A, kind, dt):
    _check_dqn(ops, B, A, kind, dt, dueling=False)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["grid", "random"])
@pytest.mark.parametrize("A", LC.DQN_A)
@pytest.mark.parametrize("B", LC.DQN_B)
def test_dueling_nstep_dqn_loss(ops, B, A, kind, dt):
    _check_dqn(ops, B, A, kind, dt, dueling=True)


@pytest.mark.parametrize("A", LC.DQN_A)
@pytest.mark.parametrize("B", LC.DQN_B)
def test_dueling_head(ops, B, A):
    c = LC.dueling_random(B, A, 1)
    adv, val = c.heads[0]
    up = c.heads[1][0] * LC.GOUT           # a full upstream gradient (B, A)

    def ref(dtype):
        a = adv.to(dtype).requires_grad_(True)
        v = val.to(dtype)[:, None].requires_grad_(True)
        out = (a + v) - a.mean(dim=-1, keepdim=True)
        ga, gv = torch.autograd.grad(out, [a, v], up.to(dtype))
        return out.detach(), ga, gv

    def run():
        a, v = G(adv), G(val[:, None])
        out = ops.dueling_head(a, v)
        out.backward(D(up))
        torch.cuda.synchronize()
        return out.detach(), a.grad, v.grad

    o64, ga64, gv64 = ref(F64)
    o32, ga32, gv32 = ref(F32)
    out, ga, gv = run()
    for a, b in zip((out, ga, gv), run()):
        assert same_bits(a, b)
    hold("dueling.out", out, o64, 1.0, o32)
    floor = max(gfloor(ga64), gfloor(gv64))
    hold("dueling.grad", ga, ga64, floor, ga32)
    hold("dueling.grad", gv, gv64, floor, gv32)


# ---------------------------------------------------------------------------
# q-head: head projections + dueling + loss in one kernel, bf16 in and out
# ---------------------------------------------------------------------------

QHEAD_KINDS = ["grid"] + [f"seed{s}" for s in LC.QHEAD_SEEDS]


def _qhead_run(ops, c):
    leaves = [G(t, BF16) for t in (c.h[0], *c.online)]
    consts = [D(t, BF16) for t in (c.h[1], c.h[2], *c.target)]
    loss, prio, qmean = ops.dueling_q_head_loss(
        *leaves, *consts, D(c.act, I64), D(c.rew), D(c.done), D(c.w), c.gamma,
        c.n_step, LC.ALPHA, pre_act=c.pre_act)
    loss.backward(gout())
    torch.cuda.synchronize()
    return loss.detach(), prio, qmean, [t.grad for t in leaves]


@pytest.mark.parametrize("kind", QHEAD_KINDS)
@pytest.mark.parametrize("pre_act", [False, True], ids=["post", "pre"])
@pytest.mark.parametrize("B", LC.QHEAD_B)
def test_dueling_q_head_loss(ops, B, pre_act, kind):
    c = (LC.qhead_grid(B, pre_act) if kind == "grid"
         else LC.qhead_random(B, pre_act, int(kind[4:])))
    ref = LC.qhead_ref(c)
    r32 = LC.qhead_ref(c, dtype=F32)
    out = (torch.zeros(B, dtype=torch.bool) if kind == "grid"
           else LC.qhead_excluded(ref))
    keep = ~out
    assert int(out.sum()) <= int(LC.EXCL_CAP * B)

    loss, prio, qmean, grads = _qhead_run(ops, c)
    loss2, prio2, qmean2, grads2 = _qhead_run(ops, c)
    assert same_bits(prio, prio2)
    for a, b in zip(grads, grads2):
        assert a.dtype == BF16 and same_bits(a, b)

    hold("qhead.prio", prio.cpu()[keep], ref["prio"][keep], 1e-3,
         r32["prio"][keep])
    hold("qhead.qmean", qmean, ref["qmean"], 1.0, r32["qmean"])
    dh = grads[0].cpu()
    dh_floor = gfloor(ref["dh"]) if float(ref["dh"].abs().max()) > 0 else 1.0
    hold("qhead.dh", dh[keep], ref["dh"][keep], dh_floor, r32["dh"][keep],
         bf16=True)
    clipped = keep & (ref["raw"].abs() > 1.0)
    assert exactly_zero(ref["dh"][clipped]) and exactly_zero(dh[clipped])
    if pre_act:     # the ReLU's backward mask, -0 and negatives included
        dead = c.h[0] <= 0
        assert bool(dead.any())
        assert exactly_zero(ref["dh"][dead]) and exactly_zero(dh[dead])
    if kind == "grid" and B >= 31:
        on_bound = (ref["raw"].abs() == 1.0) & (c.w > 0)
        assert bool(on_bound.any())
        assert bool((dh.double()[on_bound].abs().sum(dim=1) > 0).all())
    if not bool(out.any()):
        # sums over every row: only where no row may legitimately differ
        hold("qhead.loss", loss, ref["loss"], 1.0, r32["loss"])
        dw_floor = max(float(ref[k].abs().max())
                       for k in ("dwa", "dba", "dwv", "dbv"))
        if dw_floor > 0:
            for g, k in zip(grads[1:], ("dwa", "dba", "dwv", "dbv")):
                hold("qhead.dw", g.reshape(ref[k].shape), ref[k], dw_floor,
                     r32[k], bf16=True)


# ---------------------------------------------------------------------------
# R2D2 sequence loss
# ---------------------------------------------------------------------------

ETA = 0.9


def _r2d2_run(ops, ext, c, rescale):
    T, m, n, B = c.T, c.m, c.n, c.B
    q_train = G(c.q_train)
    args = (D(c.q_tgt), D(c.act, I32), D(c.rew), D(c.done), D(c.w))
    loss, prio, value, td_abs = ops.r2d2_sequence_loss(
        q_train, *args, m, n, c.gamma, LC.ALPHA, ETA, rescale)
    loss.backward(gout())
    td = torch.empty(T - 1 - m, B, dtype=F32, device=DEV)
    stats = torch.zeros(3, dtype=F32, device=DEV)
    ext.r2d2_loss_fwd(q_train.detach(), *args, m, n, c.gamma, rescale, td,
                      stats)
    torch.cuda.synchronize()
    return loss.detach(), prio, value, td_abs, td, q_train.grad


def _r2d2_fp32(c, rescale):
    """The reference's formula in fp32 (torch_ref h / h^-1), vectorised over
    the batch: td, loss, td_abs, prio and GOUT * dq_train, for e_32."""
    T, m, n, B, A = c.T, c.m, c.n, c.B, c.A
    W = T - 1 - m
    qo, qt, rew = c.q_train.float(), c.q_tgt.float(), c.rew.float()
    w, rows = c.w.float(), torch.arange(B)
    td = torch.empty(W, B)
    dq = torch.zeros(T - m, B, A)
    for ti in range(W):
        t = m + ti
        k = min(n, T - 1 - t)
        tn = t + k
        ret = sum((c.gamma ** i) * rew[t + i] for i in range(k))
        boot = qt[tn][rows, qo[tn - m].argmax(dim=1)]
        if rescale:
            boot = torch_ref.inv_value_rescale(boot)
        if tn == T - 1:
            boot = boot * (1.0 - c.done.float())
        g = ret + (c.gamma ** k) * boot
        if rescale:
            g = torch_ref.value_rescale(g)
        a = c.act[t].long()
        td[ti] = g - qo[ti][rows, a]
        dq[ti, rows, a] = -w * td[ti] * LC.GOUT / (B * W)
    return dict(td=td, loss=0.5 * (w * td.pow(2)).mean(),
                td_abs=td.abs().mean(), dq=dq,
                prio=torch_ref.sequence_priority(td.abs(), LC.ALPHA, ETA))


def _check_r2d2(ops, ext, c, rescale):
    T, m, n, B, A = c.T, c.m, c.n, c.B, c.A
    W = T - 1 - m
    ref = torch_ref.r2d2_sequence_loss_ref(
        c.q_train, c.q_tgt, c.act, c.rew, c.done, c.w, m, n, c.gamma,
        LC.ALPHA, ETA, rescale)
    loss, prio, value, td_abs, td, dq = _r2d2_run(ops, ext, c, rescale)
    r2 = _r2d2_run(ops, ext, c, rescale)
    assert same_bits(prio, r2[1]) and same_bits(td, r2[4])
    assert same_bits(dq, r2[5])
    # without rescaling every td is exact on the grid; with it the error is
    # that of the fp32 h^-1 (see test_inv_value_rescale), so the two modes
    # get constants of their own
    k = "r2d2.h." if rescale else "r2d2."
    r32 = _r2d2_fp32(c, rescale)
    hold(k + "td", td, ref["td"], 1.0, r32["td"])
    hold(k + "loss", loss, ref["loss"], 1.0, r32["loss"])
    hold("r2d2.value", value, ref["value"], 1.0)
    hold(k + "td_abs", td_abs, ref["td_abs"], 1.0, r32["td_abs"])
    hold(k + "prio", prio, ref["prio"], 1e-3, r32["prio"])
    assert dq.shape == (T - m, B, A)
    dq64 = ref["dq_train"] * LC.GOUT
    hold(k + "dq", dq, dq64, gfloor(dq64), r32["dq"])
    zero = ref["dq_train"] == 0
    assert bool(zero[W:].all())                 # the ti >= W row
    assert exactly_zero(dq.cpu()[zero])
    return ref, td, prio


@pytest.mark.parametrize("rescale", [False, True], ids=["raw", "rescaled"])
@pytest.mark.parametrize("shape", LC.R2D2_SHAPES, ids=str)
def test_r2d2_sequence_loss(ops, ext, shape, rescale):
    c = LC.r2d2_case(*shape)
    assert bool(c.ties.any()) and bool((c.done == 1).any())
    _check_r2d2(ops, ext, c, rescale)


@pytest.mark.parametrize("shape", [(16, 4, 5, 8, 6), (76, 4, 5, 5, 18)],
                         ids=str)
def test_r2d2_zero_td_sequence(ops, ext, shape):
    """td == 0 on the whole window of sequence 0 (exact on the grid without
    rescaling): its priority is exactly 0, the others are not."""
    c = LC.r2d2_zero_td_case(*shape)
    ref, td, prio = _check_r2d2(ops, ext, c, False)
    assert exactly_zero(ref["td"][:, 0]) and exactly_zero(td.cpu()[:, 0])
    assert float(prio[0]) == 0.0 and bool((prio[1:] > 0).all())


# ---------------------------------------------------------------------------
# V-trace, (T, B) and (B, T) layouts
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("clips", LC.VTRACE_CLIPS, ids=str)
@pytest.mark.parametrize("shape", LC.VTRACE_SHAPES, ids=str)
def test_vtrace(ops, shape, clips):
    c = LC.vtrace_case(*shape)
    rho_bar, c_bar, lam = clips
    tail = (c.gamma, rho_bar, c_bar, lam)

    def ref(dtype, b_logp):
        return torch_ref.vtrace(b_logp.to(dtype), c.t_logp.to(dtype),
                                c.rew.to(dtype), c.val.to(dtype),
                                c.boot.to(dtype), c.not_done.to(dtype), *tail)

    def run_tb():
        r = ops.vtrace(D(c.b_logp), D(c.t_logp), D(c.rew), D(c.val),
                       D(c.boot), D(c.not_done), *tail)
        torch.cuda.synchronize()
        return r

    # the (B, T) kernel takes raw behaviour probabilities: its reference is
    # fed the log of the fp32 mu the kernel reads
    mu32 = c.b_logp.exp().float()

    def run_bt():
        r = ops.vtrace_bt(D(mu32.t()).contiguous(), D(c.t_logp.t()).contiguous(),
                          D(c.rew.t()).contiguous(), D(c.val.t()).contiguous(),
                          D(c.boot), D(c.not_done), *tail)
        torch.cuda.synchronize()
        return r

    vs64, pg64, rho64 = ref(F64, c.b_logp)
    vs32, pg32, rho32 = ref(F32, c.b_logp)
    vs, pg, rho = run_tb()
    for a, b in zip((vs, pg, rho), run_tb()):
        assert same_bits(a, b)
    hold("vtrace.vs", vs, vs64, 1.0, vs32)
    hold("vtrace.pg", pg, pg64, 1.0, pg32)
    hold("vtrace.rho", rho, rho64, 1.0, rho32)

    bvs64, bpg64, _ = ref(F64, mu32.double().log())
    bvs, bpg = run_bt()
    for a, b in zip((bvs, bpg), run_bt()):
        assert same_bits(a, b)
    assert bvs.shape == (c.B, c.T)
    hold("vtrace.vs", bvs.t(), bvs64, 1.0, vs32)
    hold("vtrace.pg", bpg.t(), bpg64, 1.0, pg32)
    # the two layouts agree: each is within its constant of its reference,
    # and the references differ only by the rounding of mu
    for a, b, r1, r2, k in ((vs, bvs, vs64, bvs64, "vtrace.vs"),
                            (pg, bpg, pg64, bpg64, "vtrace.pg")):
        d = (a.double().cpu() - b.t().double().cpu()).abs()
        scale = r1.abs().clamp_min(1.0)
        slack = float(((r1 - r2).abs() / scale).max())
        assert float((d / scale).max()) <= 2 * TOL[k] + slack


# ---------------------------------------------------------------------------
# IMPALA policy head
# ---------------------------------------------------------------------------


def _policy_ref(c, er, dtype):
    logits = c.logits.to(dtype).requires_grad_(True)
    lp = torch.log_softmax(logits, dim=-1)
    pi = lp.exp()
    H = -(pi * lp).sum(-1)
    logpa = lp.gather(1, c.act[:, None])[:, 0]
    obj = (logpa * c.adv.to(dtype)).mean() + er * H.mean()
    (dl,) = torch.autograd.grad(obj * LC.GOUT, [logits])
    return NSd(logpa=logpa.detach(), pi=pi.detach(), H=H.detach(),
               ent=H.detach().mean(), obj=obj.detach(), dlogits=dl)


class NSd(dict):
    __getattr__ = dict.__getitem__


def _pg_floor(ref, adv, n):
    """Scale of a policy gradient: the largest reference gradient, but not
    below gout * max|adv| / n, what a row yields before its softmax
    saturates. On a saturated row (p == 1 in fp32) the taken action's
    adv * (1 - p) is below the resolution of p, in any fp32 evaluation
    (e_32 shows the same), so the realised gradient of such a row alone
    (N = 1) is no scale to measure against."""
    return max(gfloor(ref), LC.GOUT * float(adv.abs().max()) / n)


@pytest.mark.parametrize("A", [6, 18])
@pytest.mark.parametrize("N", LC.POLICY_N)
def test_policy_softmax_stats(ops, N, A):
    c = LC.policy_case(N, A)
    r64, r32 = _policy_ref(c, 0.0, F64), _policy_ref(c, 0.0, F32)

    def run():
        r = ops.policy_softmax_stats(D(c.logits), D(c.act, I64))
        torch.cuda.synchronize()
        return r

    logpa, pi, H, ent = run()
    for a, b in zip((logpa, pi, H), run()[:3]):
        assert same_bits(a, b)
    hold("policy.logpa", logpa, r64.logpa, 1.0, r32.logpa)
    hold("policy.pi", pi, r64.pi, 1.0, r32.pi)
    hold("policy.H", H, r64.H, 1.0, r32.H)
    hold("policy.ent", ent, r64.ent, 1.0, r32.ent)
    assert float(pi[0].min()) == 0.0            # row 0 underflows, stays finite


@pytest.mark.parametrize("er", [0.0, 0.01])
@pytest.mark.parametrize("N", LC.POLICY_N)
def test_impala_policy_objective(ops, N, er):
    c = LC.policy_case(N, 6)
    r64, r32 = _policy_ref(c, er, F64), _policy_ref(c, er, F32)

    def run():
        logits = G(c.logits)
        obj, ent = ops.impala_policy_objective(logits, D(c.act, I64),
                                               D(c.adv), er)
        obj.backward(gout())
        torch.cuda.synchronize()
        return obj.detach(), logits.grad

    obj, dl = run()
    assert same_bits(dl, run()[1])
    hold("policy.obj", obj, r64.obj, 1.0, r32.obj)
    hold("policy.dlogits", dl, r64.dlogits, _pg_floor(r64.dlogits, c.adv, N),
         r32.dlogits)


@pytest.mark.parametrize("er", [0.0, 0.01])
@pytest.mark.parametrize("shape", LC.IMPALA_SHAPES, ids=str)
def test_impala_fused_loss(ops, ext, shape, er):
    B, T, A = shape
    c = LC.impala_case(B, T, A)
    r64 = LC.impala_ref(c.out, c.act, c.adv, c.vs, er, B, T, A)
    r32 = LC.impala_ref(c.out.float(), c.act, c.adv.float(), c.vs.float(), er,
                        B, T, A)

    def run():
        out = G(c.out)
        o3 = out.detach().view(B, T + 1, A + 1)
        logits = o3[:, :T, :A].reshape(B * T, A).contiguous()
        v_t = o3[:, :T, A].contiguous()
        act = D(c.act, I64)
        stats = ops.policy_softmax_stats(logits, act)
        loss, obj, critic = ops.impala_fused_loss(
            out, v_t, stats, act, D(c.adv), D(c.vs), er, T)
        loss.backward(gout())
        torch.cuda.synchronize()
        return loss.detach(), obj, critic, out.grad

    loss, obj, critic, dout = run()
    again = run()
    assert same_bits(dout, again[3])
    assert same_bits(critic, again[2])          # no atomic upstream of it
    # the single-block forward on fixed inputs (mean_H comes from an atomic
    # sum, so it is held fixed here): all three scalars repeat bit for bit
    n = B * T
    fixed = (D(c.adv), D(c.adv.flip(0)), torch.full((1,), 1.25, device=DEV),
             D(c.vs.reshape(-1)), D(c.vs.reshape(-1).flip(0)), er)
    outs = [torch.empty(3, 1, device=DEV) for _ in range(2)]
    for o in outs:
        ext.impala_loss_fwd(*fixed, o[0], o[1], o[2])
    assert n == fixed[0].numel() and same_bits(outs[0], outs[1])
    hold("impala.loss", loss, r64.loss, 1.0, r32.loss)
    hold("impala.obj", obj, r64.obj, 1.0, r32.obj)
    hold("impala.critic", critic, r64.critic, 1.0, r32.critic)
    hold("impala.dout", dout, r64.dout, _pg_floor(r64.dout, c.adv, B * T),
         r32.dout)
    d3 = dout.cpu().view(B, T + 1, A + 1)
    assert exactly_zero(r64.dout.view(B, T + 1, A + 1)[:, T])
    assert exactly_zero(d3[:, T])               # t == T rows
    assert bool((d3[:, :T, A] != 0).any())      # the value column


# ---------------------------------------------------------------------------
# value rescale, sequence priority, grad clip
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n", LC.RESCALE_N)
def test_value_rescale(ops, n):
    x = LC.rescale_grid(n)
    y = ops.value_rescale(D(x))
    assert same_bits(y, ops.value_rescale(D(x)))
    hold("rescale.h", y, torch_ref.value_rescale(x), 1.0,
         torch_ref.value_rescale(x.float()))
    z = x == 0
    assert exactly_zero(y.cpu()[z[:n]])


@pytest.mark.parametrize("n", LC.RESCALE_N)
def test_inv_value_rescale(ops, n):
    """Pins the present error of the fp32 h^-1, whose sqrt(t) - 1 cancels
    near 0; the arithmetic is not changed here (see docs/KERNELS.md)."""
    x = LC.rescale_grid(n)
    y = ops.inv_value_rescale(D(x))
    assert same_bits(y, ops.inv_value_rescale(D(x)))
    hold("rescale.h_inv", y, torch_ref.inv_value_rescale(x), 1.0,
         torch_ref.inv_value_rescale(x.float()))


@pytest.mark.parametrize("shape", LC.SEQPRIO_SHAPES, ids=str)
def test_sequence_priority(ops, shape):
    td = LC.seqprio_case(*shape)
    p = ops.sequence_priority(D(td), LC.ALPHA, ETA)
    assert same_bits(p, ops.sequence_priority(D(td), LC.ALPHA, ETA))
    hold("seqprio", p, torch_ref.sequence_priority(td, LC.ALPHA, ETA), 1e-3,
         torch_ref.sequence_priority(td.float(), LC.ALPHA, ETA))
    assert float(p[0]) == 0.0                   # all-zero column


@pytest.mark.parametrize("n", LC.CLIP_N)
def test_clip_flat_grad(ops, n):
    x = LC.clip_case(n)
    norm64 = float(x.double().norm())
    buf = torch.full((1,), 123.0, dtype=F32, device=DEV)   # stale on purpose
    # below the threshold: untouched
    y = x.to(DEV)
    ops.clip_flat_grad_(y, 2.0 * norm64 + 1.0, buf)
    assert torch.equal(y.cpu(), x)
    # above it
    max_norm = 0.25 * norm64
    assert norm64 > max_norm > 0
    ref = x.double() * max_norm / (norm64 + 1e-6)
    ref32 = x * (max_norm / (x.norm() + 1e-6))
    ops.clip_flat_grad_(y, max_norm, buf)
    hold("clip", y, ref, gfloor(ref), ref32)
    # the reused buffer is zeroed per call: the clipped vector's norm is at
    # the threshold, so a stale sum would scale it a second time
    y2 = y.clone()
    ops.clip_flat_grad_(y2, max_norm * (1 + 1e-3), buf)
    assert torch.equal(y2, y)
    z = x.to(DEV)
    ops.clip_flat_grad_(z, max_norm)            # a fresh buffer: same bits up
    hold("clip", z, ref, gfloor(ref), ref32)    # to the atomic order


# ---------------------------------------------------------------------------
# host-side rejection: one spoiled argument per call, thrown before launch.
# Every spoiled tensor is a view of a buffer with at least the bytes the
# kernel would read, so a missing check fails pytest.raises and nothing else.
# ---------------------------------------------------------------------------

_WRONG = {F32: F64, BF16: F32, I64: I32, I32: I64, F64: F32}


def _z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _spoils(t, shape_arg):
    """(label, spoiled tensor) for one good tensor argument."""
    n = t.numel()
    wrong = _WRONG[t.dtype]
    out = [("dtype", _z(wrong, 2 * n + 2)[:n].view(t.shape)),
           ("on host", torch.zeros(t.shape, dtype=t.dtype))]
    if n >= 2:
        if t.dim() >= 2:
            big = _z(t.dtype, 2 * t.shape[0], *t.shape[1:])
            out.append(("strided", big[::2]))
        else:
            out.append(("strided", _z(t.dtype, 2 * n)[::2]))
    if not shape_arg:
        out.append(("count", _z(t.dtype, n + 1)))
    return out


B_, A_, T_, M_ = 5, 6, 7, 2       # small geometry of the good calls
W_ = T_ - 1 - M_


def _bf(*shape):
    return _z(BF16, *shape)


def _qhead_heads():
    return [("wa", _bf(6, 512)), ("ba", _bf(6)), ("wv", _bf(512)),
            ("bv", _bf(1))]


# binding -> (names of the arguments whose sizes set the shape, argument list)
BINDINGS = {
    "dqn_loss_fwd": (("q_s",), lambda: [
        ("q_s", _z(F32, B_, A_)), ("q_sp_on", _z(F32, B_, A_)),
        ("q_sp_tg", _z(F32, B_, A_)), ("act", _z(I64, B_)),
        ("rew", _z(F32, B_)), ("done", _z(F32, B_)), ("w", _z(F32, B_)),
        0.97, 0.6, ("loss_out", _z(F32, 1)), ("prio_out", _z(F32, B_)),
        ("grad_coef", _z(F32, B_)), ("qmax_out", _z(F32, 1))]),
    "dqn_loss_bwd": (("grad_q",), lambda: [
        ("grad_coef", _z(F32, B_)), ("act", _z(I64, B_)),
        ("gout", _z(F32, 1)), ("grad_q", _z(F32, B_, A_))]),
    "dueling_fwd": (("adv",), lambda: [
        ("adv", _z(F32, B_, A_)), ("val", _z(F32, B_)),
        ("out", _z(F32, B_, A_))]),
    "dueling_bwd": (("g",), lambda: [
        ("g", _z(F32, B_, A_)), ("gadv", _z(F32, B_, A_)),
        ("gval", _z(F32, B_))]),
    "dueling_dqn_loss_fwd": (("adv_s",), lambda: [
        ("adv_s", _z(F32, B_, A_)), ("val_s", _z(F32, B_)),
        ("adv_on", _z(F32, B_, A_)), ("val_on", _z(F32, B_)),
        ("adv_tg", _z(F32, B_, A_)), ("val_tg", _z(F32, B_)),
        ("act", _z(I64, B_)), ("rew", _z(F32, B_)), ("done", _z(F32, B_)),
        ("w", _z(F32, B_)), 0.97, 0.6, ("loss_out", _z(F32, 1)),
        ("prio_out", _z(F32, B_)), ("grad_coef", _z(F32, B_)),
        ("qmax_out", _z(F32, 1))]),
    "dueling_dqn_loss_bwd": (("g_adv",), lambda: [
        ("grad_coef", _z(F32, B_)), ("act", _z(I64, B_)),
        ("gout", _z(F32, 1)), ("g_adv", _z(F32, B_, A_)),
        ("g_val", _z(F32, B_))]),
    "dueling_q_loss_fwd": (("h_s",), lambda: [
        ("h_s", _bf(B_, 1024)), ("h_on", _bf(B_, 1024)),
        ("h_tg", _bf(B_, 1024)), *_qhead_heads(),
        *[(k + "_t", t) for k, t in _qhead_heads()], ("act", _z(I64, B_)),
        ("rew", _z(F32, B_)), ("done", _z(F32, B_)), ("w", _z(F32, B_)),
        0.97, 0.6, ("loss_out", _z(F32, 1)), ("prio_out", _z(F32, B_)),
        ("grad_coef", _z(F32, B_)), ("qmax_out", _z(F32, 1)), False]),
    "dueling_q_loss_bwd": (("h_s",), lambda: [
        ("grad_coef", _z(F32, B_)), ("act", _z(I64, B_)),
        ("gout", _z(F32, 1)), ("wa", _bf(6, 512)), ("wv", _bf(512)),
        ("h_s", _bf(B_, 1024)), ("dh", _bf(B_, 1024)), ("dwa", _bf(6, 512)),
        ("dba", _bf(6)), ("dwv", _bf(512)), ("dbv", _bf(1)), False]),
    "r2d2_loss_fwd": (("q_tgt",), lambda: [
        ("q_train", _z(F32, T_ - M_, B_, A_)), ("q_tgt", _z(F32, T_, B_, A_)),
        ("act", _z(I32, T_, B_)), ("rew", _z(F32, T_, B_)),
        ("done", _z(F32, B_)), ("w", _z(F32, B_)), M_, 3, 0.5, True,
        ("td_out", _z(F32, W_, B_)), ("stats", _z(F32, 3))]),
    "r2d2_prio": (("td",), lambda: [
        ("td", _z(F32, W_, B_)), 0.6, 0.9, ("prio", _z(F32, B_))]),
    "r2d2_loss_bwd": (("td", "dq"), lambda: [
        ("td", _z(F32, W_, B_)), ("act", _z(I32, T_, B_)),
        ("w", _z(F32, B_)), ("gout", _z(F32, 1)), T_, M_,
        ("dq", _z(F32, T_ - M_, B_, A_))]),
    "vtrace": (("rew",), lambda: [
        ("b_logp", _z(F32, T_, B_)), ("t_logp", _z(F32, T_, B_)),
        ("rew", _z(F32, T_, B_)), ("values", _z(F32, T_, B_)),
        ("boot", _z(F32, B_)), ("not_done", _z(F32, B_)), 0.99, 1.0, 1.0,
        1.0, ("vs", _z(F32, T_, B_)), ("pg_adv", _z(F32, T_, B_)),
        ("rho_out", _z(F32, T_, B_))]),
    "vtrace_bt": (("rew",), lambda: [
        ("mu", torch.ones(B_, T_, dtype=F32, device=DEV)),
        ("t_logp", _z(F32, B_, T_)), ("rew", _z(F32, B_, T_)),
        ("values", _z(F32, B_, T_)), ("boot", _z(F32, B_)),
        ("not_done", _z(F32, B_)), 0.99, 1.0, 1.0, 1.0,
        ("vs", _z(F32, B_, T_)), ("pg_adv", _z(F32, B_, T_))]),
    "policy_loss_fwd": (("logits",), lambda: [
        ("logits", _z(F32, B_, A_)), ("act", _z(I64, B_)),
        ("adv", _z(F32, B_)), 0.01, ("obj_out", _z(F32, 1)),
        ("ent_out", _z(F32, 1)), ("logpa_out", _z(F32, B_)),
        ("pi_save", _z(F32, B_, A_)), ("H_save", _z(F32, B_))]),
    "policy_loss_bwd": (("pi_save",), lambda: [
        ("pi_save", _z(F32, B_, A_)), ("H_save", _z(F32, B_)),
        ("act", _z(I64, B_)), ("adv", _z(F32, B_)), ("gout", _z(F32, 1)),
        0.01, 1.0, ("dlogits", _z(F32, B_, A_))]),
    "impala_loss_fwd": (("logpa",), lambda: [
        ("logpa", _z(F32, B_)), ("adv", _z(F32, B_)), ("mean_H", _z(F32, 1)),
        ("v", _z(F32, B_)), ("vs", _z(F32, B_)), 0.01,
        ("loss_out", _z(F32, 1)), ("obj_out", _z(F32, 1)),
        ("critic_out", _z(F32, 1))]),
    "impala_out_bwd": ((), lambda: [
        ("pi_save", _z(F32, B_ * T_, A_)), ("H_save", _z(F32, B_ * T_)),
        ("act", _z(I64, B_ * T_)), ("adv", _z(F32, B_ * T_)),
        ("v", _z(F32, B_ * T_)), ("vs", _z(F32, B_ * T_)),
        ("gloss", _z(F32, 1)), B_, T_, A_, 0.01,
        ("dout", _z(F32, B_ * (T_ + 1), A_ + 1))]),
    "value_rescale": (("x",), lambda: [
        ("x", _z(F32, 9)), ("y", _z(F32, 9)), 1e-3]),
    "inv_value_rescale": (("x",), lambda: [
        ("x", _z(F32, 9)), ("y", _z(F32, 9)), 1e-3]),
    "seq_priority": (("td_abs",), lambda: [
        ("td_abs", _z(F32, T_, B_)), 0.9, 0.6, ("out", _z(F32, B_))]),
    "grad_clip": (("flat",), lambda: [
        ("flat", _z(F32, 12)), 40.0, ("sqsum_buf", _z(F32, 1))]),
}


def _call(ext, name, args):
    getattr(ext, name)(*[a[1] if isinstance(a, tuple) else a for a in args])


@pytest.mark.parametrize("name", sorted(BINDINGS))
def test_binding_rejects_spoiled_arguments(ext, name):
    shape_args, make = BINDINGS[name]
    _call(ext, name, make())                    # the good call goes through
    torch.cuda.synchronize()
    tried = 0
    for i, a in enumerate(make()):
        if not isinstance(a, tuple):
            continue
        arg, good = a
        for label, bad in _spoils(good, arg in shape_args):
            args = make()
            args[i] = (arg, bad)
            with pytest.raises(RuntimeError, match=rf"\b{arg}\b"):
                _call(ext, name, args)
            tried += 1
    assert tried >= 6
    torch.cuda.synchronize()


def test_grad_clip_rejects_misaligned(ext):
    flat = _z(F32, 13)
    with pytest.raises(RuntimeError, match=r"\bflat\b.*aligned"):
        ext.grad_clip(flat[1:], 40.0, _z(F32, 1))


@pytest.mark.parametrize("arg", ["wa", "wa_t"])
def test_q_head_rejects_transposed_heads(ext, arg):
    """(512, 6) has the right count and is contiguous; it is still not the
    (6, 512) the kernel indexes."""
    args = BINDINGS["dueling_q_loss_fwd"][1]()
    i = [a[0] if isinstance(a, tuple) else None for a in args].index(arg)
    args[i] = (arg, _bf(512, 6))
    with pytest.raises(RuntimeError, match=rf"\b{arg}\b"):
        _call(ext, "dueling_q_loss_fwd", args)


@pytest.mark.parametrize("bad", [(-1, 3), (T_ - 1, 3), (M_, 0)])
def test_r2d2_rejects_bad_window(ext, bad):
    m, n = bad
    args = BINDINGS["r2d2_loss_fwd"][1]()
    args[6], args[7] = m, n
    with pytest.raises(RuntimeError):
        _call(ext, "r2d2_loss_fwd", args)
