"""The any-action-count q-head kernels (dueling_q_loss_any_*: bf16-MFMA heads,
fp32-MFMA head gradients, ordered folds) against the fp64 reference
torch_ref.dueling_q_head_loss_ref, at A in 2..18.

Rules and floors are those of test_gpu_losses.py's q-head family: upstream
gradient GOUT, floors 1 (sums), 1e-3 (prio), the largest reference gradient
(gradients); bf16 outputs after half a bf16 ulp. TOL is 4 x the error
measured on an MI355X over the cases of this file (docs/KERNELS.md).
"""

import copy
import functools
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
HH = 512

# name: 4 x e_gpu          e_gpu measured on an MI355X | e_32 (CPU fp32)
TOL = {
    "loss": 1.4e-07,        # 3.61e-08 | 4.04e-08
    "qmean": 5.0e-07,       # 1.26e-07 | 8.06e-08
    "prio": 9.5e-05,        # 2.37e-05 | 8.13e-05
    "dh": 1.1e-06,          # 2.65e-07 | 4.50e-07
    "dw": 3.9e-07,          # 9.80e-08 | 5.49e-07
}

# (A, B, pre_act): 16 | 17 straddle the second head block, 15 leaves one dead
# row; B: ragged tile, one tile, tile + 1, several blocks, > 1 pass per slice
CASES = [(2, 1, False), (2, 17, True), (3, 15, True), (6, 16, False),
         (6, 33, True), (15, 130, False), (16, 16, True), (16, 33, False),
         (17, 17, False), (17, 130, True), (18, 1, True), (18, 15, False),
         (18, 33, False), (18, 130, True)]


def _random(A, B, pre, seed):
    """LC.qhead_random at A heads."""
    g = LC._gen(23, A, B, pre, seed)

    def bf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF16).double()

    def heads():
        return (bf(A, HH, scale=0.05), bf(A, scale=0.1),
                bf(1, HH, scale=0.05), bf(1, scale=0.1))

    def hidden():
        h = bf(B, 2 * HH)
        return h if pre else torch.relu(h)

    online, target = heads(), heads()
    return NS(A=A, B=B, pre_act=pre, gamma=LC.RAND_GAMMA, n_step=LC.RAND_N,
              h=(hidden(), hidden(), hidden()), online=online, target=target,
              act=torch.randint(0, A, (B,), generator=g),
              rew=torch.randn(B, generator=g).double(),
              done=(torch.rand(B, generator=g) < 0.2).double(),
              w=(torch.rand(B, generator=g) + 0.1).float().double())


@functools.lru_cache(maxsize=None)
def random_case(A, B, pre):
    """First seed whose fp64 reference loses <= 5 % of the rows to the
    exclusion band; returns (case, fp64 ref, fp32 ref, excluded rows)."""
    for seed in range(32):
        c = _random(A, B, pre, seed)
        ref = LC.qhead_ref(c)
        out = LC.qhead_excluded(ref)
        if int(out.sum()) <= int(LC.EXCL_CAP * B):
            return c, ref, LC.qhead_ref(c, dtype=F32), out
    raise AssertionError("no seed under the exclusion cap")


TIES = {2: (0, 1), 16: (3, 15), 18: (15, 16)}   # 18: across the head blocks


@functools.lru_cache(maxsize=None)
def planted_case(A, pre):
    """Exact grid (heads in 1/64, hidden in 1/2, gamma^n = 1/2): every head
    dot is exact in fp32. Every third row ties TIES[A] at the top of the
    online s' row; its target row is ba_t alone, j / 4 per action, so a wrong
    a* moves the target by >= 1/8. Where 1/A is exact the rewards are solved
    for LC.RAW_PLAN (raw == +-1 among them); at A = 18 for raw = 1/4."""
    B = 33
    g = LC._gen(24, A, pre)
    done, w, raw_want = LC._row_plan(B, g)
    if A == 18:
        raw_want = torch.full((B,), 0.25, dtype=torch.float64)
    lo, hi = TIES[A]

    def heads():
        wa = LC._ints(g, -16, 16, A, HH) / 64.0
        wa[:, :8] = 0.0
        wa[[lo, hi], :8] = 0.25
        return (wa, torch.zeros(A, dtype=torch.float64),
                LC._ints(g, -16, 16, 1, HH) / 64.0, LC._ints(g, -8, 8, 1) / 64.0)

    online, target = heads(), heads()
    target = (target[0], torch.arange(A).double() / 4.0, *target[2:])
    h = [LC._grid_hidden(g, B, pre) for _ in range(3)]
    tie = torch.arange(B) % 3 == 0
    h[1][tie, :HH] = 0.0
    h[1][tie, :8] = 1.5
    h[2][tie, :HH] = 0.0
    c = NS(A=A, B=B, pre_act=pre, gamma=0.5, n_step=1, h=tuple(h),
           online=online, target=target, tie=tie, lo=lo,
           act=torch.randint(0, A, (B,), generator=g),
           rew=torch.zeros(B, dtype=torch.float64), done=done, w=w)
    c.rew = raw_want - LC.qhead_ref(c)["raw"]
    return c, LC.qhead_ref(c)


@pytest.fixture(scope="module")
def ops():
    from distributed_rl_amd import ops as _ops

    _ops.hip_ext(required=True)
    return _ops


def D(t, dtype=F32):
    return t.detach().to(dtype).to(DEV)


def on_device(c):
    leaves = [D(t, BF16).requires_grad_(True) for t in (c.h[0], *c.online)]
    rest = [D(t, BF16) for t in (c.h[1], c.h[2], *c.target)]
    return (leaves, rest + [D(c.act, I64), D(c.rew), D(c.done), D(c.w)],
            torch.tensor(LC.GOUT, dtype=F32, device=DEV))


def step(ops, c, leaves, rest, gout):
    loss, prio, qmean = ops.dueling_q_head_loss(
        *leaves, *rest, c.gamma, c.n_step, LC.ALPHA, pre_act=c.pre_act)
    grads = torch.autograd.grad(loss, leaves, gout)
    return [loss.detach(), prio, qmean, *grads]


def run(ops, c):
    out = step(ops, c, *on_device(c))
    torch.cuda.synchronize()
    return out


def hold(name, got, ref, floor, ref32=None, bf16=False):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().reshape(-1)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
    if ref.numel() == 0:
        return
    err = (got - ref).abs()
    if bf16:
        err = (err - LC.ulp_bf16(ref)).clamp_min(0.0)
    e = float((err / ref.abs().clamp_min(floor)).max())
    e32 = LC.rel_err(ref32, ref, floor) if ref32 is not None else float("nan")
    print(f"ERR qhead_any.{name} e_gpu={e:.3e} e_32={e32:.3e}")
    assert e <= TOL[name], (name, e, TOL[name])


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(
        a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def check_against_ref(got, ref, r32, keep, sums):
    loss, prio, qmean, dh = got[:4]
    r32 = r32 or {}
    hold("prio", prio.cpu()[keep], ref["prio"][keep], 1e-3,
         r32["prio"][keep] if r32 else None)
    hold("qmean", qmean, ref["qmean"], 1.0, r32.get("qmean"))
    dh_floor = float(ref["dh"].abs().max()) or 1.0
    hold("dh", dh.cpu()[keep], ref["dh"][keep], dh_floor,
         r32["dh"][keep] if r32 else None, bf16=True)
    if sums:    # sums over every row: only where no row may differ
        hold("loss", loss, ref["loss"], 1.0, r32.get("loss"))
        names = ("dwa", "dba", "dwv", "dbv")
        dw_floor = max(float(ref[k].abs().max()) for k in names) or 1.0
        for g, k in zip(got[4:], names):
            hold("dw", g.reshape(ref[k].shape), ref[k], dw_floor,
                 r32.get(k), bf16=True)


@pytest.mark.parametrize("A,B,pre", CASES, ids=[
    f"{a}-{b}-{'pre' if p else 'post'}" for a, b, p in CASES])
def test_values_and_grads(ops, monkeypatch, A, B, pre):
    """Every output against fp64, and two calls bit for bit (the loss and
    q-mean too: their folds are ordered)."""
    monkeypatch.setenv("DRL_QHEAD_ANY", "1")    # A = 6 on the new kernels
    c, ref, r32, out = random_case(A, B, pre)
    assert int(out.sum()) <= int(LC.EXCL_CAP * B)
    got, again = run(ops, c), run(ops, c)
    for a, b in zip(got, again):
        assert same_bits(a, b)
    check_against_ref(got, ref, r32, ~out, sums=not bool(out.any()))
    if pre:
        dead = c.h[0] <= 0
        assert bool((got[3].cpu()[dead] == 0).all())


@pytest.mark.parametrize("pre", [False, True], ids=["post", "pre"])
@pytest.mark.parametrize("A", sorted(TIES))
def test_planted_rows(ops, A, pre):
    c, ref = planted_case(A, pre)
    assert bool((ref["a_star"][c.tie] == c.lo).all())   # earliest index wins
    got = run(ops, c)
    dh = got[3].cpu().double()
    check_against_ref(got, ref, None, torch.ones(c.B, dtype=torch.bool), True)
    zero = ref["dh"] == 0
    assert bool(zero.any()) and bool((dh[zero] == 0).all())
    if A != 18:     # 1/A exact: raw sits on the clip bounds exactly
        on_bound = (ref["raw"].abs() == 1.0) & (c.w > 0)
        assert {-1.0, 1.0} <= set(ref["raw"][on_bound].tolist())
        assert bool((dh[on_bound].abs().sum(dim=1) > 0).all())
        assert bool(((c.w == 0) & (ref["dh"].abs().sum(dim=1) == 0)).any())
    if pre:
        dead = c.h[0] <= 0
        assert bool((c.h[0] == 0).logical_and(torch.signbit(c.h[0])).any())
        assert bool((dh[dead] == 0).all())


def test_gate_at_six(ops, monkeypatch):
    """DRL_QHEAD_ANY=1 sends A = 6 to the new kernels, which agree with the
    (512, 6) ones; unset, the op is the old bindings bit for bit."""
    c = LC.qhead_random(33, True, 0)
    monkeypatch.delenv("DRL_QHEAD_ANY", raising=False)
    old = run(ops, c)
    ext = ops.hip_ext()
    t = [D(x, BF16) for x in (c.h[0], c.h[1], c.h[2], *c.online, *c.target)]
    t[5], t[9] = t[5].reshape(-1), t[9].reshape(-1)
    acc, prio, coef = (torch.zeros(2, device=DEV), torch.empty(33, device=DEV),
                       torch.empty(33, device=DEV))
    ext.dueling_q_loss_fwd(*t, D(c.act, I64), D(c.rew), D(c.done), D(c.w),
                           c.gamma ** c.n_step, LC.ALPHA, acc[0:1], prio, coef,
                           acc[1:2], True)
    torch.cuda.synchronize()
    assert same_bits(old[1], prio)
    monkeypatch.setenv("DRL_QHEAD_ANY", "1")
    new = run(ops, c)
    ref = {k: v.detach().double().cpu() for k, v in zip(
        ("loss", "prio", "qmean", "dh", "dwa", "dba", "dwv", "dbv"), old)}
    ref["dwv"], keep = ref["dwv"].reshape(1, HH), torch.ones(33, dtype=bool)
    check_against_ref(new, ref, None, keep, sums=True)


def _z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _good_args(A=18, B=5):
    heads = [_z(BF16, A, HH), _z(BF16, A), _z(BF16, HH), _z(BF16, 1)]
    h, f, act = _z(BF16, B, 1024), _z(F32, B), _z(I64, B)
    fwd = dict(zip(
        "h_s h_on h_tg wa ba wv bv wa_t ba_t wv_t bv_t act rew done w gamma_n "
        "alpha loss_out prio_out grad_coef qmax_out pre_act".split(),
        [h, h, h, *heads, *heads, act, f, f, f, 0.97, 0.6, _z(F32, 1),
         _z(F32, B), _z(F32, B), _z(F32, 1), False]))
    bwd = dict(zip(
        "grad_coef act gout wa wv h_s dh dwa dba dwv dbv pre_act".split(),
        [f, act, _z(F32, 1), heads[0], heads[2], h, _z(BF16, B, 1024),
         *(torch.zeros_like(t) for t in heads), False]))
    return {"fwd": fwd, "bwd": bwd}


def _bf_view(rows, cols, skip=0):
    buf = torch.zeros(2 * rows * cols + 8, dtype=BF16, device=DEV)
    return buf[skip:skip + rows * cols].view(rows, cols)


SPOILS = {
    "A=1": ("fwd", "wa", lambda: _bf_view(1, HH)),
    "A=19": ("bwd", "wa", lambda: _bf_view(19, HH)),
    "wa_t other A": ("fwd", "wa_t", lambda: _bf_view(17, HH)),
    "wa transposed": ("fwd", "wa", lambda: _bf_view(HH, 18)),
    "host rew": ("fwd", "rew", lambda: torch.zeros(5)),
    "dba short": ("bwd", "dba", lambda: _bf_view(1, 17).view(17)),
    "h_s misaligned": ("fwd", "h_s", lambda: _bf_view(5, 1024, skip=1)),
}


@pytest.mark.parametrize("label", sorted(SPOILS))
def test_binding_rejects(ops, label):
    which, arg, make = SPOILS[label]
    ext = ops.hip_ext()
    fn = getattr(ext, f"dueling_q_loss_any_{which}")
    fn(*_good_args()[which].values())       # the good call goes through
    args = _good_args()[which]
    args[arg] = make()
    with pytest.raises(RuntimeError, match=rf"\b{arg}\b"):
        fn(*args.values())
    torch.cuda.synchronize()
    assert ext.dueling_q_loss_any_supported(512, 18)
    assert not ext.dueling_q_loss_any_supported(512, 19)
    assert not ext.dueling_q_loss_any_supported(256, 6)


def test_learner_at_18_actions(ops):
    """ACTION_SIZE = 18 takes the grouped-conv, pre-activation, fused-head
    branch; its loss and priorities are those of the Linear heads +
    dueling_nstep_dqn_loss composition on the same hidden rows."""
    import torch.nn.functional as F

    from distributed_rl_amd.algos.ape_x import ApexLearner
    from distributed_rl_amd.config import Config, load_config

    raw = copy.deepcopy(load_config("ape_x").raw)
    raw["ACTION_SIZE"] = 18
    raw["model"]["module02"]["fSize"] = [512, 18]
    raw["REPLAY_MEMORY_LEN"], raw["BATCHSIZE"] = 1024, 32
    learner = ApexLearner(Config(raw=raw), device=DEV, enable_tb=False)
    assert learner._use_q_loss
    n = 256
    frames = lambda: torch.randint(  # noqa: E731
        0, 256, (n, 4, 84, 84), dtype=torch.uint8, device=DEV)
    learner.push_experience({
        "state": frames(), "next_state": frames(),
        "action": torch.randint(0, 18, (n,), dtype=torch.int32, device=DEV),
        "reward": torch.rand(n, device=DEV),
        "done": (torch.rand(n, device=DEV) < 0.1).float(),
    }, torch.rand(n, device=DEV) + 0.1)
    data, _, w = learner.replay.sample(32, learner.beta)
    stats, prio = learner._fwd_bwd(data, w)

    sp = data["next_state"].permute(0, 3, 1, 2)
    with torch.no_grad():
        hs = (learner._fast_hidden(data["state"].permute(0, 3, 1, 2)),
              learner._fast_hidden(sp), learner._target_hidden(sp))
        heads = []
        for h, p in zip(hs, (learner._head_params, learner._head_params,
                             learner._thead_params)):
            wa, ba, wv, bv = (t.double() for t in p)
            heads += [F.linear(h[:, :HH].double(), wa, ba).float(),
                      F.linear(h[:, HH:].double(), wv, bv).float()]
        loss2, prio2, _ = ops.dueling_nstep_dqn_loss(
            *heads, data["action"].long(), data["reward"], data["done"], w,
            learner.gamma, learner.n_step, learner.alpha)
    torch.cuda.synchronize()
    hold("loss", stats["loss"], loss2.cpu(), 1.0)
    hold("prio", prio, prio2.cpu(), 1e-3)


def test_graph_replay_matches_eager(ops):
    """Forward + backward of the op at A = 18, B = 32 captured in one graph;
    a replay gives the eager call's bits. Last in the file."""
    c = random_case(18, 33, False)[0]
    c = NS(**{**vars(c), "h": tuple(h[:32] for h in c.h), "act": c.act[:32],
              "rew": c.rew[:32], "done": c.done[:32], "w": c.w[:32]})
    eager, dev = run(ops, c), on_device(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(ops, c, *dev)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(ops, c, *dev)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert same_bits(a, b)
