"""Ape-X step fusions: grouped conv forward, bf16 weight-grad store,
pre-activation head loss, optimizer tail in one pass. Each is arithmetic-
preserving (same operations on the same values in the same order), so every
check against the unfused path is bit-exact (torch.equal) except the two
atomically accumulated batch means of the head loss."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (H, W, C, KH, KW, S, COUT) — same table as tests/test_gpu_conv.py
SHAPES = [
    (84, 84, 4, 8, 8, 4, 32),
    (20, 20, 32, 4, 4, 2, 64),
    (9, 9, 64, 3, 3, 1, 64),
    (84, 84, 4, 8, 8, 4, 16),
    (20, 20, 16, 4, 4, 2, 32),
]
APEX_SHAPES = SHAPES[:3]


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _cl(t):
    return t.to(memory_format=torch.channels_last)


def _conv_inputs(shape, N, u8, njobs, seed):
    """njobs jobs with different weights; jobs 1 and 2 share one input."""
    H, W, C, KH, KW, S, COUT = shape
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)

    def mkx():
        if u8:
            return _cl(torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8,
                                     device=DEV, generator=g))
        return _cl(torch.randn(N, C, H, W, device=DEV, generator=g
                               ).to(torch.bfloat16))

    x0, x1 = mkx(), mkx()
    xs = [x0, x1, x1][:njobs]
    ws = [_cl((torch.randn(COUT, C, KH, KW, device=DEV, generator=g) * 0.1
               ).to(torch.bfloat16)) for _ in range(njobs)]
    bs = [(torch.randn(COUT, device=DEV, generator=g) * 0.1
           ).to(torch.bfloat16) for _ in range(njobs)]
    return xs, ws, bs


# ---------------------------------------------------------------------------
# grouped conv forward
# ---------------------------------------------------------------------------

# conv3 at N=3 / N=33: M = 147 (one ragged block per job) / 1617 (several
# blocks, ragged last); conv1 at N=3: M = 1200
GROUPED_CASES = [
    # (shape, u8, chw_out)
    (APEX_SHAPES[0], True, False),
    (APEX_SHAPES[0], False, False),
    (APEX_SHAPES[1], False, False),
    (APEX_SHAPES[2], False, False),
    (APEX_SHAPES[2], False, True),
]


@pytest.mark.parametrize("njobs", [1, 2, 3])
@pytest.mark.parametrize("N", [3, 33])
@pytest.mark.parametrize("case", GROUPED_CASES,
                         ids=lambda c: f"{c[0][0]}x{c[0][2]}-u8{int(c[1])}"
                                       f"-chw{int(c[2])}")
def test_grouped_conv_fwd_bit_identical(ext, case, N, njobs):
    shape, u8, chw = case
    H, W, C, KH, KW, S, COUT = shape
    P, Q = (H - KH) // S + 1, (W - KW) // S + 1
    xs, ws, bs = _conv_inputs(shape, N, u8, njobs, seed=100 + N + njobs)
    from distributed_rl_amd import ops

    refs = [ops.fused_conv_relu(x, w, b, S, chw_out=chw)
            for x, w, b in zip(xs, ws, bs)]
    # raw binding on NaN-prefilled outputs: every element must be written
    if chw:
        outs = [torch.full((N, COUT * P * Q), float("nan"),
                           dtype=torch.bfloat16, device=DEV)
                for _ in range(njobs)]
    else:
        outs = [_cl(torch.full((N, COUT, P, Q), float("nan"),
                               dtype=torch.bfloat16, device=DEV))
                for _ in range(njobs)]
    ext.conv_fwd_grouped(xs, ws, bs, outs, S, chw)
    got = ops.fused_conv_relu_grouped(xs, ws, bs, S, chw_out=chw)
    torch.cuda.synchronize()
    for j in range(njobs):
        assert not torch.isnan(outs[j].float()).any(), j
        assert torch.equal(outs[j], refs[j]), j
        assert torch.equal(got[j], refs[j]), j


def test_grouped_conv_rejects_mixed_batch(ext):
    shape = APEX_SHAPES[2]
    xs, ws, bs = _conv_inputs(shape, 3, False, 2, seed=7)
    xs[1] = _cl(torch.zeros(4, 64, 9, 9, dtype=torch.bfloat16, device=DEV))
    outs = [_cl(torch.empty(3, 64, 7, 7, dtype=torch.bfloat16, device=DEV))
            for _ in range(2)]
    with pytest.raises(RuntimeError):
        ext.conv_fwd_grouped(xs, ws, bs, outs, 1, False)


@pytest.mark.parametrize("case", GROUPED_CASES[1:],
                         ids=lambda c: f"{c[0][0]}x{c[0][2]}-chw{int(c[2])}")
def test_grouped_conv_backward_job0_only(ext, case):
    """Job 0 differentiable (x, w, b); jobs 1 and 2 on plain tensors: their
    outputs carry no graph and their inputs get no grads."""
    shape, _, chw = case
    S = shape[5]
    N = 33
    from distributed_rl_amd import ops

    xs, ws, bs = _conv_inputs(shape, N, False, 3, seed=11)
    leaves = [t.detach().clone().requires_grad_(True)
              for t in (xs[0], ws[0], bs[0])]
    ref_leaves = [t.detach().clone().requires_grad_(True)
                  for t in (xs[0], ws[0], bs[0])]
    outs = ops.fused_conv_relu_grouped(
        [leaves[0], xs[1], xs[2]], [leaves[1], ws[1], ws[2]],
        [leaves[2], bs[1], bs[2]], S, chw_out=chw)
    ref = ops.fused_conv_relu(*ref_leaves, S, chw_out=chw)
    assert outs[0].requires_grad
    assert not outs[1].requires_grad and not outs[2].requires_grad
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    gout = torch.randn(ref.shape, device=DEV, generator=g).to(torch.bfloat16)
    if not chw:
        gout = _cl(gout)
    outs[0].backward(gout)
    ref.backward(gout)
    torch.cuda.synchronize()
    for a, b in zip(leaves, ref_leaves):
        assert torch.equal(a.grad, b.grad)
    for t in (xs[1], ws[1], bs[1], ws[2], bs[2]):
        assert t.grad is None


def test_cnn2d_forward_grouped_matches_modules():
    import copy

    from distributed_rl_amd.config import load_config
    from distributed_rl_amd.models.base_agent import CNN2D

    cfg = load_config("ape_x")
    torch.manual_seed(2)
    info = next(c for c in cfg.model_info.values()
                if str(c.get("netCat", "")).upper() == "CNN2D")
    online = CNN2D(info).to(DEV).to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    target = copy.deepcopy(online)
    with torch.no_grad():
        for p in target.parameters():
            p.mul_(0.5)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    s, sp = (_cl(torch.randint(0, 256, (3, 4, 84, 84), dtype=torch.uint8,
                               device=DEV, generator=g)) for _ in range(2))
    assert online._grouped_ok(s)
    f = CNN2D.forward_grouped([(s, online, True), (sp, online, False),
                               (sp, target, False)])
    with torch.no_grad():
        refs = [online(s), online(sp), target(sp)]
    assert f[0].requires_grad and not f[1].requires_grad \
        and not f[2].requires_grad
    for a, b in zip(f, refs):
        assert a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------
# weight-grad reduce writing bf16
# ---------------------------------------------------------------------------


def _wrw_pair(ext, x, gout, shape, with_bias):
    H, W, C, KH, KW, S, COUT = shape
    ws = torch.zeros(COUT, KH * KW * C, dtype=torch.float32, device=DEV)
    gb_ws = (torch.zeros(COUT, dtype=torch.float32, device=DEV) if with_bias
             else torch.empty(0, device=DEV))
    ext.conv_wrw(x, gout, ws, gb_ws, S)
    gw = torch.full((COUT, KH, KW, C), float("nan"), dtype=torch.bfloat16,
                    device=DEV).permute(0, 3, 1, 2)
    gb = (torch.full((COUT,), float("nan"), dtype=torch.bfloat16, device=DEV)
          if with_bias else torch.empty(0, device=DEV))
    ext.conv_wrw(x, gout, gw, gb, S)
    torch.cuda.synchronize()
    ref_w = ws.view(COUT, KH, KW, C).permute(0, 3, 1, 2).to(torch.bfloat16)
    assert not torch.isnan(gw.float()).any()
    assert torch.equal(gw, ref_w)
    assert gw.is_contiguous(memory_format=torch.channels_last)
    if with_bias:
        assert torch.equal(gb, gb_ws.to(torch.bfloat16))


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_wrw_bf16_out_equals_cast(ext, shape):
    H, W, C, KH, KW, S, COUT = shape
    torch.manual_seed(5)
    N = 5
    P, Q = (H - KH) // S + 1, (W - KW) // S + 1
    x = _cl(torch.randn(N, C, H, W, device=DEV).to(torch.bfloat16))
    gout = _cl(torch.randn(N, COUT, P, Q, device=DEV).to(torch.bfloat16))
    _wrw_pair(ext, x, gout, shape, with_bias=True)


def test_conv_wrw_bf16_out_u8_input(ext):
    torch.manual_seed(6)
    shape = SHAPES[0]
    N = 5
    x = _cl(torch.randint(0, 256, (N, 4, 84, 84), dtype=torch.uint8,
                          device=DEV))
    gout = _cl(torch.randn(N, 32, 20, 20, device=DEV).to(torch.bfloat16))
    _wrw_pair(ext, x, gout, shape, with_bias=False)
    _wrw_pair(ext, x, gout, shape, with_bias=True)


# ---------------------------------------------------------------------------
# pre-activation head loss
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("B", [5, 64])
def test_preact_head_loss_equals_relu_then_loss(B):
    from distributed_rl_amd import ops

    torch.manual_seed(41 + B)
    HH, A = 512, 6

    def mkz():
        z = (torch.randn(B, 2 * HH, device=DEV) * 0.5).to(torch.bfloat16)
        z[:, 3] = 0.0
        z[:, HH + 7] = -0.0
        z[0, :16] = 0.0
        return z

    z_s, z_on, z_tg = mkz(), mkz(), mkz()
    assert 0.4 < (z_s.float() < 0).float().mean() < 0.6

    def mk(*shape, s):
        return (torch.randn(*shape, device=DEV) * s).to(torch.bfloat16)

    wa, ba, wv, bv = mk(A, HH, s=0.05), mk(A, s=0.1), mk(1, HH, s=0.05), \
        mk(1, s=0.1)
    wat, bat, wvt, bvt = mk(A, HH, s=0.05), mk(A, s=0.1), mk(1, HH, s=0.05), \
        mk(1, s=0.1)
    actions = torch.randint(0, A, (B,), device=DEV)
    rewards = torch.randn(B, device=DEV)
    dones = (torch.rand(B, device=DEV) < 0.1).float()
    weights = torch.rand(B, device=DEV) + 0.5

    def run(h_s, h_on, h_tg, pre):
        h = h_s.detach().clone().requires_grad_(True)
        ps = [p.detach().clone().requires_grad_(True)
              for p in (wa, ba, wv, bv)]
        loss, prio, qm = ops.dueling_q_head_loss(
            h, *ps, h_on, h_tg, wat, bat, wvt, bvt, actions, rewards, dones,
            weights, 0.99, 3, 0.6, pre_act=pre)
        loss.backward()
        return loss.detach(), prio, qm, h.grad, [p.grad for p in ps]

    new = run(z_s, z_on, z_tg, True)
    old = run(F.relu(z_s), F.relu(z_on), F.relu(z_tg), False)
    torch.cuda.synchronize()
    assert torch.equal(new[1], old[1])  # prio
    # loss / qmean: float atomics over the batch in hardware order — the
    # tolerance of tests/test_bench_cli.py::test_dump_outputs_reproducible_on_gpu
    print("loss", float(new[0]), float(old[0]), "qmean", float(new[2]),
          float(old[2]))
    assert torch.allclose(new[0], old[0], rtol=1e-4, atol=1e-5)
    assert torch.allclose(new[2], old[2], rtol=1e-4, atol=1e-5)
    mask = (z_s > 0).to(old[3].dtype)
    assert torch.equal(new[3], old[3] * mask)
    for a, b in zip(new[4], old[4]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# optimizer tail in one pass
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("centered", [True, False])
def test_rmsprop_fused_tail_bit_identical(ext, centered, momentum, grad_scale):
    n = 2100  # not a multiple of the vector width or the block size
    torch.manual_seed(9)
    lr, alpha, eps, wd = 1e-2, 0.95, 1.5e-7, 1e-3

    def state():
        torch.manual_seed(10)
        p = torch.randn(n, device=DEV)
        sq = torch.zeros(n, device=DEV)
        ga = torch.zeros(n, device=DEV) if centered else torch.empty(0)
        mom = torch.zeros(n, device=DEV) if momentum > 0 else torch.empty(0)
        return p, sq, ga, mom

    pa, sqa, gaa, moma = state()
    pb, sqb, gab, momb = state()
    shadow_a = torch.full((n,), float("nan"), dtype=torch.bfloat16,
                          device=DEV)
    shadow_b = torch.full((n,), float("nan"), dtype=torch.bfloat16,
                          device=DEV)
    mgrad = torch.empty(n, device=DEV)
    for step in range(4):
        g16 = (torch.randn(n, device=DEV) * 0.1).to(torch.bfloat16)
        # reference: upcast (+ scale) -> rmsprop_step -> copy_
        mgrad.copy_(g16)
        if grad_scale != 1.0:
            mgrad.mul_(grad_scale)
        ext.rmsprop_step(pa, mgrad, sqa, gaa, moma, lr, alpha, eps, wd,
                         momentum, centered, momentum > 0)
        shadow_a.copy_(pa)
        # fused
        ext.rmsprop_step(pb, pb, sqb, gab, momb, lr, alpha, eps, wd,
                         momentum, centered, momentum > 0, g_bf16=g16,
                         grad_scale=grad_scale, p_bf16=shadow_b)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb)
    assert torch.equal(sqa, sqb)
    if centered:
        assert torch.equal(gaa, gab)
    if momentum > 0:
        assert torch.equal(moma, momb)
    assert torch.equal(shadow_a, shadow_b)


# ---------------------------------------------------------------------------
# learner level: every new path on vs every gate forced to the old path
# ---------------------------------------------------------------------------

GATES = ("DRL_GROUPED_CONV", "DRL_WRW_BF16", "DRL_PREACT_LOSS",
         "DRL_FUSED_OPT_TAIL")


def _run_learner(steps=3):
    from distributed_rl_amd.algos.ape_x import ApexLearner
    from distributed_rl_amd.config import load_config

    torch.manual_seed(123)
    learner = ApexLearner(load_config("ape_x"), device=DEV, enable_tb=False,
                          batch_size=8, replay_capacity=256)
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    B = 256
    cols = {
        "state": torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8,
                               device=DEV, generator=g),
        "action": torch.randint(0, 6, (B,), dtype=torch.int32, device=DEV,
                                generator=g),
        "reward": torch.rand(B, device=DEV, generator=g),
        "next_state": torch.randint(0, 256, (B, 4, 84, 84),
                                    dtype=torch.uint8, device=DEV,
                                    generator=g),
        "done": (torch.rand(B, device=DEV, generator=g) < 0.1).float(),
    }
    learner.push_experience(cols, torch.rand(B, device=DEV, generator=g) + 0.1)
    for _ in range(steps):
        learner.step()
    torch.cuda.synchronize()
    return (learner.mp.flat_mparam.clone(), learner.mp.flat_cparam.clone(),
            [t.clone() for t in learner.optim.sq + learner.optim.ga])


def test_learner_new_paths_bit_identical_to_old(monkeypatch):
    for k in GATES:
        monkeypatch.setenv(k, "1")
    new = _run_learner()
    for k in GATES:
        monkeypatch.setenv(k, "0")
    old = _run_learner()
    assert torch.equal(new[0], old[0])
    assert torch.equal(new[1], old[1])
    for a, b in zip(new[2], old[2]):
        assert torch.equal(a, b)
    # the steps did train: the second-moment state left its zero init
    assert float(new[2][0].abs().sum()) > 0
