"""Own weight- and input-gradient kernels of the 3x3 pad-1 ResNet convs
(conv3x3p1_wrw_kernel; conv3x3p1_fwd_kernel at the mirrored geometry with the
flipped weight and the masked epilogue) against aten.convolution_backward in
float64 on the CPU, from bf16-rounded operands.

N=3 makes M = 5292 / 1323 / 363 rows: never a multiple of the 32-row chunk
or of a block's 64- or 128-row pass, several m-slices and a ragged tail. N=1
at 11x11 (M = 121) is fewer passes than an m-slice is sized for: one block.
"""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16

# (H, W, C, COUT, N)
CASES = [
    (42, 42, 16, 16, 3),
    (42, 42, 16, 32, 3),
    (21, 21, 32, 32, 3),
    (11, 11, 32, 32, 3),
    (11, 11, 32, 32, 1),
]
IDS = ["x".join(map(str, c)) for c in CASES]


def _cl(t):
    return t.to(BF16).contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def data(ext):
    """Per case: bf16-rounded x, gout, w on the device and the float64 CPU
    reference gradients, built once and never written."""
    out = {}
    gen = torch.Generator().manual_seed(23)
    for (H, W, C, COUT, n) in CASES:
        x = torch.randn(n, C, H, W, generator=gen).to(BF16)
        g = torch.randn(n, COUT, H, W, generator=gen).to(BF16)
        w = (torch.randn(COUT, C, 3, 3, generator=gen) * 0.05).to(BF16)
        gx, gw, gb = torch.ops.aten.convolution_backward(
            g.double(), x.double(), w.double(), [COUT], [1, 1], [1, 1],
            [1, 1], False, [0, 0], 1, [True, True, True])
        out[(H, W, C, COUT, n)] = dict(
            x=_cl(x.to(DEV)), g=_cl(g.to(DEV)), w=_cl(w.to(DEV)),
            gx=gx, gb=gb,
            # (cout, kh, kw, c): the kernel's K order
            gw=gw.permute(0, 2, 3, 1).reshape(COUT, 9 * C))
    return out


def _wrw(ext, x, g, dtype=torch.float32, bias=True, relu_in=False):
    COUT, C = g.shape[1], x.shape[1]
    gw = torch.full((COUT, 9 * C), float("nan"), dtype=dtype, device=DEV)
    gb = (torch.full((COUT,), float("nan"), dtype=dtype, device=DEV) if bias
          else torch.empty(0, device=DEV))
    ext.conv3x3p1_wrw(x, g, gw, gb, relu_in)
    return gw, gb


def _dgrad(ext, g, w, mask=None):
    n, _, H, W = g.shape
    gx = _cl(torch.full((n, w.shape[1], H, W), float("nan"), device=DEV))
    ws = torch.empty(w.numel(), dtype=BF16, device=DEV)
    ext.conv3x3p1_dgrad(g, w, ws, gx,
                        mask if mask is not None
                        else torch.empty(0, dtype=BF16, device=DEV))
    return gx


def _between_nans(t):
    """t as a slice of one allocation with a NaN image on either side."""
    big = torch.full((t.shape[0] + 2, *t.shape[1:]), float("nan"), device=DEV,
                     dtype=BF16).contiguous(memory_format=torch.channels_last)
    big[1:-1] = t
    s = big[1:-1]
    assert s.is_contiguous(memory_format=torch.channels_last)
    assert s.data_ptr() != big.data_ptr()
    return s


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrw_fp32_vs_fp64(ext, data, case):
    """fp32 sums over 32-row chunks, planes folded in order: 1.5e-7 of
    max|ref| from fp64 in a CPU simulation; 1e-5 leaves room for another
    order."""
    d = data[case]
    gw, gb = _wrw(ext, d["x"], d["g"])
    for name, got, ref in [("gw", gw, d["gw"]), ("gb", gb, d["gb"])]:
        err = (got.double().cpu() - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{case} {name}: max err {err:.4g} / max ref {scale:.4g} "
              f"= {err / scale:.3g}")
        assert err <= 1e-5 * scale, f"{case} {name}: {err} vs {scale}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrw_bf16_output(ext, data, case):
    """Same partials, order and rounding as the fp32 workspace path."""
    d = data[case]
    gw32, gb32 = _wrw(ext, d["x"], d["g"])
    gw16, gb16 = _wrw(ext, d["x"], d["g"], dtype=BF16)
    assert torch.equal(gw16, gw32.to(BF16))
    assert torch.equal(gb16, gb32.to(BF16))
    # a channels_last weight-shaped gradient tensor takes the same bytes
    COUT, C = case[3], case[2]
    gw4 = torch.empty(COUT, 3, 3, C, dtype=BF16, device=DEV).permute(0, 3, 1, 2)
    ext.conv3x3p1_wrw(d["x"], d["g"], gw4, torch.empty(0, device=DEV), False)
    assert torch.equal(gw4.permute(0, 2, 3, 1).reshape(COUT, 9 * C), gw16)
    ref = d["gw"]
    diff = (gw16.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max()
    print(f"{case} bf16 gw: max diff/bound {(diff / bound).max().item():.3g}")
    assert (diff <= bound).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrw_exact_borders(ext, case):
    """All-ones x and gout: gw[co][kh][kw][c] counts the samples whose tap
    is inside the image — integers below 2^24, exact in fp32."""
    H, W, C, COUT, n = case
    x = _cl(torch.ones(n, C, H, W, device=DEV))
    g = _cl(torch.ones(n, COUT, H, W, device=DEV))
    gw, gb = _wrw(ext, x, g)
    k = torch.arange(3, device=DEV)
    cnt = n * (H - (k - 1).abs())[:, None] * (W - (k - 1).abs())[None, :]
    expect = cnt.float()[None, :, :, None].expand(COUT, 3, 3, C)
    assert expect[0, 1, 1, 0] == n * H * W
    assert expect[0, 0, 2, 0] == n * (H - 1) * (W - 1)
    assert torch.equal(gw.view(COUT, 3, 3, C), expect)
    assert torch.equal(gb, torch.full_like(gb, n * H * W))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrw_no_halo_reads(ext, data, case):
    d = data[case]
    gw, gb = _wrw(ext, _between_nans(d["x"]), _between_nans(d["g"]))
    plain = _wrw(ext, d["x"].clone(memory_format=torch.channels_last),
                 d["g"].clone(memory_format=torch.channels_last))
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    assert torch.equal(gw, plain[0]) and torch.equal(gb, plain[1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrw_relu_in_identity(ext, data, case):
    d = data[case]
    a, _ = _wrw(ext, d["x"], d["g"], bias=False, relu_in=True)
    b, _ = _wrw(ext, torch.relu(d["x"]), d["g"], bias=False, relu_in=False)
    assert torch.equal(a, b)
    # and it does change the result
    c, _ = _wrw(ext, d["x"], d["g"], bias=False, relu_in=False)
    assert not torch.equal(a, c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrw_deterministic(ext, data, case):
    d = data[case]
    a = _wrw(ext, d["x"], d["g"])
    b = _wrw(ext, d["x"], d["g"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# The m-grid is the smallest of passes/8, 16 MiB of planes and the resident
# blocks; CASES stay on the first (21 / 6 / 3 / 2 / 1 blocks). These two reach
# the other two: 11x11x32->32 at N=960 is 3630 passes -> 454 > the 451 planes
# of 37120 B that fit 16 MiB; 42x42x16->16 at N=192 is 10584 passes -> 1323 >
# the 1280 blocks (5 per CU x 256 CUs) resident on an MI355X.
BIG = [(11, 11, 32, 32, 960), (42, 42, 16, 16, 192)]


@pytest.mark.parametrize("case", BIG, ids=["x".join(map(str, c)) for c in BIG])
def test_wrw_capped_m_grid(ext, case):
    """Same bounds as test_wrw_fp32_vs_fp64, plus determinism and the bf16
    store, where the plane budget or the residency caps the m-grid."""
    H, W, C, COUT, n = case
    gen = torch.Generator().manual_seed(29)
    x = torch.randn(n, C, H, W, generator=gen).to(BF16)
    g = torch.randn(n, COUT, H, W, generator=gen).to(BF16)
    _, ref_gw, ref_gb = torch.ops.aten.convolution_backward(
        g.double(), x.double(), torch.zeros(COUT, C, 3, 3, dtype=torch.double),
        [COUT], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True])
    ref_gw = ref_gw.permute(0, 2, 3, 1).reshape(COUT, 9 * C)
    xd, gd = _cl(x.to(DEV)), _cl(g.to(DEV))
    gw, gb = _wrw(ext, xd, gd)
    for name, got, ref in [("gw", gw, ref_gw), ("gb", gb, ref_gb)]:
        err = (got.double().cpu() - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{case} {name}: max err {err:.4g} / max ref {scale:.4g} "
              f"= {err / scale:.3g}")
        assert err <= 1e-5 * scale, f"{case} {name}: {err} vs {scale}"
    again = _wrw(ext, xd, gd)
    assert torch.equal(gw, again[0]) and torch.equal(gb, again[1])
    gw16, gb16 = _wrw(ext, xd, gd, dtype=BF16)
    assert torch.equal(gw16, gw.to(BF16)) and torch.equal(gb16, gb.to(BF16))


# ---------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad_equals_forward_of_flipped_weight(ext, data, case):
    from distributed_rl_amd import ops

    d = data[case]
    gx = _dgrad(ext, d["g"], d["w"])
    # W'[ci][co][kh][kw] = W[co][ci][2-kh][2-kw]
    w_host = _cl(d["w"].flip(2, 3).transpose(0, 1))
    assert torch.equal(gx, ops.fused_conv3x3(d["g"], w_host, None))
    # the forward's criterion against the float64 gradient
    err = (gx.double().cpu() - d["gx"]).abs().max().item()
    scale = d["gx"].abs().max().item()
    print(f"{case} gx: max err {err:.4g} / max ref {scale:.4g} "
          f"= {err / scale:.3g}")
    assert err / scale < 2e-2
    # masked epilogue == relu_mask_bwd of the unmasked result
    masked = _dgrad(ext, d["g"], d["w"], mask=d["x"])
    expect = torch.empty_like(gx)
    ext.relu_mask_bwd(gx, d["x"], expect)
    assert torch.equal(masked, expect)
    assert not torch.equal(masked, gx)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad_no_halo_reads(ext, data, case):
    d = data[case]
    gx = _dgrad(ext, _between_nans(d["g"]), d["w"], mask=_between_nans(d["x"]))
    plain = _dgrad(ext, d["g"].clone(memory_format=torch.channels_last),
                   d["w"], mask=d["x"])
    assert torch.isfinite(gx.float()).all()
    assert torch.equal(gx, plain)


# the forward checks of test_gpu_resconv.py for the new instantiation
G_NEW = (42, 42, 32, 16)
N_FWD = 3


def test_new_forward_vs_fp32():
    from distributed_rl_amd import ops
    from distributed_rl_amd.ops import torch_ref

    H, W, C, COUT = G_NEW
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = _cl(torch.randn(N_FWD, C, H, W, device=DEV, generator=gen))
    w = _cl(torch.randn(COUT, C, 3, 3, device=DEV, generator=gen) * 0.05)
    b = (torch.randn(COUT, device=DEV, generator=gen) * 0.1).to(BF16)
    r = _cl(torch.randn(N_FWD, COUT, H, W, device=DEV, generator=gen))
    for name, kw in [("plain", {}),
                     ("relu_in+relu_out", dict(relu_in=True, relu_out=True)),
                     ("residual", dict(residual=r))]:
        out = ops.fused_conv3x3(x, w, b, **kw)
        ref = torch_ref.conv3x3_res(
            x.float(), w.float(), b.float(), kw.get("relu_in", False),
            kw.get("relu_out", False),
            r.float() if "residual" in kw else None)
        assert out.shape == ref.shape and out.dtype == BF16
        assert out.is_contiguous(memory_format=torch.channels_last)
        err = (out.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{G_NEW} {name}: max err {err:.4g} / max ref {scale:.4g} "
              f"= {err / scale:.3g}")
        assert err / scale < 2e-2, f"{name}: {err} vs {scale}"


def test_new_forward_exact_border_count():
    """All-ones input and weights: out = C x (in-bounds taps), exactly."""
    from distributed_rl_amd import ops

    H, W, C, COUT = G_NEW
    x = _cl(torch.ones(N_FWD, C, H, W, device=DEV))
    w = _cl(torch.ones(COUT, C, 3, 3, device=DEV))
    out = ops.fused_conv3x3(x, w, None)
    th = torch.full((H,), 3.0, device=DEV)
    th[0] = th[-1] = 2.0
    tw = torch.full((W,), 3.0, device=DEV)
    tw[0] = tw[-1] = 2.0
    expect = (C * th[:, None] * tw[None, :]).expand(N_FWD, COUT, H, W)
    assert expect[0, 0, 0, 0] == 4 * C and expect[0, 0, 1, 1] == 9 * C
    assert torch.equal(out.float(), expect)


# ---------------------------------------------------------------------------
# argument rejection: every call must raise before any launch. The device
# tensors that replace a right one are never smaller than it.
# ---------------------------------------------------------------------------

RJ = (11, 11, 32, 32, 3)


def _wrw_args(data):
    d = data[RJ]
    return dict(x=d["x"], g=d["g"],
                gw=torch.zeros(32, 288, dtype=torch.float32, device=DEV),
                gb=torch.zeros(32, dtype=torch.float32, device=DEV))


def _bad_dtype(a):
    a["g"] = a["g"].float().contiguous(memory_format=torch.channels_last)


def _bad_nchw_gout(a):
    a["g"] = a["g"].contiguous()
    assert not a["g"].is_contiguous(memory_format=torch.channels_last)


def _bad_batch(a):
    a["g"] = _cl(torch.zeros(4, 32, 11, 11, device=DEV))


def _bad_gw_numel(a):
    a["gw"] = torch.zeros(32, 288 + 32, dtype=a["gw"].dtype, device=DEV)


def _bad_cpu(a):
    a["g"] = a["g"].cpu()


SPOILERS = [_bad_dtype, _bad_nchw_gout, _bad_batch, _bad_gw_numel, _bad_cpu]


@pytest.mark.parametrize("spoil", SPOILERS, ids=lambda f: f.__name__[5:])
def test_wrw_rejects(ext, data, spoil):
    a = _wrw_args(data)
    ext.conv3x3p1_wrw(a["x"], a["g"], a["gw"], a["gb"], False)
    spoil(a)
    with pytest.raises(RuntimeError):
        ext.conv3x3p1_wrw(a["x"], a["g"], a["gw"], a["gb"], False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("spoil", SPOILERS, ids=lambda f: f.__name__[5:])
def test_dgrad_rejects(ext, data, spoil):
    d = data[RJ]
    # gw plays the flipped-weight workspace here
    a = dict(g=d["g"], gw=torch.zeros(32 * 288, dtype=BF16, device=DEV))
    gx = torch.zeros_like(d["x"])
    none = torch.empty(0, dtype=BF16, device=DEV)
    ext.conv3x3p1_dgrad(a["g"], d["w"], a["gw"], gx, none)
    spoil(a)
    a["gw"] = a["gw"].reshape(-1)
    with pytest.raises(RuntimeError):
        ext.conv3x3p1_dgrad(a["g"], d["w"], a["gw"], gx, none)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------


def _set_gates(monkeypatch, v):
    monkeypatch.setenv("DRL_OWN_RESCONV_WRW", v)
    monkeypatch.setenv("DRL_OWN_RESCONV_DGRAD", v)


def _compare(shape, names, mine, theirs):
    for m, t, name in zip(mine, theirs, names):
        m, t = m.float(), t.float()
        scale = t.abs().max().item() + 1e-6
        mae = (m - t).abs().mean().item()
        frac_big = ((m - t).abs() > 0.1 * scale).float().mean().item()
        print(f"{shape} {name}: mae/scale {mae / scale:.3g} "
              f"frac_big {frac_big:.3g}")
        assert mae / scale < 5e-3, f"{name}: mae {mae} scale {scale}"
        assert frac_big < 0.01, f"{name}: {frac_big:.3%} entries off"


@pytest.mark.parametrize("gates", ["1", "0"])
@pytest.mark.parametrize("shape", [(11, 11, 32, 4), (42, 42, 16, 3),
                                   (21, 21, 32, 3)])
def test_block_backward_matches_eager(ext, monkeypatch, shape, gates):
    """Residual block as two fused convs vs fp32 eager autograd, with the
    criteria of test_gpu_resconv.test_block_backward_matches_eager."""
    from distributed_rl_amd import ops

    _set_gates(monkeypatch, gates)
    H, W, C, n = shape
    torch.manual_seed(7)
    x = _cl(torch.randn(n, C, H, W, device=DEV))
    w1, w2 = (_cl(torch.randn(C, C, 3, 3, device=DEV) * 0.05)
              for _ in range(2))
    b1, b2 = ((torch.randn(C, device=DEV) * 0.1).to(BF16) for _ in range(2))
    g = _cl(torch.randn(n, C, H, W, device=DEV))

    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xl, w1l, b1l, w2l, b2l = leaves
    y = ops.fused_conv3x3(xl, w1l, b1l, relu_in=True, relu_out=True)
    out = ops.fused_conv3x3(y, w2l, b2l, residual=xl)
    mine = torch.autograd.grad(out, leaves, g)
    assert all(m.dtype == BF16 for m in mine)
    assert mine[1].is_contiguous(memory_format=torch.channels_last)

    fl = [t.float().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xf, w1f, b1f, w2f, b2f = fl
    yf = F.conv2d(F.relu(xf), w1f, b1f, padding=1)
    of = xf + F.conv2d(F.relu(yf), w2f, b2f, padding=1)
    theirs = torch.autograd.grad(of, fl, g.float())
    _compare(shape, ["gx", "gw1", "gb1", "gw2", "gb2"], mine, theirs)


@pytest.mark.parametrize("gates", ["1", "0"])
def test_entry_conv_backward_matches_eager(ext, monkeypatch, gates):
    """The lone 42x42 16->32 section-entry conv (no flags): its input
    gradient runs the 42x42 32->16 instantiation."""
    from distributed_rl_amd import ops

    _set_gates(monkeypatch, gates)
    torch.manual_seed(9)
    x = _cl(torch.randn(3, 16, 42, 42, device=DEV))
    w = _cl(torch.randn(32, 16, 3, 3, device=DEV) * 0.05)
    b = (torch.randn(32, device=DEV) * 0.1).to(BF16)
    g = _cl(torch.randn(3, 32, 42, 42, device=DEV))
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    mine = torch.autograd.grad(ops.fused_conv3x3(*leaves), leaves, g)
    fl = [t.float().requires_grad_(True) for t in (x, w, b)]
    theirs = torch.autograd.grad(F.conv2d(*fl, padding=1), fl, g.float())
    _compare("42x42x16->32", ["gx", "gw", "gb"], mine, theirs)


def _resnet_net():
    from distributed_rl_amd.config import load_config
    from distributed_rl_amd.models import BaseAgent

    torch.manual_seed(5)
    ref = BaseAgent(load_config("impala_resnet").model_info).to(DEV)
    return copy.deepcopy(ref).to(memory_format=torch.channels_last).to(BF16)


def _count_calls(monkeypatch, ext):
    counts = {"wrw": 0, "dgrad": 0}

    def wrap(name, key):
        real = getattr(ext, name)

        def counting(*a, **kw):
            counts[key] += 1
            return real(*a, **kw)

        monkeypatch.setattr(ext, name, counting)

    wrap("conv3x3p1_wrw", "wrw")
    wrap("conv3x3p1_dgrad", "dgrad")
    return counts


def test_model_backward_call_counts(ext, monkeypatch):
    """Gates on: the 14 padded convs of the torso take the own kernels, and
    the library's convolution_backward runs once, for the first conv (seen
    at the dispatcher: nn.Conv2d's backward never passes through Python)."""
    from torch.utils._python_dispatch import TorchDispatchMode

    monkeypatch.setenv("DRL_OWN_RESCONV", "1")
    _set_gates(monkeypatch, "1")
    net = _resnet_net()
    params = list(net.parameters())
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV))
    counts = _count_calls(monkeypatch, ext)
    lib = []

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.convolution_backward.default:
                lib.append(tuple(args[1].shape))
            return func(*args, **(kwargs or {}))

    with Count():
        grads = torch.autograd.grad(net([x])[0].float().square().sum(),
                                    params)
    assert counts == {"wrw": 14, "dgrad": 14}, counts
    assert lib == [(2, 4, 84, 84)], lib
    for g in grads:
        assert torch.isfinite(g.float()).all()

    # gates off: nothing of the backward reaches the own kernels
    _set_gates(monkeypatch, "0")
    torch.autograd.grad(net([x])[0].float().square().sum(), params)
    assert counts == {"wrw": 14, "dgrad": 14}, counts


def test_model_graph_capture(ext, monkeypatch):
    """One captured forward+backward of the model with both gates on replays
    to finite gradients (no bit-equality across replays: the max-pool
    backward upstream is library code)."""
    monkeypatch.setenv("DRL_OWN_RESCONV", "1")
    _set_gates(monkeypatch, "1")
    net = _resnet_net()
    counts = _count_calls(monkeypatch, ext)
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV))
    params = list(net.parameters())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(net([x])[0].float().square().sum(), params)
    torch.cuda.current_stream().wait_stream(side)
    assert counts == {"wrw": 28, "dgrad": 28}, counts

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = net([x])[0]
        grads = torch.autograd.grad(y.float().square().sum(), params)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(y.float()).all()
        for g in grads:
            assert torch.isfinite(g.float()).all()
        assert any(g.float().abs().max() > 0 for g in grads)
