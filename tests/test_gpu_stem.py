"""Hand-written stem conv of the IMPALA-ResNet torso (conv3x3c4_fwd_kernel /
conv3x3c4_wrw_kernel: 3x3 stride-1 pad-1, 84x84, C=4 -> 16): forward and
weight gradient against CPU references, exact integer cases, border counts,
no halo reads, determinism, argument checks, the autograd op, the model gate
and graph capture.

N = 3 makes M = 21168 rows: a multiple of neither 256 nor 128, so every
kernel runs several blocks and a ragged tail. References are computed once on
the CPU (fp64) and never written."""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
H = W = 84
C, COUT = 4, 16
N = 3


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _wrw_ref(x, g):
    """fp64 CPU (gw as (16, 36) in the kernel's (kh, kw, c) order, gb)."""
    _, gw, gb = torch.ops.aten.convolution_backward(
        g.double(), x.double(), torch.zeros(COUT, C, 3, 3, dtype=torch.double),
        [COUT], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True])
    return gw.permute(0, 2, 3, 1).reshape(COUT, 9 * C), gb


@pytest.fixture(scope="module")
def data(ext):
    """bf16-rounded random operands and integer operands (exact in bf16) on
    the CPU, their fp64 references, and device copies."""
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(N, C, H, W, generator=gen).to(BF16)
    w = (torch.randn(COUT, C, 3, 3, generator=gen) * 0.05).to(BF16)
    b = (torch.randn(COUT, generator=gen) * 0.1).to(BF16)
    g = torch.randn(N, COUT, H, W, generator=gen).to(BF16)
    xi = torch.randint(-8, 9, (N, C, H, W), generator=gen).to(BF16)
    wi = torch.randint(-4, 5, (COUT, C, 3, 3), generator=gen).to(BF16)
    bi = torch.randint(-16, 17, (COUT,), generator=gen).to(BF16)
    gi = torch.randint(-4, 5, (N, COUT, H, W), generator=gen).to(BF16)
    gw, gb = _wrw_ref(x, g)
    gwi, gbi = _wrw_ref(xi, gi)
    d = dict(x=x, w=w, b=b, g=g, xi=xi, wi=wi, bi=bi, gi=gi, gw=gw, gb=gb,
             gwi=gwi, gbi=gbi,
             out_i=F.conv2d(xi.double(), wi.double(), bi.double(), padding=1))
    for k in ("x", "w", "g", "xi", "wi", "gi"):
        d[k + "d"] = _cl(d[k].to(DEV))
    d["bd"], d["bid"] = b.to(DEV), bi.to(DEV)
    return d


def _fwd(ext, x, w, b=None):
    out = _cl(torch.full((x.shape[0], COUT, H, W), float("nan"), dtype=BF16,
                         device=DEV))
    ext.conv3x3c4_fwd(x, w, b if b is not None
                      else torch.empty(0, dtype=BF16, device=DEV), out)
    return out


def _wrw(ext, x, g, dtype=torch.float32, bias=True):
    gw = torch.full((COUT, 9 * C), float("nan"), dtype=dtype, device=DEV)
    gb = (torch.full((COUT,), float("nan"), dtype=dtype, device=DEV) if bias
          else torch.empty(0, device=DEV))
    ext.conv3x3c4_wrw(x, g, gw, gb)
    return gw, gb


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
# forward
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_fwd_vs_fp32(ext, data, bias):
    """Against fp32 of the bf16-rounded operands, the criterion of
    test_gpu_resconv.test_fwd_vs_fp32."""
    from distributed_rl_amd import ops

    b = data["bd"] if bias else None
    out = ops.fused_stem_conv3x3(data["xd"], data["wd"], b)
    ref = F.conv2d(data["x"].float(), data["w"].float(),
                   data["b"].float() if bias else None, padding=1)
    assert out.shape == ref.shape and out.dtype == BF16
    assert out.is_contiguous(memory_format=torch.channels_last)
    err = (out.float().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"stem fwd bias={bias}: max err {err:.4g} / max ref {scale:.4g} "
          f"= {err / scale:.3g}")
    assert err / scale < 2e-2
    # the binding writes the same bytes
    assert torch.equal(_fwd(ext, data["xd"], data["wd"], b), out)


def test_fwd_exact_integers(ext, data):
    """x in [-8, 8], w in [-4, 4], b in [-16, 16]: every partial sum is an
    integer of magnitude <= 36*32 + 16 = 1168 < 2^24, so any fp32 summation
    order is exact; the reference is fp64 on the CPU, rounded once."""
    out = _fwd(ext, data["xid"], data["wid"], data["bid"])
    ref = data["out_i"]
    assert ref.abs().max() <= 1168
    want = _cl(ref.float().to(BF16))
    assert torch.equal(out.cpu(), want)


def test_fwd_exact_border_count(ext):
    """All-ones x and w: out = 4 x (in-bounds taps), exactly."""
    x = _cl(torch.ones(N, C, H, W, dtype=BF16, device=DEV))
    w = _cl(torch.ones(COUT, C, 3, 3, dtype=BF16, device=DEV))
    out = _fwd(ext, x, w)
    th = torch.full((H,), 3.0, device=DEV)
    th[0] = th[-1] = 2.0
    tw = torch.full((W,), 3.0, device=DEV)
    tw[0] = tw[-1] = 2.0
    expect = (C * th[:, None] * tw[None, :]).expand(N, COUT, H, W)
    assert expect[0, 0, 0, 0] == 16 and expect[0, 0, 0, 1] == 24 \
        and expect[0, 0, 1, 1] == 36
    assert torch.equal(out.float(), expect)


def test_fwd_no_halo_reads(ext, data):
    """x sits between two NaN images of one allocation: a tap read across an
    image border would pull a NaN into the output."""
    out = _fwd(ext, _between_nans(data["xd"]), data["wd"], data["bd"])
    plain = _fwd(ext, data["xd"].clone(memory_format=torch.channels_last),
                 data["wd"], data["bd"])
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, plain)


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------


def _check_wrw_bound(tag, got, ref):
    err = (got.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{tag}: max err {err:.4g} / max ref {scale:.4g} = {err / scale:.3g}")
    assert err <= 1e-5 * scale, f"{tag}: {err} vs {scale}"


@pytest.mark.parametrize("bias", [True, False], ids=["gb", "nogb"])
def test_wrw_fp32_vs_fp64(ext, data, bias):
    """The bound of test_gpu_resconv_bwd.test_wrw_fp32_vs_fp64: 1e-5 of
    max|ref|."""
    gw, gb = _wrw(ext, data["xd"], data["gd"], bias=bias)
    _check_wrw_bound("stem gw", gw, data["gw"])
    if bias:
        _check_wrw_bound("stem gb", gb, data["gb"])
    else:
        assert gb.numel() == 0


def test_wrw_exact_integers(ext, data):
    """x in [-8, 8], gout in [-4, 4]: |gw| <= 21168*32 = 677376 and
    |gb| <= 84672, both below 2^24, so the fp32 workspace equals the fp64
    reference exactly and the bf16 output is that rounded once."""
    assert data["gwi"].abs().max() <= 677376
    assert data["gbi"].abs().max() <= 84672
    gw, gb = _wrw(ext, data["xid"], data["gid"])
    assert torch.equal(gw.double().cpu(), data["gwi"])
    assert torch.equal(gb.double().cpu(), data["gbi"])
    gw16, gb16 = _wrw(ext, data["xid"], data["gid"], dtype=BF16)
    assert torch.equal(gw16.cpu(), data["gwi"].float().to(BF16))
    assert torch.equal(gb16.cpu(), data["gbi"].float().to(BF16))


def test_wrw_bf16_output(ext, data):
    """Same partials, order and rounding as the fp32 workspace path."""
    gw32, gb32 = _wrw(ext, data["xd"], data["gd"])
    gw16, gb16 = _wrw(ext, data["xd"], data["gd"], dtype=BF16)
    assert torch.equal(gw16, gw32.to(BF16))
    assert torch.equal(gb16, gb32.to(BF16))
    # a channels_last weight-shaped gradient tensor takes the same bytes
    gw4 = torch.empty(COUT, 3, 3, C, dtype=BF16, device=DEV).permute(0, 3, 1, 2)
    ext.conv3x3c4_wrw(data["xd"], data["gd"], gw4, torch.empty(0, device=DEV))
    assert torch.equal(gw4.permute(0, 2, 3, 1).reshape(COUT, 9 * C), gw16)


def test_wrw_exact_borders(ext):
    """All-ones x and gout: gw[co][kh][kw][c] = N x (pixels whose tap is in
    bounds)."""
    x = _cl(torch.ones(N, C, H, W, dtype=BF16, device=DEV))
    g = _cl(torch.ones(N, COUT, H, W, dtype=BF16, device=DEV))
    gw, gb = _wrw(ext, x, g)
    k = torch.arange(3, device=DEV)
    cnt = N * (H - (k - 1).abs())[:, None] * (W - (k - 1).abs())[None, :]
    expect = cnt.float()[None, :, :, None].expand(COUT, 3, 3, C)
    assert expect[0, 0, 2, 0] == N * 83 * 83
    assert expect[0, 0, 1, 0] == N * 83 * 84
    assert expect[0, 1, 1, 0] == N * 84 * 84
    assert torch.equal(gw.view(COUT, 3, 3, C), expect)
    assert torch.equal(gb, torch.full_like(gb, N * H * W))


def test_wrw_no_halo_reads(ext, data):
    gw, gb = _wrw(ext, _between_nans(data["xd"]), _between_nans(data["gd"]))
    plain = _wrw(ext, data["xd"].clone(memory_format=torch.channels_last),
                 data["gd"].clone(memory_format=torch.channels_last))
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    assert torch.equal(gw, plain[0]) and torch.equal(gb, plain[1])


def test_wrw_deterministic(ext, data):
    a = _wrw(ext, data["xd"], data["gd"])
    b = _wrw(ext, data["xd"], data["gd"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_wrw_capped_m_grid(ext):
    """N = 192: 42336 passes want 5292 blocks, more than are resident on
    the device, so the residency cap sets the m-grid. Same bounds as
    test_wrw_fp32_vs_fp64, and deterministic."""
    n = 192
    gen = torch.Generator().manual_seed(37)
    x = torch.randn(n, C, H, W, generator=gen).to(BF16)
    g = torch.randn(n, COUT, H, W, generator=gen).to(BF16)
    ref_gw, ref_gb = _wrw_ref(x, g)
    xd, gd = _cl(x.to(DEV)), _cl(g.to(DEV))
    gw, gb = _wrw(ext, xd, gd)
    _check_wrw_bound("stem N=192 gw", gw, ref_gw)
    _check_wrw_bound("stem N=192 gb", gb, ref_gb)
    again = _wrw(ext, xd, gd)
    assert torch.equal(gw, again[0]) and torch.equal(gb, again[1])


# ---------------------------------------------------------------------------
# argument checks: each raises before any launch and names the argument
# ---------------------------------------------------------------------------


def _args():
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    return dict(x=_cl(z(2, C, H, W)), w=_cl(z(COUT, C, 3, 3)), b=z(COUT),
                out=_cl(z(2, COUT, H, W)), g=_cl(z(2, COUT, H, W)),
                gw=z(COUT, 9 * C, dt=torch.float32),
                gb=z(COUT, dt=torch.float32))


def _misaligned_weight():
    """A dense channels_last (16, 4, 3, 3) view 2 bytes into its buffer."""
    flat = torch.zeros(COUT * 9 * C + 4, dtype=BF16, device=DEV)
    w = flat[1:1 + COUT * 9 * C].view(COUT, 3, 3, C).permute(0, 3, 1, 2)
    assert w.is_contiguous(memory_format=torch.channels_last)
    assert w.data_ptr() % 8 == 2
    return w


def test_rejections(ext):
    def fwd(a):
        ext.conv3x3c4_fwd(a["x"], a["w"], a["b"], a["out"])

    def wrw(a):
        ext.conv3x3c4_wrw(a["x"], a["g"], a["gw"], a["gb"])

    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    spoil = [
        ("cpu x", fwd, "conv3x3c4_fwd x", lambda a: a.update(x=a["x"].cpu())),
        ("cpu gout", wrw, "conv3x3c4_wrw gout",
         lambda a: a.update(g=a["g"].cpu())),
        ("fp32 x", fwd, "conv3x3c4_fwd x", lambda a: a.update(x=a["x"].float())),
        ("fp32 x wrw", wrw, "conv3x3c4_wrw x",
         lambda a: a.update(x=a["x"].float())),
        ("nchw x", fwd, "conv3x3c4_fwd x",
         lambda a: a.update(x=a["x"].contiguous())),
        ("nchw gout", wrw, "conv3x3c4_wrw gout",
         lambda a: a.update(g=a["g"].contiguous())),
        ("wrong H", fwd, "conv3x3c4_fwd x",
         lambda a: a.update(x=_cl(z(2, C, 42, W)), out=_cl(z(2, COUT, 42, W)))),
        ("wrong H wrw", wrw, "conv3x3c4_wrw x",
         lambda a: a.update(x=_cl(z(2, C, 42, W)), g=_cl(z(2, COUT, 42, W)))),
        ("wrong COUT", fwd, "conv3x3c4_fwd weight",
         lambda a: a.update(w=_cl(z(32, C, 3, 3)), b=z(32),
                            out=_cl(z(2, 32, H, W)))),
        ("wrong COUT wrw", wrw, "conv3x3c4_wrw gout",
         lambda a: a.update(g=_cl(z(2, 32, H, W)),
                            gw=z(32, 9 * C, dt=torch.float32),
                            gb=z(32, dt=torch.float32))),
        ("out of the wrong size", fwd, "conv3x3c4_fwd out",
         lambda a: a.update(out=_cl(z(3, COUT, H, W)))),
        ("gout of another batch", wrw, "conv3x3c4_wrw gout",
         lambda a: a.update(g=_cl(z(3, COUT, H, W)))),
        ("gw of the wrong element count", wrw, "conv3x3c4_wrw gw",
         lambda a: a.update(gw=z(COUT, 9 * C + 1, dt=torch.float32))),
        ("gb of the wrong dtype", wrw, "conv3x3c4_wrw gb",
         lambda a: a.update(gb=z(COUT))),
        ("bias of the wrong size", fwd, "conv3x3c4_fwd bias",
         lambda a: a.update(b=z(COUT + 1))),
        ("misaligned weight view", fwd, "conv3x3c4_fwd weight",
         lambda a: a.update(w=_misaligned_weight())),
    ]
    fwd(_args())
    wrw(_args())  # the unspoiled calls pass
    for name, call, names_arg, change in spoil:
        a = _args()
        change(a)
        with pytest.raises(RuntimeError, match=names_arg):
            call(a)
            pytest.fail(f"{name} was accepted")
    # a valid call afterwards still works
    a = _args()
    a["x"].fill_(1.0)
    a["w"].fill_(1.0)
    fwd(a)
    wrw(a)
    torch.cuda.synchronize()
    assert a["out"][0, 0, 1, 1] == 36


# ---------------------------------------------------------------------------
# autograd op
# ---------------------------------------------------------------------------


def _compare(names, mine, theirs):
    """The criteria of test_gpu_resconv_bwd.test_block_backward_matches_eager."""
    for m, t, name in zip(mine, theirs, names):
        m, t = m.float(), t.float()
        scale = t.abs().max().item() + 1e-6
        mae = (m - t).abs().mean().item()
        frac_big = ((m - t).abs() > 0.1 * scale).float().mean().item()
        print(f"stem {name}: mae/scale {mae / scale:.3g} "
              f"frac_big {frac_big:.3g}")
        assert mae / scale < 5e-3, f"{name}: mae {mae} scale {scale}"
        assert frac_big < 0.01, f"{name}: {frac_big:.3%} entries off"


def _lib_backward_masks():
    """A dispatch mode that records the output mask of every library
    convolution_backward."""
    from torch.utils._python_dispatch import TorchDispatchMode

    seen = []

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.convolution_backward.default:
                seen.append((tuple(args[1].shape), list(args[-1])))
            return func(*args, **(kwargs or {}))

    return Count(), seen


@pytest.mark.parametrize("mode", ["frames", "x_grad", "wrw_off"])
def test_op_backward_matches_eager(ext, data, monkeypatch, mode):
    """frames: x is data, nothing reaches the library. x_grad: the library
    supplies gx only. wrw_off (DRL_OWN_STEM_WRW=0): it supplies gw and gb."""
    from distributed_rl_amd import ops

    if mode == "wrw_off":
        monkeypatch.setenv("DRL_OWN_STEM_WRW", "0")
    else:
        monkeypatch.delenv("DRL_OWN_STEM_WRW", raising=False)
    x = data["xd"].clone(memory_format=torch.channels_last)
    w = data["wd"].clone(memory_format=torch.channels_last).requires_grad_(True)
    b = data["bd"].clone().requires_grad_(True)
    leaves, names = [w, b], ["gw", "gb"]
    if mode == "x_grad":
        x.requires_grad_(True)
        leaves, names = [x, w, b], ["gx", "gw", "gb"]
    count, seen = _lib_backward_masks()
    with count:
        mine = torch.autograd.grad(ops.fused_stem_conv3x3(x, w, b), leaves,
                                   data["gd"].contiguous())  # NCHW gout is fine
    want_lib = {"frames": [], "x_grad": [[True, False, False]],
                "wrw_off": [[False, True, True]]}[mode]
    assert [m for _, m in seen] == want_lib, seen
    assert all(m.dtype == BF16 for m in mine)
    assert mine[-2].is_contiguous(memory_format=torch.channels_last)

    fl = [t.detach().float().requires_grad_(True) for t in (x, w, b)]
    theirs = torch.autograd.grad(F.conv2d(*fl, padding=1), fl,
                                 data["gd"].float())
    _compare(names, mine, theirs[-len(names):])


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------


def _resnet_agent():
    from distributed_rl_amd.config import load_config
    from distributed_rl_amd.models import BaseAgent

    torch.manual_seed(5)
    ref = BaseAgent(load_config("impala_resnet").model_info).to(DEV)
    net = copy.deepcopy(ref).to(memory_format=torch.channels_last).to(BF16)
    return ref, net


def _count_ops(monkeypatch):
    from distributed_rl_amd import ops

    counts = {"stem": 0, "conv3": 0}

    def wrap(name, key):
        real = getattr(ops, name)

        def counting(*a, **kw):
            counts[key] += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, counting)

    wrap("fused_stem_conv3x3", "stem")
    wrap("fused_conv3x3", "conv3")
    return counts


def test_model_stem_path(ext, monkeypatch):
    """All conv gates on: 1 + 14 convs on own kernels, no library
    convolution_backward at all, and the output as close to the fp32 model as
    the library bf16 path is (the rule of test_model_fused_path). Gate unset
    or 0: the stem op is not called and the library backward runs once, on
    the frames."""
    ref, net = _resnet_agent()
    params = list(net.parameters())
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV).to(BF16))
    counts = _count_ops(monkeypatch)
    monkeypatch.setenv("DRL_OWN_RESCONV", "1")
    monkeypatch.setenv("DRL_OWN_RESCONV_WRW", "1")
    monkeypatch.setenv("DRL_OWN_RESCONV_DGRAD", "1")
    monkeypatch.setenv("DRL_OWN_STEM_WRW", "1")

    monkeypatch.setenv("DRL_OWN_STEM", "1")
    count, seen = _lib_backward_masks()
    y_own = net([x])[0]
    assert counts == {"stem": 1, "conv3": 14}, counts
    with count:
        grads = torch.autograd.grad(y_own.float().square().sum(), params)
    assert seen == [], seen
    for g in grads:
        assert torch.isfinite(g.float()).all()
    assert any(g.float().abs().max() > 0 for g in grads)

    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("DRL_OWN_STEM")
        else:
            monkeypatch.setenv("DRL_OWN_STEM", setting)
        counts.update(stem=0, conv3=0)
        count, seen = _lib_backward_masks()
        y_off = net([x])[0]
        assert counts == {"stem": 0, "conv3": 14}, (setting, counts)
        with count:
            torch.autograd.grad(y_off.float().square().sum(), params)
        assert [s for s, _ in seen] == [(2, 4, 84, 84)], (setting, seen)

    with torch.no_grad():
        y_ref = ref([x.float()])[0]
        monkeypatch.setenv("DRL_OWN_RESCONV", "0")
        y_lib = net([x])[0]
    err_own = (y_own.float() - y_ref).abs().max().item()
    err_lib = (y_lib.float() - y_ref).abs().max().item()
    print(f"model: stem+resconv err {err_own:.4g}, library bf16 err "
          f"{err_lib:.4g}")
    assert err_own <= 2 * err_lib


def test_model_graph_capture(ext, monkeypatch):
    """One captured forward+backward of the bare torso with the stem, conv
    and pool gates on: two replays give bit-equal output and bit-equal
    gradients for EVERY parameter, body.0.weight included."""
    from distributed_rl_amd.models.base_agent import ImpalaResNet

    for name in ("DRL_OWN_STEM", "DRL_OWN_STEM_WRW", "DRL_OWN_RESCONV",
                 "DRL_OWN_RESCONV_WRW", "DRL_OWN_RESCONV_DGRAD",
                 "DRL_OWN_POOL"):
        monkeypatch.setenv(name, "1")
    torch.manual_seed(5)
    net = ImpalaResNet({"iSize": 4, "channels": [16, 32, 32], "nBlocks": 2})
    net = net.to(DEV).to(memory_format=torch.channels_last).to(BF16)
    counts = _count_ops(monkeypatch)
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV).to(BF16))
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())
    assert "body.0.weight" in names

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(net(x).float().square().sum(), params)
    torch.cuda.current_stream().wait_stream(side)
    assert counts == {"stem": 2, "conv3": 28}, counts

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = net(x)
        grads = torch.autograd.grad(y.float().square().sum(), params)
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append([y.clone()] + [g.clone() for g in grads])
    assert torch.isfinite(seen[0][0].float()).all()
    assert seen[0][0].abs().max() > 0
    assert torch.equal(seen[0][0], seen[1][0])
    differ = [n for n, a, b in zip(names, seen[0][1:], seen[1][1:])
              if not torch.equal(a, b)]
    print("gradients that differ between replays:", differ)
    for n, a in zip(names, seen[0][1:]):
        assert torch.isfinite(a.float()).all(), n
        assert a.float().abs().max() > 0, n
    assert differ == []
