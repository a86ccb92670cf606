"""The stem conv (C=4 -> 16) with run-time H and W (conv3x3c4_fwd_hw_kernel,
conv3x3c4_wrw_hw_kernel, the _hw bindings): exact-grid inputs against
float64 bit for bit at the edge shapes, the run-time kernel against the
table kernel at 84x84, halo, border count, rejections and the autograd op.

Cases and their bounds: tests/resconv_hw_cases.py."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resconv_hw_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
C, COUT = RC.STEM


def _cl(t):
    """bf16 channels_last on the device, INSIDE a larger allocation: guard
    images of NaN (at least 64 pixels) on both sides. A kernel that forms a
    wrong address (a mutated row decode or tap offset) then reads a wrong
    value or a NaN that the comparison sees, not memory outside the
    allocation."""
    t = t.to(device=DEV, dtype=BF16)
    g = 64 // max(1, t.shape[2] * t.shape[3]) + 1
    big = torch.full((t.shape[0] + 2 * g, *t.shape[1:]), float("nan"),
                     device=DEV, dtype=BF16).contiguous(
                         memory_format=torch.channels_last)
    big[g:-g] = t
    v = big[g:-g]
    assert v.is_contiguous(memory_format=torch.channels_last)
    return v


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _fwd(ext, x, w, b, hw=True):
    out = torch.full((x.shape[0], COUT, x.shape[2], x.shape[3]), float("nan"),
                     dtype=BF16, device=DEV).contiguous(
                         memory_format=torch.channels_last)
    (ext.conv3x3c4_fwd_hw if hw else ext.conv3x3c4_fwd)(
        x, w, b if b is not None else torch.empty(0, device=DEV, dtype=BF16),
        out)
    return out


def _wrw(ext, x, g, dtype=torch.float32, hw=True):
    gw = torch.full((COUT, 9 * C), float("nan"), dtype=dtype, device=DEV)
    gb = torch.full((COUT,), float("nan"), dtype=dtype, device=DEV)
    (ext.conv3x3c4_wrw_hw if hw else ext.conv3x3c4_wrw)(x, g, gw, gb)
    return gw, gb


def _between_nans(t):
    big = torch.full((t.shape[0] + 2, *t.shape[1:]), float("nan"), device=DEV,
                     dtype=BF16).contiguous(memory_format=torch.channels_last)
    big[1:-1] = t
    return big[1:-1]


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(
        a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32),
        b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_fwd_exact(ext, shape):
    from distributed_rl_amd import ops
    from distributed_rl_amd.ops import torch_ref

    H, W, N = shape
    d = RC.make_case(H, W, N, C, COUT)
    ref = torch_ref.conv3x3_res(d["x"], d["w"], d["b"])
    x, w = _cl(d["x"]), _cl(d["w"])
    b = d["b"].to(device=DEV, dtype=BF16)
    assert _same_bits(_fwd(ext, x, w, b).cpu(), ref.to(BF16))
    # the public op picks the run-time kernel away from 84x84
    assert not ext.conv3x3c4_supported(H, W, C, COUT)
    out = ops.fused_stem_conv3x3(x, w, b)
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert _same_bits(out.cpu(), ref.to(BF16))


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_wrw_exact(ext, shape):
    H, W, _ = shape
    N = RC.wrw_batch(H, W, RC.STEM_WRW_ROWS)
    d = RC.make_case(H, W, N, C, COUT)
    x, g = _cl(d["x"]), _cl(d["g"])
    gw, gb = _wrw(ext, x, g)
    assert torch.equal(gw.double().cpu(), d["gw"]), (shape, N)
    assert torch.equal(gb.double().cpu(), d["gb"]), (shape, N)
    gw16, gb16 = _wrw(ext, x, g, dtype=BF16)
    assert _same_bits(gw16, gw.to(BF16)) and _same_bits(gb16, gb.to(BF16))
    again = _wrw(ext, x, g)
    assert _same_bits(again[0], gw) and _same_bits(again[1], gb)


def test_wrw_capped_m_grid_and_plan(ext):
    """64x64 at a batch where the residency or the 16 MiB plane budget sets
    the stem's m-grid (wanted blocks, from the rules, exceed the cap; the
    launch's plan is the cap and takes the run-time entry's rows per
    pass). Exact-grid inputs, exact by their own sums although M > 2^17."""
    import torch.nn.functional as F

    H = W = 64
    rows = RC.STEM_WRW_ROWS
    n_elem = COUT * 9 * C
    pad = ext.wrw_plane_pad()
    resident = ext.conv3x3c4_wrw_plan(1, H, W, True)[2]
    cap = (16 << 20) // ((n_elem + pad) * 4)
    limit = min(cap, resident)
    N = (8 * rows * (limit + 1) + H * W - 1) // (H * W)
    mb, want, _ = RC.m_grid(N * H * W, rows, n_elem, pad, resident)
    print(f"stem: N={N} wanted {want} blocks, plane cap {cap}, "
          f"resident {resident}")
    assert want > limit and mb == limit
    assert tuple(ext.conv3x3c4_wrw_plan(N, H, W, True)) == \
        (limit, rows, resident)
    # small batches: the 8-passes rule, for the table kernel too
    assert tuple(ext.conv3x3c4_wrw_plan(3, 84, 84, True))[:2] == \
        (RC.m_grid(3 * 84 * 84, rows, n_elem, pad, resident)[0], rows)
    assert tuple(ext.conv3x3c4_wrw_plan(3, 84, 84, False))[:2] == \
        tuple(ext.conv3x3c4_wrw_plan(3, 84, 84, True))[:2]
    with pytest.raises(RuntimeError, match="no stem conv kernel"):
        ext.conv3x3c4_wrw_plan(3, 64, 64, False)
    gen = torch.Generator().manual_seed(37)
    x = _cl(RC.grid((N, C, H, W), 0.25, 2.0, gen))
    g = _cl(RC.grid((N, COUT, H, W), 0.25, 2.0, gen))

    def ref64(xx, gg):
        cols = F.unfold(xx.double(), 3, padding=1)        # (N, C*9, HW)
        gm = gg.double().reshape(N, COUT, H * W)
        gw = torch.einsum("nol,nkl->ok", gm, cols)
        return (gw.view(COUT, C, 9).permute(0, 2, 1).reshape(COUT, 9 * C),
                gm.sum((0, 2)))

    bound_gw, bound_gb = ref64(x.abs(), g.abs())
    assert bound_gw.max().item() * 16 < 2 ** 24
    assert bound_gb.max().item() * 4 < 2 ** 24
    ref_gw, ref_gb = ref64(x, g)
    gw, gb = _wrw(ext, x, g)
    assert torch.equal(gw.double(), ref_gw)
    assert torch.equal(gb.double(), ref_gb)
    again = _wrw(ext, x, g)
    assert _same_bits(again[0], gw) and _same_bits(again[1], gb)


def test_runtime_kernel_gives_the_table_kernels_bits(ext):
    """84x84, N = 3, random-valued inputs: conv3x3c4_fwd_hw against
    conv3x3c4_fwd, and the weight gradients (same rows per pass, m-grid
    from the 8-passes rule in both)."""
    gen = torch.Generator().manual_seed(17)
    x = _cl(torch.randn(3, C, 84, 84, generator=gen))
    w = _cl(torch.randn(COUT, C, 3, 3, generator=gen) * 0.1)
    b = (torch.randn(COUT, generator=gen) * 0.1).to(device=DEV, dtype=BF16)
    g = _cl(torch.randn(3, COUT, 84, 84, generator=gen))
    a = _fwd(ext, x, w, b, hw=False)
    h = _fwd(ext, x, w, b, hw=True)
    assert torch.isfinite(a.float()).all() and _same_bits(a, h)
    ta = _wrw(ext, x, g, hw=False)
    th = _wrw(ext, x, g, hw=True)
    assert _same_bits(ta[0], th[0]) and _same_bits(ta[1], th[1])
    again = _wrw(ext, x, g, hw=True)
    assert _same_bits(again[0], th[0]) and _same_bits(again[1], th[1])


@pytest.mark.parametrize("hw", [(2, 2, 70), (5, 7, 9), (1, 9, 3)],
                         ids=["2x2", "5x7", "1x9"])
def test_no_halo_reads(ext, hw):
    H, W, N = hw
    gen = torch.Generator().manual_seed(19)
    x = _cl(torch.randn(N, C, H, W, generator=gen))
    w = _cl(torch.randn(COUT, C, 3, 3, generator=gen) * 0.1)
    g = _cl(torch.randn(N, COUT, H, W, generator=gen))
    out = _fwd(ext, _between_nans(x), w, None)
    plain = _fwd(ext, _cl(x), w, None)
    assert torch.isfinite(out.float()).all() and _same_bits(out, plain)
    gw, gb = _wrw(ext, _between_nans(x), _between_nans(g))
    pw, pb = _wrw(ext, _cl(x), _cl(g))
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    assert _same_bits(gw, pw) and _same_bits(gb, pb)


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_exact_border_count(ext, shape):
    H, W, N = shape

    def taps(n):
        t = torch.full((n,), 3.0)
        t[0] -= 1
        t[-1] -= 1
        return t

    out = _fwd(ext, _cl(torch.ones(N, C, H, W)),
               _cl(torch.ones(COUT, C, 3, 3)), None)
    expect = (C * taps(H)[:, None] * taps(W)[None, :]).expand(N, COUT, H, W)
    assert torch.equal(out.float().cpu(), expect)


def _args(H=5, W=7):
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    clz = lambda *s: z(*s).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    return dict(x=clz(2, C, H, W), w=clz(COUT, C, 3, 3), b=z(COUT),
                out=clz(2, COUT, H, W), g=clz(2, COUT, H, W),
                gw=z(COUT, 9 * C, dt=torch.float32),
                gb=z(COUT, dt=torch.float32))


def _misaligned_weight():
    flat = torch.zeros(COUT * 9 * C + 4, dtype=BF16, device=DEV)
    w = flat[1:1 + COUT * 9 * C].view(COUT, 3, 3, C).permute(0, 3, 1, 2)
    assert w.is_contiguous(memory_format=torch.channels_last)
    assert w.data_ptr() % 8 == 2
    return w


def _aliased():
    """x (2, 4, 5, 7) and out (2, 16, 5, 7), both dense channels_last, that
    start at the same address."""
    buf = torch.zeros(2 * COUT * 35, dtype=BF16, device=DEV)
    out = buf.view(2, 5, 7, COUT).permute(0, 3, 1, 2)
    x = buf[:2 * C * 35].view(2, 5, 7, C).permute(0, 3, 1, 2)
    assert x.data_ptr() == out.data_ptr()
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert out.is_contiguous(memory_format=torch.channels_last)
    return dict(x=x, out=out)


def test_rejections(ext):
    """Each raises before any launch, names the argument and says _hw."""
    def fwd(a):
        ext.conv3x3c4_fwd_hw(a["x"], a["w"], a["b"], a["out"])

    def wrw(a):
        ext.conv3x3c4_wrw_hw(a["x"], a["g"], a["gw"], a["gb"])

    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    clz = lambda *s: z(*s).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    spoil = [
        ("C = 8", fwd, "conv3x3c4_fwd_hw x: no stem conv kernel for this "
         "geometry",
         lambda a: a.update(x=clz(2, 8, 5, 7), w=clz(COUT, 8, 3, 3))),
        ("COUT = 32", fwd, "conv3x3c4_fwd_hw weight: no stem conv kernel for "
         "this geometry",
         lambda a: a.update(w=clz(32, C, 3, 3), b=z(32),
                            out=clz(2, 32, 5, 7))),
        ("COUT = 32 wrw", wrw, "conv3x3c4_wrw_hw gout: no stem conv kernel "
         "for this geometry",
         lambda a: a.update(g=clz(2, 32, 5, 7),
                            gw=z(32, 9 * C, dt=torch.float32),
                            gb=z(32, dt=torch.float32))),
        ("out of another H", fwd, "conv3x3c4_fwd_hw out",
         lambda a: a.update(out=clz(2, COUT, 6, 7))),
        ("gout of another H", wrw, "conv3x3c4_wrw_hw gout",
         lambda a: a.update(g=clz(2, COUT, 6, 7))),
        ("nchw x", fwd, "conv3x3c4_fwd_hw x",
         lambda a: a.update(x=z(2, C, 5, 7))),
        ("nchw gout", wrw, "conv3x3c4_wrw_hw gout",
         lambda a: a.update(g=z(2, COUT, 5, 7))),
        ("fp32 x", fwd, "conv3x3c4_fwd_hw x",
         lambda a: a.update(x=a["x"].float())),
        ("fp32 x wrw", wrw, "conv3x3c4_wrw_hw x",
         lambda a: a.update(x=a["x"].float())),
        ("cpu x", fwd, "conv3x3c4_fwd_hw x",
         lambda a: a.update(x=a["x"].cpu())),
        ("cpu gout", wrw, "conv3x3c4_wrw_hw gout",
         lambda a: a.update(g=a["g"].cpu())),
        ("misaligned weight view", fwd, "conv3x3c4_fwd_hw weight is "
         "misaligned", lambda a: a.update(w=_misaligned_weight())),
        ("out aliasing x", fwd, "conv3x3c4_fwd_hw out must not alias x",
         lambda a: a.update(**_aliased())),
        ("gw of the wrong element count", wrw, "conv3x3c4_wrw_hw gw",
         lambda a: a.update(gw=z(COUT, 9 * C + 1, dt=torch.float32))),
    ]
    fwd(_args())
    wrw(_args())
    fwd(_args(84, 84))  # the _hw bindings take the table geometry too
    for name, call, names_arg, change in spoil:
        a = _args()
        change(a)
        with pytest.raises(RuntimeError, match=names_arg):
            call(a)
            pytest.fail(f"{name} was accepted")
    # the table bindings still reject every size but 84x84
    a = _args()
    with pytest.raises(RuntimeError, match="conv3x3c4_fwd x"):
        ext.conv3x3c4_fwd(a["x"], a["w"], a["b"], a["out"])
    with pytest.raises(RuntimeError, match="conv3x3c4_wrw x"):
        ext.conv3x3c4_wrw(a["x"], a["g"], a["gw"], a["gb"])
    # a valid call afterwards still works
    a = _args()
    a["x"].fill_(1.0)
    a["w"].fill_(1.0)
    a["g"].fill_(1.0)
    fwd(a)
    wrw(a)
    torch.cuda.synchronize()
    assert a["out"][0, 0, 1, 1] == 9 * C and a["out"][0, 0, 0, 0] == 4 * C
    assert a["gw"][0, 4 * C] == 2 * 5 * 7


def test_autograd_op_off_the_table(ext, monkeypatch):
    """fused_stem_conv3x3 at 32x24: own forward and own ordered weight
    gradient (no library backward when x needs no gradient), exact on the
    grid inputs."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from distributed_rl_amd import ops

    monkeypatch.delenv("DRL_OWN_STEM_WRW", raising=False)
    d = RC.make_case(32, 24, 2, C, COUT)
    x = _cl(d["x"])
    w = _cl(d["w"]).requires_grad_(True)
    b = d["b"].to(device=DEV, dtype=BF16).requires_grad_(True)
    lib = []

    class _Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.convolution_backward.default:
                lib.append(1)
            return func(*args, **(kwargs or {}))

    with _Spy():
        out = ops.fused_stem_conv3x3(x, w, b)
        gw, gb = torch.autograd.grad(out, [w, b], _cl(d["g"]))
    assert not lib
    assert _same_bits(gw.permute(0, 2, 3, 1).reshape(COUT, 9 * C).cpu(),
                      d["gw"].to(BF16))
    assert _same_bits(gb.cpu(), d["gb"].to(BF16))
