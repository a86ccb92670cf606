"""The 3x3 pad-1 conv kernels with run-time H and W (conv3x3p1_fwd_hw_kernel,
conv3x3p1_wrw_hw_kernel): exact-grid inputs against float64 bit for bit at
the shapes where the row decode, the bounds tests and the tap offset can go
wrong; the run-time kernel against the table kernel; halo, border count,
flags, rejections; and the torso at 32x24 end to end.

Cases and their bounds: tests/resconv_hw_cases.py (checked on the CPU by
test_resconv_hw_ref.py)."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resconv_hw_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16


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


def _empty():
    return torch.empty(0, device=DEV, dtype=BF16)


def _fwd(ext, x, w, b=None, r=None, relu_in=False, relu_out=False,
         any_hw=False):
    out = torch.empty(x.shape[0], w.shape[0], x.shape[2], x.shape[3],
                      dtype=BF16, device=DEV,
                      memory_format=torch.channels_last)
    ext.conv3x3p1_fwd(x, w, b if b is not None else _empty(),
                      r if r is not None else _empty(), out, relu_in,
                      relu_out, any_hw=any_hw)
    return out


def _wrw(ext, x, g, relu_in=False, dtype=torch.float32, any_hw=False):
    C, COUT = x.shape[1], g.shape[1]
    gw = torch.full((COUT, 9 * C), float("nan"), dtype=dtype, device=DEV)
    gb = torch.full((COUT,), float("nan"), dtype=dtype, device=DEV)
    ext.conv3x3p1_wrw(x, g, gw, gb, relu_in, any_hw=any_hw)
    return gw, gb


def _dgrad(ext, g, w, mask=None, any_hw=False):
    gx = torch.full((g.shape[0], w.shape[1], g.shape[2], g.shape[3]),
                    float("nan"), dtype=BF16, device=DEV).contiguous(
                        memory_format=torch.channels_last)
    ws = torch.empty(w.numel(), dtype=BF16, device=DEV)
    ext.conv3x3p1_dgrad(g, w, ws, gx, mask if mask is not None else _empty(),
                        any_hw=any_hw)
    return gx


def _between_nans(t):
    big = torch.full((t.shape[0] + 2, *t.shape[1:]), float("nan"), device=DEV,
                     dtype=BF16).contiguous(memory_format=torch.channels_last)
    big[1:-1] = t
    v = big[1:-1]
    assert v.is_contiguous(memory_format=torch.channels_last)
    assert v.data_ptr() != big.data_ptr()
    return v


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(
        a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32),
        b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


# ---------------------------------------------------------------------------
# exact-grid inputs: no tolerance
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_fwd_and_dgrad_exact(ext, shape):
    """Forward (through the public op) and masked input gradient equal the
    float64 reference rounded once to bf16, bit for bit."""
    from distributed_rl_amd import ops

    H, W, N = shape
    for C, COUT in RC.FWD_PAIRS:
        d = RC.make_case(H, W, N, C, COUT)
        x, w, r, g = (_cl(d[k]) for k in ("x", "w", "r", "g"))
        b = d["b"].to(device=DEV, dtype=BF16)
        out = ops.fused_conv3x3(x, w, b, residual=r)
        assert out.is_contiguous(memory_format=torch.channels_last)
        assert _same_bits(out.cpu(), d["out"].to(BF16)), (shape, C, COUT)
        out = ops.fused_conv3x3(x, w, b, relu_in=True, relu_out=True)
        assert _same_bits(out.cpu(), d["out_rr"].to(BF16)), (shape, C, COUT)
        # input gradient of this conv: the forward kernel at (COUT -> C)
        gx = _dgrad(ext, g, w)
        assert _same_bits(gx.cpu(), d["gx"].to(BF16)), (shape, C, COUT)
        gx = _dgrad(ext, g, w, mask=x)
        assert _same_bits(gx.cpu(), d["gx_masked"].to(BF16)), (shape, C, COUT)


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_wrw_exact(ext, shape):
    """gw / gb into the fp32 workspace equal float64 exactly, whatever the
    m-grid; the bf16 store equals that rounded once; two calls agree."""
    H, W, _ = shape
    for (C, COUT), rows in RC.WRW_ROWS.items():
        N = RC.wrw_batch(H, W, rows)
        d = RC.make_case(H, W, N, C, COUT)
        x, g = _cl(d["x"]), _cl(d["g"])
        gw, gb = _wrw(ext, x, g)
        assert torch.equal(gw.double().cpu(), d["gw"]), (shape, C, COUT, N)
        assert torch.equal(gb.double().cpu(), d["gb"]), (shape, C, COUT, N)
        gw_r, _ = _wrw(ext, x, g, relu_in=True)
        assert torch.equal(gw_r.double().cpu(), d["gw_relu"]), (shape, C, COUT)
        gw16, gb16 = _wrw(ext, x, g, dtype=BF16)
        assert _same_bits(gw16, gw.to(BF16)) and _same_bits(gb16, gb.to(BF16))
        again = _wrw(ext, x, g)
        assert _same_bits(again[0], gw) and _same_bits(again[1], gb)


def _gw_ref64_on_device(x, g):
    """float64 weight gradient as one im2col product on the device:
    (COUT, 9C) in (kh, kw, c) order, and gb."""
    N, C, H, W = x.shape
    COUT = g.shape[1]
    cols = F.unfold(x.double(), 3, padding=1)            # (N, C*9, HW)
    gm = g.double().reshape(N, COUT, H * W)
    gw = torch.einsum("nol,nkl->ok", gm, cols)           # (COUT, (c, tap))
    gw = gw.view(COUT, C, 9).permute(0, 2, 1).reshape(COUT, 9 * C)
    return gw, gm.sum((0, 2))


def _assert_exact_by_the_data(x, g):
    """M may exceed 2^17 here, so exactness is shown from the data: every
    fp32 partial sum of gw is bounded by sum |g||x| (units of 1/16) and of
    gb by sum |g| (units of 1/4); below 2^24 units they are exact."""
    bound_gw, bound_gb = _gw_ref64_on_device(x.abs(), g.abs())
    assert bound_gw.max().item() * 16 < 2 ** 24
    assert bound_gb.max().item() * 4 < 2 ** 24


@pytest.mark.parametrize("pair", list(RC.WRW_ROWS),
                         ids=lambda p: f"{p[0]}to{p[1]}")
def test_wrw_capped_m_grid(ext, pair):
    """64x64 at a batch where the 16 MiB plane budget or the residency, not
    the 8-passes rule, sets the m-grid: the wanted block count, computed
    from the rules, exceeds the cap, and the launch's plan is the cap.
    Exact-grid inputs: gw / gb equal float64 exactly whatever the m-grid."""
    C, COUT = pair
    rows = RC.WRW_ROWS[pair]
    H = W = 64
    n_elem = COUT * 9 * C
    pad = ext.wrw_plane_pad()
    resident = ext.conv3x3p1_wrw_plan(1, H, W, C, COUT)[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert resident > 0 and resident % cus == 0
    cap = (16 << 20) // ((n_elem + pad) * 4)
    limit = min(cap, resident)
    N = (8 * rows * (limit + 1) + H * W - 1) // (H * W)
    mb, want, _ = RC.m_grid(N * H * W, rows, n_elem, pad, resident)
    print(f"{pair}: N={N} wanted {want} blocks, plane cap {cap}, "
          f"resident {resident}")
    assert want > limit and mb == limit
    assert tuple(ext.conv3x3p1_wrw_plan(N, H, W, C, COUT)) == \
        (limit, rows, resident)
    gen = torch.Generator().manual_seed(31)
    x = _cl(RC.grid((N, C, H, W), 0.25, 2.0, gen))
    g = _cl(RC.grid((N, COUT, H, W), 0.25, 2.0, gen))
    _assert_exact_by_the_data(x, g)
    ref_gw, ref_gb = _gw_ref64_on_device(x, g)
    gw, gb = _wrw(ext, x, g)
    assert torch.equal(gw.double(), ref_gw), pair
    assert torch.equal(gb.double(), ref_gb), pair
    again = _wrw(ext, x, g)
    assert _same_bits(again[0], gw) and _same_bits(again[1], gb)
    gw16, gb16 = _wrw(ext, x, g, dtype=BF16)
    assert _same_bits(gw16, gw.to(BF16)) and _same_bits(gb16, gb.to(BF16))


def test_wrw_plan_of_the_runtime_path(ext):
    """The m-grid of the run-time path comes from the run-time entry's rows
    per pass and residency, not the table entry's: conv3x3p1_wrw_plan is
    what the launch uses. At 11x11, N = 3 (M = 363) the table entry (32
    rows) runs 12 passes on 2 blocks, the run-time entry (64) 6 on 1."""
    pad = ext.wrw_plane_pad()
    for H, W, C, COUT, table_rows in RC.TABLE:
        rows = RC.WRW_ROWS[(C, COUT)]
        for N in (3, 64):
            M = N * H * W
            n_elem = COUT * 9 * C
            mb, r, resident = ext.conv3x3p1_wrw_plan(N, H, W, C, COUT,
                                                     any_hw=True)
            assert r == rows, (H, W, C, COUT)
            assert mb == RC.m_grid(M, rows, n_elem, pad, resident)[0]
            tmb, tr, tres = ext.conv3x3p1_wrw_plan(N, H, W, C, COUT)
            assert tr == table_rows
            assert tmb == RC.m_grid(M, table_rows, n_elem, pad, tres)[0]
    assert ext.conv3x3p1_wrw_plan(3, 11, 11, 32, 32)[:2] == (2, 32)
    assert ext.conv3x3p1_wrw_plan(3, 11, 11, 32, 32, any_hw=True)[:2] == (1, 64)
    # off the table both spellings are the run-time entry
    assert ext.conv3x3p1_wrw_plan(9, 5, 7, 16, 32) == \
        ext.conv3x3p1_wrw_plan(9, 5, 7, 16, 32, any_hw=True)
    with pytest.raises(RuntimeError, match="no 3x3 pad-1 wrw kernel"):
        ext.conv3x3p1_wrw_plan(9, 5, 7, 32, 16)


# ---------------------------------------------------------------------------
# run-time kernel against the table kernel (random-valued inputs, N = 3)
# ---------------------------------------------------------------------------


def _random_operands(H, W, C, COUT, n=3, seed=11):
    gen = torch.Generator().manual_seed(seed + H + C + COUT)
    x = _cl(torch.randn(n, C, H, W, generator=gen))
    w = _cl(torch.randn(COUT, C, 3, 3, generator=gen) * 0.05)
    b = (torch.randn(COUT, generator=gen) * 0.1).to(device=DEV, dtype=BF16)
    r = _cl(torch.randn(n, COUT, H, W, generator=gen))
    g = _cl(torch.randn(n, COUT, H, W, generator=gen))
    return x, w, b, r, g


@pytest.mark.parametrize(
    "geom", [t[:4] for t in RC.TABLE] + RC.TABLE_FWD_ONLY,
    ids=lambda g: "x".join(map(str, g)))
def test_runtime_kernel_gives_the_table_kernels_bits(ext, geom):
    H, W, C, COUT = geom
    x, w, b, r, g = _random_operands(H, W, C, COUT)
    for kw in [{}, dict(relu_in=True, relu_out=True), dict(r=r)]:
        a = _fwd(ext, x, w, b, **kw)
        h = _fwd(ext, x, w, b, any_hw=True, **kw)
        assert _same_bits(a, h), (geom, kw.keys())
    # masked input gradient of a (C -> COUT) conv whose mirrored geometry
    # this is: weight (C, COUT, 3, 3), gout has C channels
    wd = _cl(torch.randn(C, COUT, 3, 3,
                         generator=torch.Generator().manual_seed(3)) * 0.05)
    mask = _cl(torch.randn(3, COUT, H, W,
                           generator=torch.Generator().manual_seed(4)))
    a = _dgrad(ext, x, wd, mask=mask)
    h = _dgrad(ext, x, wd, mask=mask, any_hw=True)
    assert _same_bits(a, h) and torch.isfinite(a.float()).all()
    assert not torch.equal(a, _dgrad(ext, x, wd))


@pytest.mark.parametrize("geom", RC.TABLE, ids=lambda g: "x".join(map(str, g)))
def test_wrw_runtime_kernel_against_table_kernel(ext, geom):
    """N = 3 keeps the m-grid on the 8-passes rule for both kernels. Where
    both take the same rows per pass the planes, and so the bits, are the
    same; 11x11 runs 32 rows per pass in the table and 64 in the run-time
    entry, so there the bound is 1e-5 * scale against float64."""
    H, W, C, COUT, table_rows = geom
    x, _, _, _, g = _random_operands(H, W, C, COUT)
    a = _wrw(ext, x, g, relu_in=True)
    h = _wrw(ext, x, g, relu_in=True, any_hw=True)
    again = _wrw(ext, x, g, relu_in=True, any_hw=True)
    assert _same_bits(h[0], again[0]) and _same_bits(h[1], again[1])
    if table_rows == RC.WRW_ROWS[(C, COUT)]:
        assert _same_bits(a[0], h[0]) and _same_bits(a[1], h[1]), geom
    ref_gw, ref_gb = _gw_ref64_on_device(torch.relu(x), g)
    for got, ref in [(h[0], ref_gw), (h[1], ref_gb)]:
        err = (got.double() - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item(), geom


# ---------------------------------------------------------------------------
# halo, border count, flags
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("hw", [(2, 2, 70), (5, 7, 9), (1, 9, 3)],
                         ids=["2x2", "5x7", "1x9"])
def test_no_halo_reads(ext, hw):
    """The batch sits between two NaN images of one allocation: a tap read
    across an image border would pull a NaN into the result."""
    H, W, N = hw
    for C, COUT in RC.FWD_PAIRS:
        x, w, b, _, g = _random_operands(H, W, C, COUT, n=N)
        out = _fwd(ext, _between_nans(x), w, b)
        plain = _fwd(ext, _cl(x), w, b)
        assert torch.isfinite(out.float()).all()
        assert _same_bits(out, plain)
        if (C, COUT) in RC.WRW_ROWS:
            gw, gb = _wrw(ext, _between_nans(x), _between_nans(g))
            pw, pb = _wrw(ext, _cl(x), _cl(g))
            assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
            assert _same_bits(gw, pw) and _same_bits(gb, pb)


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_exact_border_count(ext, shape):
    """All-ones input and weights: out = C x (taps in bounds), exactly —
    1, 2 or 3 per axis at the 1- and 2-wide shapes."""
    from distributed_rl_amd import ops

    H, W, N = shape

    def taps(n):
        t = torch.full((n,), 3.0)
        t[0] -= 1
        t[-1] -= 1
        return t

    th, tw = taps(H), taps(W)
    assert (H > 1 or th.tolist() == [1.0]) and (H != 2 or th.tolist() == [2, 2])
    for C, COUT in RC.FWD_PAIRS:
        x = _cl(torch.ones(N, C, H, W))
        w = _cl(torch.ones(COUT, C, 3, 3))
        out = ops.fused_conv3x3(x, w, None)
        expect = (C * th[:, None] * tw[None, :]).expand(N, COUT, H, W)
        assert torch.equal(out.float().cpu(), expect), (shape, C, COUT)


def test_flag_identities(ext):
    from distributed_rl_amd import ops

    for C, COUT in RC.FWD_PAIRS:
        x, w, b, r, _ = _random_operands(5, 7, C, COUT, n=9)
        a = ops.fused_conv3x3(x, w, b, relu_in=True)
        assert torch.equal(a, ops.fused_conv3x3(torch.relu(x), w, b))
        o = ops.fused_conv3x3(x, w, b)
        assert torch.equal(ops.fused_conv3x3(x, w, b, relu_out=True),
                           torch.relu(o))
        z = ops.fused_conv3x3(x, torch.zeros_like(w), torch.zeros_like(b),
                              residual=r)
        assert torch.equal(z, r)


# ---------------------------------------------------------------------------
# rejections: each raises before any launch and names the argument
# ---------------------------------------------------------------------------

RH, RW, RC_, RCOUT = 5, 7, 16, 32


def _args():
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    clz = lambda *s: z(*s).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    return dict(x=clz(2, RC_, RH, RW), w=clz(RCOUT, RC_, 3, 3), b=z(RCOUT),
                out=clz(2, RCOUT, RH, RW), g=clz(2, RCOUT, RH, RW),
                gx=clz(2, RC_, RH, RW),
                gw=z(RCOUT, 9 * RC_, dt=torch.float32),
                gb=z(RCOUT, dt=torch.float32))


def _misaligned_weight():
    flat = torch.zeros(RCOUT * 9 * RC_ + 8, dtype=BF16, device=DEV)
    w = flat[1:1 + RCOUT * 9 * RC_].view(RCOUT, 3, 3, RC_).permute(0, 3, 1, 2)
    assert w.is_contiguous(memory_format=torch.channels_last)
    assert w.data_ptr() % 16 == 2
    return w


def test_rejections(ext):
    e = _empty

    def fwd(a):
        ext.conv3x3p1_fwd(a["x"], a["w"], a["b"], e(), a["out"], False, False)

    def wrw(a):
        ext.conv3x3p1_wrw(a["x"], a["g"], a["gw"], a["gb"], False)

    def dgrad(a):
        ws = torch.empty(a["w"].numel(), dtype=BF16, device=DEV)
        ext.conv3x3p1_dgrad(a["g"], a["w"], ws, a["gx"], e())

    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    clz = lambda *s: z(*s).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    spoil = [
        ("(C, COUT) = (8, 16)", fwd, "no 3x3 pad-1 conv kernel for this "
         "geometry",
         lambda a: a.update(x=clz(2, 8, RH, RW), w=clz(16, 8, 3, 3),
                            b=z(16), out=clz(2, 16, RH, RW))),
        ("(C, COUT) = (8, 16) wrw", wrw, "no 3x3 pad-1 wrw kernel for this "
         "geometry",
         lambda a: a.update(x=clz(2, 8, RH, RW), g=clz(2, 16, RH, RW),
                            gw=z(16, 72, dt=torch.float32),
                            gb=z(16, dt=torch.float32))),
        ("out of another H", fwd, "conv3x3p1_fwd output",
         lambda a: a.update(out=clz(2, RCOUT, RH + 1, RW))),
        ("gout of another H", wrw, "conv3x3p1_wrw gout",
         lambda a: a.update(g=clz(2, RCOUT, RH + 1, RW))),
        ("gx of another H", dgrad, "conv3x3p1_dgrad gx",
         lambda a: a.update(gx=clz(2, RC_, RH + 1, RW))),
        ("nchw input", fwd, "conv3x3p1_fwd input",
         lambda a: a.update(x=z(2, RC_, RH, RW))),
        ("nchw x wrw", wrw, "conv3x3p1_wrw x",
         lambda a: a.update(x=z(2, RC_, RH, RW))),
        ("fp32 input", fwd, "conv3x3p1_fwd input",
         lambda a: a.update(x=a["x"].float())),
        ("fp32 gout", dgrad, "conv3x3p1_dgrad gout",
         lambda a: a.update(g=a["g"].float())),
        ("cpu input", fwd, "conv3x3p1_fwd input",
         lambda a: a.update(x=a["x"].cpu())),
        ("cpu gout wrw", wrw, "conv3x3p1_wrw gout",
         lambda a: a.update(g=a["g"].cpu())),
        ("misaligned weight view", fwd, "weight is misaligned",
         lambda a: a.update(w=_misaligned_weight())),
        ("out aliasing in", fwd, "must not alias",
         lambda a: a.update(x=clz(2, 16, RH, RW), w=clz(16, 16, 3, 3),
                            b=z(16), out=None)),
    ]
    fwd(_args())
    wrw(_args())
    dgrad(_args())  # the unspoiled calls pass
    for name, call, names_arg, change in spoil:
        a = _args()
        change(a)
        if a["out"] is None:
            a["out"] = a["x"]
        with pytest.raises(RuntimeError, match=names_arg):
            call(a)
            pytest.fail(f"{name} was accepted")
    # a valid call afterwards still works
    a = _args()
    a["x"].fill_(1.0)
    a["w"].fill_(1.0)
    a["g"].fill_(1.0)
    fwd(a)
    wrw(a)
    torch.cuda.synchronize()
    assert a["out"][0, 0, 1, 1] == 9 * RC_
    assert a["out"][0, 0, 0, 0] == 4 * RC_
    assert a["gw"][0, 4 * RC_] == 2 * RH * RW  # centre tap: every pixel


# ---------------------------------------------------------------------------
# the torso at 32x24 (sections 16x12, 8x6, 4x3)
# ---------------------------------------------------------------------------


def _torso():
    import copy

    from distributed_rl_amd.models.base_agent import ImpalaResNet

    torch.manual_seed(5)
    ref = ImpalaResNet(dict(iSize=4, channels=[16, 32, 32], nBlocks=2)).to(DEV)
    net = copy.deepcopy(ref).to(memory_format=torch.channels_last).to(BF16)
    return ref, net


def _count(monkeypatch, names):
    from distributed_rl_amd import ops

    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(ops, n)

        def counting(*a, _real=real, _n=n, **kw):
            calls[_n] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ops, n, counting)
    return calls


OPS = ["fused_conv3x3", "fused_stem_conv3x3", "fused_maxpool3x3s2"]


def _frames():
    gen = torch.Generator().manual_seed(9)
    return _cl(torch.rand(2, 4, 32, 24, generator=gen))


def test_model_all_gates_on(ext, monkeypatch):
    """All gates on: 15 convs and 3 pools on the own ops, no library
    backward when the frames need no gradient, and as close to the fp32
    model as the library bf16 path (test_model_fused_path's rule)."""
    for gate in ("DRL_OWN_RESCONV", "DRL_OWN_RESCONV_WRW",
                 "DRL_OWN_RESCONV_DGRAD", "DRL_OWN_STEM", "DRL_OWN_STEM_WRW",
                 "DRL_OWN_POOL"):
        monkeypatch.setenv(gate, "1")
    ref, net = _torso()
    x = _frames()
    calls = _count(monkeypatch, OPS)
    lib_bwd = []
    from torch.utils._python_dispatch import TorchDispatchMode

    class _NoLibBackward(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.convolution_backward.default:
                lib_bwd.append(1)
            return func(*args, **(kwargs or {}))

    with _NoLibBackward():
        y = net(x)
        grads = torch.autograd.grad(y.float().square().sum(),
                                    list(net.parameters()))
    assert calls == dict(fused_conv3x3=14, fused_stem_conv3x3=1,
                         fused_maxpool3x3s2=3), calls
    assert not lib_bwd, "aten.convolution_backward ran"
    assert all(torch.isfinite(g.float()).all() for g in grads)
    with torch.no_grad():
        y_ref = ref(x.float())
        y_own = net(x)
        for gate in ("DRL_OWN_RESCONV", "DRL_OWN_STEM", "DRL_OWN_POOL"):
            monkeypatch.setenv(gate, "0")
        y_lib = net(x)
    err_own = (y_own.float() - y_ref).abs().max().item()
    err_lib = (y_lib.float() - y_ref).abs().max().item()
    print(f"32x24 torso: own err {err_own:.4g}, library bf16 err {err_lib:.4g}")
    assert err_own <= 2 * err_lib


def test_model_graph_replay_is_reproducible(ext, monkeypatch):
    """A captured forward+backward replays twice to bit-equal output and
    bit-equal gradients of every parameter (ordered sums everywhere)."""
    for gate in ("DRL_OWN_RESCONV", "DRL_OWN_STEM", "DRL_OWN_POOL"):
        monkeypatch.setenv(gate, "1")
    _, net = _torso()
    x = _frames()
    params = list(net.parameters())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(net(x).float().square().sum(), params)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = net(x)
        grads = torch.autograd.grad(y.float().square().sum(), params)
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append([y.clone()] + [g.clone() for g in grads])
    assert seen[0][0].abs().max() > 0
    for a, b in zip(*seen):
        assert torch.isfinite(a.float()).all()
        assert _same_bits(a, b)


def test_model_gates_unset(ext, monkeypatch):
    """Environment unset: the stem stays in torch, everything else runs on
    the own kernels."""
    for gate in ("DRL_OWN_RESCONV", "DRL_OWN_RESCONV_WRW",
                 "DRL_OWN_RESCONV_DGRAD", "DRL_OWN_STEM", "DRL_OWN_STEM_WRW",
                 "DRL_OWN_POOL"):
        monkeypatch.delenv(gate, raising=False)
    _, net = _torso()
    calls = _count(monkeypatch, OPS)
    y = net(_frames())
    torch.autograd.grad(y.float().square().sum(), list(net.parameters()))
    assert calls == dict(fused_conv3x3=14, fused_stem_conv3x3=0,
                         fused_maxpool3x3s2=3), calls
    assert torch.isfinite(y.float()).all()
