"""The stem conv on uint8 (N, 4, H, W) frames (conv3x3c4_u8_*_kernel): bit
for bit against fp64 on inputs whose fp32 sums are exact in any order
(stem_u8_cases.py). Frames, out and gout sit inside larger allocations of the
test's own: a wrong address reads 255 or NaN, or breaks a sentinel."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_u8_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
C, COUT = SC.C, SC.COUT
SENTINEL = -3.0


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _guarded(t, fill, dtype, channels_last=True):
    """t on the device between guard images of `fill` (at least 64 pixels on
    each side); returns (view of t's place, the guards)."""
    n = 64 // (t.shape[2] * t.shape[3]) + 1
    big = torch.full((t.shape[0] + 2 * n, *t.shape[1:]), fill, device=DEV,
                     dtype=dtype)
    if channels_last:
        big = big.contiguous(memory_format=torch.channels_last)
    big[n:-n] = t.to(device=DEV, dtype=dtype)
    return big[n:-n], (big[:n], big[-n:])


def _intact(guards, fill):
    return all(bool((g != g).all()) if fill != fill else bool((g == fill).all())
               for g in guards)


def _frames(d):
    return _guarded(d["frames"], 255, torch.uint8, channels_last=False)[0]


def _fwd(ext, frames, w, b):
    N, _, H, W = frames.shape
    out, guards = _guarded(torch.full((N, COUT, H, W), float("nan")),
                           SENTINEL, BF16)
    ext.conv3x3c4_u8_fwd(frames, w, b, out)
    assert _intact(guards, SENTINEL)
    return out


def _w(d):
    return d["w"].to(device=DEV, dtype=BF16).contiguous(
        memory_format=torch.channels_last)


@pytest.mark.parametrize("shape", SC.SHAPES, ids=SC.IDS)
def test_fwd_exact(ext, shape):
    d = SC.case(shape)
    out = _fwd(ext, _frames(d), _w(d), d["b"].to(device=DEV, dtype=BF16))
    assert torch.equal(out.cpu(), d["out"].to(BF16))
    nob = _fwd(ext, _frames(d), _w(d), torch.empty(0, device=DEV, dtype=BF16))
    assert torch.equal(nob.cpu(), (d["out"] - d["b"].view(1, -1, 1, 1)).to(BF16))


@pytest.mark.parametrize("shape,regime", SC.WRW_CASES, ids=SC.WRW_IDS)
def test_wrw_exact(ext, shape, regime):
    d = SC.case(shape, regime)
    frames = _frames(d)
    g, guards = _guarded(d["g"], float("nan"), BF16)
    for dtype in (torch.float32, BF16):
        for with_gb in (True, False):
            gw = torch.full((COUT, 9 * C), float("nan"), dtype=dtype,
                            device=DEV)
            gb = torch.full((COUT if with_gb else 0,), float("nan"),
                            dtype=dtype, device=DEV)
            ext.conv3x3c4_u8_wrw(frames, g, gw, gb)
            assert torch.equal(gw.cpu(), d["gw"].to(dtype)), (dtype, with_gb)
            assert not with_gb or torch.equal(gb.cpu(), d["gb"].to(dtype))
    again = torch.empty_like(gw), torch.empty(COUT, dtype=BF16, device=DEV)
    ext.conv3x3c4_u8_wrw(frames, g, *again)
    assert torch.equal(again[0], gw) and torch.equal(again[1].cpu(),
                                                     d["gb"].to(BF16))
    assert _intact(guards, float("nan"))


def test_op_backward(ext):
    from distributed_rl_amd import ops

    d = SC.case((2, 13, 12))
    w = _w(d).requires_grad_(True)
    b = d["b"].to(device=DEV, dtype=BF16).requires_grad_(True)
    out = ops.fused_stem_conv3x3_u8(_frames(d), w, b)
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out.cpu(), d["out"].to(BF16))
    assert out.grad_fn.next_functions[0][0] is None  # no gradient to frames
    gw, gb = torch.autograd.grad(out, [w, b], _guarded(d["g"], 0.0, BF16)[0])
    assert torch.equal(gw.permute(0, 2, 3, 1).reshape(COUT, 9 * C).cpu(),
                       d["gw"].to(BF16))
    assert torch.equal(gb.cpu(), d["gb"].to(BF16))


def test_model_u8_input(ext, monkeypatch):
    """DRL_STEM_U8=1 on uint8 frames against DRL_OWN_STEM=1 on the
    dequantised copy: both forwards are exact on a 1/4-grid stem weight and
    bias, so the rest of the net sees the same bits. body.0.weight's own
    gradient sums the net's (non-grid) gout in another order than K2d's
    kernel, so its equality is a property of these inputs: measured equal at
    the kernel's 6 band rows; at 12, 1 of its 576 elements differed by 2^-11
    (one bf16 ulp), everything else equal."""
    from distributed_rl_amd import ops
    from distributed_rl_amd.models.base_agent import ImpalaResNet

    torch.manual_seed(5)
    net = ImpalaResNet({"iSize": 4}).to(device=DEV, dtype=BF16).to(
        memory_format=torch.channels_last)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        net.body[0].weight.copy_(SC._quarters((COUT, C, 3, 3), gen))
        net.body[0].bias.copy_(SC._quarters((COUT,), gen))
    frames = torch.randint(0, 256, (3, C, 20, 24), generator=gen,
                           dtype=torch.uint8).to(DEV)

    def run(x, **env):
        for k in ("DRL_STEM_U8", "DRL_OWN_STEM"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        y = net(x)
        coef = torch.linspace(-1, 1, y.numel(), device=DEV).view_as(y)
        return y, torch.autograd.grad((y.float() * coef).sum(),
                                      list(net.parameters()))

    y_ref, g_ref = run(ops.dequant_frames_nhwc(frames), DRL_OWN_STEM="1")
    y_u8, g_u8 = run(frames, DRL_STEM_U8="1")
    assert torch.equal(y_u8, y_ref)
    differ = [(name, (a.float() - b.float()).abs().max().item(),
               int((a != b).sum()), a.numel())
              for (name, _), a, b in zip(net.named_parameters(), g_u8, g_ref)
              if not torch.equal(a, b)]
    print("gradients that differ (name, max |diff|, elements, of):", differ)
    # gate unset: the frames are dequantised and take today's path
    assert torch.equal(run(frames)[0],
                       run(ops.dequant_frames_nhwc(frames))[0])
    assert not differ


def test_rejections(ext):
    """One spoiled argument per call; the error names it."""
    def args():
        z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)  # noqa: E731
        return dict(x=z(2, C, 5, 7, dt=torch.uint8), w=cl(z(COUT, C, 3, 3)),
                    b=z(COUT), out=cl(z(2, COUT, 5, 7)),
                    g=cl(z(2, COUT, 5, 7)), gw=z(COUT, 9 * C, dt=torch.float32),
                    gb=z(COUT, dt=torch.float32))

    def fwd(a):
        ext.conv3x3c4_u8_fwd(a["x"], a["w"], a["b"], a["out"])

    def wrw(a):
        ext.conv3x3c4_u8_wrw(a["x"], a["g"], a["gw"], a["gb"])

    spoil = [
        (fwd, "conv3x3c4_u8_fwd x", lambda a: a.update(x=a["x"].cpu())),
        (wrw, "conv3x3c4_u8_wrw x", lambda a: a.update(x=a["x"].char())),
        (fwd, "conv3x3c4_u8_fwd x", lambda a: a.update(
            x=a["x"].transpose(2, 3).contiguous().transpose(2, 3))),
        (fwd, "conv3x3c4_u8_fwd x", lambda a: a.update(x=a["x"][:, :3])),
        (fwd, "conv3x3c4_u8_fwd out",
         lambda a: a.update(out=a["out"][:, :, :4])),
        (wrw, "conv3x3c4_u8_wrw gw is misaligned", lambda a: a.update(
            gw=torch.zeros(577, device=DEV)[1:].view(COUT, 9 * C))),
    ]
    fwd(args())
    wrw(args())
    for call, names_arg, change in spoil:
        a = args()
        change(a)
        with pytest.raises(RuntimeError, match=names_arg):
            call(a)
    assert not ext.conv3x3c4_u8_supported(5, 7, 3, COUT)
    assert ext.conv3x3c4_u8_supported(1, 512, C, COUT)
    assert ext.conv3x3c4_u8_plan(2, 13, 12)[:2] == (12, 6)
