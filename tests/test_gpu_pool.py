"""Hand-written NHWC bf16 max-pool 3x3 stride 2 pad 1
(maxpool3x3s2_fwd_kernel / maxpool3x3s2_bwd_kernel): forward bits and tap
plane against the CPU library, no halo reads, the ordered gather backward,
argument checks, the autograd op, the model gate and graph capture.

Operands are built once on the CPU from a seeded generator, rounded to bf16,
and never written."""

import pytest
import torch
import torch.nn.functional as F

from test_pool_ref import KINDS, SHAPES, IDS, make_x
from test_pool_ref import bits as _bits, picked_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def data():
    """Per (shape, kind): CPU x, the CPU library's out and tap plane, a CPU
    gout, and the device copies."""
    from distributed_rl_amd.ops import torch_ref

    out = {}
    gen = torch.Generator().manual_seed(23)
    for shape in SHAPES:
        for kind in KINDS:
            x = make_x(shape, kind)
            want, taps = torch_ref.maxpool3x3s2_taps(x)
            g = _cl(torch.randn(want.shape, generator=gen).to(BF16))
            out[(shape, kind)] = dict(
                x=x, want=want, taps=taps, g=g, xd=x.to(DEV),
                tapsd=_cl(taps.to(DEV)), gd=g.to(DEV))
    return out


CASES = [(s, k) for s in SHAPES for k in KINDS]
CASE_IDS = [f"{i}-{k}" for i in IDS for k in KINDS]


def _fwd(ext, x, with_idx=True):
    N, C, H, W = x.shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.full((N, C, P, Q), float("nan"), dtype=BF16,
                     device=DEV).contiguous(memory_format=torch.channels_last)
    if with_idx:
        idx = torch.full((N, C, P, Q), 255, dtype=torch.uint8, device=DEV
                         ).contiguous(memory_format=torch.channels_last)
    else:
        idx = torch.empty(0, dtype=torch.uint8, device=DEV)
    ext.maxpool3x3s2_fwd(x, out, idx)
    return out, idx


def _bwd(ext, g, taps, H, W):
    N, C = g.shape[:2]
    gx = torch.full((N, C, H, W), float("nan"), dtype=BF16, device=DEV
                    ).contiguous(memory_format=torch.channels_last)
    ext.maxpool3x3s2_bwd(g, taps, gx)
    return gx


def _between_nans(t, fill=float("nan")):
    """t as a slice of one allocation with a NaN (255 for the uint8 plane)
    image on either side."""
    big = torch.full((t.shape[0] + 2, *t.shape[1:]), fill, device=DEV,
                     dtype=t.dtype).contiguous(
                         memory_format=torch.channels_last)
    big[1:-1] = t
    s = big[1:-1]
    assert s.is_contiguous(memory_format=torch.channels_last)
    assert s.data_ptr() != big.data_ptr()
    return s


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_bits_and_taps(ext, data, case):
    d = data[case]
    out, idx = _fwd(ext, d["xd"])
    assert torch.equal(_bits(out), _bits(d["want"]))
    assert torch.equal(idx.cpu(), d["taps"])
    # the winner's bits go through as they are, a NaN's payload included
    assert torch.equal(out.cpu().view(torch.int16),
                       picked_bits(d["x"], d["taps"]))
    # no index plane: same output
    out2, _ = _fwd(ext, d["xd"], with_idx=False)
    assert torch.equal(_bits(out2), _bits(d["want"]))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_reads_no_halo(ext, data, shape):
    d = data[(shape, "randn")]
    out, idx = _fwd(ext, _between_nans(d["xd"]))
    assert torch.isfinite(out.float()).all()
    assert torch.equal(_bits(out), _bits(d["want"]))
    assert torch.equal(idx.cpu(), d["taps"])


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", [c for c in CASES if c[1] != "special"],
                         ids=[i for i in CASE_IDS if "special" not in i])
def test_backward(ext, data, case):
    from distributed_rl_amd.ops import torch_ref

    d = data[case]
    H, W = d["x"].shape[2:]
    gx = _bwd(ext, d["gd"], d["tapsd"], H, W)
    # bit-equal to the ordered fp32 sum rounded once: every element written
    want = torch_ref.maxpool3x3s2_bwd(d["g"], d["taps"], H, W).to(BF16)
    assert torch.equal(_bits(gx), _bits(want))
    # against float64 autograd of the library, |gx - ref| <= 2^-8 * S with
    # S the same backward of |gout|: the one rounding to bf16 (8 significant
    # bits) moves a value in [2^e, 2^(e+1)) by at most half an ulp,
    # 2^-8 * 2^e <= 2^-8 * |sum| <= 2^-8 * S; the fp32 sum of at most four
    # bf16 terms adds 2^-23 relative at most, and only when the terms lie
    # 2^16 apart. Measured: up to 0.00389 * S (2^-8 = 0.00391).
    xd = d["x"].double().requires_grad_(True)
    y = F.max_pool2d(xd, 3, 2, 1)
    (ref,) = torch.autograd.grad(y, xd, d["g"].double(), retain_graph=True)
    (S,) = torch.autograd.grad(y, xd, d["g"].double().abs())
    err = (gx.cpu().double() - ref).abs()
    print(f"{case}: max err/S {(err / S.clamp_min(1e-30)).max().item():.3g}")
    assert (err <= 2.0 ** -8 * S).all()
    # deterministic
    again = _bwd(ext, d["gd"], d["tapsd"], H, W)
    assert torch.equal(_bits(gx), _bits(again))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_reads_no_halo(ext, data, shape):
    d = data[(shape, "ties")]
    H, W = d["x"].shape[2:]
    plain = _bwd(ext, d["gd"], d["tapsd"], H, W)
    gx = _bwd(ext, _between_nans(d["gd"]), _between_nans(d["tapsd"], 255),
              H, W)
    assert torch.isfinite(gx.float()).all()
    assert torch.equal(_bits(gx), _bits(plain))


# ---------------------------------------------------------------------------
# argument checks: each raises before any launch
# ---------------------------------------------------------------------------


def _args(N=2, H=6, W=5, C=16):
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    mk = lambda *s, dt=BF16: _cl(torch.zeros(*s, dtype=dt, device=DEV))  # noqa: E731
    return dict(x=mk(N, C, H, W), out=mk(N, C, P, Q),
                idx=mk(N, C, P, Q, dt=torch.uint8), g=mk(N, C, P, Q),
                gx=mk(N, C, H, W))


def test_rejections(ext):
    def fwd(a):
        ext.maxpool3x3s2_fwd(a["x"], a["out"], a["idx"])

    def bwd(a):
        ext.maxpool3x3s2_bwd(a["g"], a["idx"], a["gx"])

    fwd(_args())
    bwd(_args())  # the unspoiled calls pass
    spoil = [
        ("cpu x", fwd, lambda a: a.update(x=a["x"].cpu())),
        ("cpu gout", bwd, lambda a: a.update(g=a["g"].cpu())),
        ("fp16 x", fwd, lambda a: a.update(x=a["x"].half())),
        ("nchw x", fwd, lambda a: a.update(x=a["x"].contiguous())),
        ("nchw gout", bwd, lambda a: a.update(g=a["g"].contiguous())),
        ("out of the wrong P", fwd,
         lambda a: a.update(out=_cl(torch.zeros(2, 16, 4, 3, dtype=BF16,
                                                device=DEV)))),
        ("int64 idx fwd", fwd, lambda a: a.update(idx=a["idx"].long())),
        ("int64 idx bwd", bwd, lambda a: a.update(idx=a["idx"].long())),
        ("gx of the wrong H", bwd,
         lambda a: a.update(gx=_cl(torch.zeros(2, 16, 8, 5, dtype=BF16,
                                               device=DEV)))),
    ]
    for name, call, change in spoil:
        a = _args()
        change(a)
        with pytest.raises(RuntimeError):
            call(a)
            pytest.fail(f"{name} was accepted")
    for call in (fwd, bwd):
        with pytest.raises(RuntimeError):
            call(_args(C=8))
    assert ext.maxpool3x3s2_supported(84, 84, 16)
    assert ext.maxpool3x3s2_supported(1, 1, 32)
    assert not ext.maxpool3x3s2_supported(84, 84, 8)
    assert not ext.maxpool3x3s2_supported(84, 84, 24)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# autograd op
# ---------------------------------------------------------------------------


def test_op_autograd_saves_only_the_tap_plane(ext, data):
    from distributed_rl_amd import ops
    from distributed_rl_amd.ops import torch_ref

    d = data[((2, 21, 21, 32), "ties")]
    H, W = d["x"].shape[2:]
    saved = []
    x = d["xd"].clone(memory_format=torch.channels_last).requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(
            lambda t: saved.append((t.dtype, t.numel())) or t, lambda t: t):
        y = ops.fused_maxpool3x3s2(x)
    assert torch.equal(_bits(y), _bits(d["want"]))
    assert saved == [(torch.uint8, y.numel())], saved
    # a gout that is not channels_last is accepted
    (gx,) = torch.autograd.grad(y, x, d["gd"].contiguous())
    assert gx.is_contiguous(memory_format=torch.channels_last)
    want = torch_ref.maxpool3x3s2_bwd(d["g"], d["taps"], H, W).to(BF16)
    assert torch.equal(_bits(gx), _bits(want))
    # no gradient wanted: no plane at all
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(
            lambda t: saved.append((t.dtype, t.numel())) or t, lambda t: t):
        y2 = ops.fused_maxpool3x3s2(d["xd"])
    assert torch.equal(y2, y.detach()) and not saved


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------


def _torso():
    from distributed_rl_amd.models.base_agent import ImpalaResNet

    torch.manual_seed(5)
    net = ImpalaResNet({"iSize": 4, "channels": [16, 32, 32], "nBlocks": 2})
    return net.to(DEV).to(memory_format=torch.channels_last).to(BF16)


def _count_pool(monkeypatch):
    from distributed_rl_amd import ops

    calls = []
    real = ops.fused_maxpool3x3s2

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "fused_maxpool3x3s2", counting)
    return calls


@pytest.mark.parametrize("resconv", ["1", "0"])
def test_model_gate(ext, monkeypatch, resconv):
    """Gate open: all three pools take the op, whatever the conv gate says,
    and the (exact) forward does not change. Gate closed: the op is not
    called."""
    monkeypatch.setenv("DRL_OWN_RESCONV", resconv)
    net = _torso()
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV).to(BF16))
    calls = _count_pool(monkeypatch)
    with torch.no_grad():
        monkeypatch.setenv("DRL_OWN_POOL", "1")
        y_own = net(x)
        assert len(calls) == 3
        monkeypatch.setenv("DRL_OWN_POOL", "0")
        y_lib = net(x)
        assert len(calls) == 3, "DRL_OWN_POOL=0 must not use the kernel"
    assert y_own.abs().max() > 0
    assert torch.equal(y_own, y_lib)


def test_model_graph_capture(ext, monkeypatch):
    """One captured forward+backward of the bare torso, all gates at their
    defaults and the pool gate open: two replays give bit-equal output and
    bit-equal gradients for every parameter but the first conv's weight,
    whose library split-K sum is atomic."""
    for name in ("DRL_OWN_RESCONV", "DRL_OWN_RESCONV_WRW",
                 "DRL_OWN_RESCONV_DGRAD"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DRL_OWN_POOL", "1")
    net = _torso()
    calls = _count_pool(monkeypatch)
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV).to(BF16))
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(net(x).float().square().sum(), params)
    torch.cuda.current_stream().wait_stream(side)
    assert len(calls) == 6

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
    assert any(a.float().abs().max() > 0 for a in seen[0][1:])
    # body.0.weight: the first conv (84x84, C=4) stays on the library, whose
    # weight gradient sums split-K partials with atomics
    assert [n for n in differ if n != "body.0.weight"] == []
