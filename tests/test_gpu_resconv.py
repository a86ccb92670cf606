"""Hand-written MFMA 3x3 stride-1 pad-1 conv (conv3x3p1_fwd_kernel) for the
IMPALA-ResNet torso: forward against fp32 on bf16-rounded operands, exact
border handling, flag identities, block backward, the model path and
hipGraph capture.

N=3 makes M = 5292 / 1323 / 363 rows: never a multiple of a block's rows
(256 or 128), so every geometry runs more than one block and a ragged tail.
"""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

GEOMS = [
    # (H, W, C, COUT) — cfg/impala_resnet.json at 84x84
    (42, 42, 16, 16),
    (42, 42, 16, 32),
    (21, 21, 32, 32),
    (11, 11, 32, 32),
]
N = 3


def _cl(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def operands(ext):
    """bf16-rounded (x, w, b, r) per geometry, built once and never written."""
    out = {}
    gen = torch.Generator(device=DEV).manual_seed(11)
    for (H, W, C, COUT) in GEOMS:
        x = _cl(torch.randn(N, C, H, W, device=DEV, generator=gen))
        w = _cl(torch.randn(COUT, C, 3, 3, device=DEV, generator=gen) * 0.05)
        b = (torch.randn(COUT, device=DEV, generator=gen) * 0.1).to(
            torch.bfloat16)
        r = _cl(torch.randn(N, COUT, H, W, device=DEV, generator=gen))
        out[(H, W, C, COUT)] = (x, w, b, r)
    return out


def _ref(x, w, b, relu_in=False, relu_out=False, residual=None):
    from distributed_rl_amd.ops import torch_ref

    return torch_ref.conv3x3_res(
        x.float(), w.float(), None if b is None else b.float(), relu_in,
        relu_out, None if residual is None else residual.float())


def test_supported_geometries(ext):
    for g in GEOMS:
        assert ext.conv3x3p1_supported(*g)
    # the first conv (C=4, K=36) stays on the library
    assert not ext.conv3x3p1_supported(84, 84, 4, 16)


@pytest.mark.parametrize("geom", GEOMS)
def test_fwd_vs_fp32(operands, geom):
    from distributed_rl_amd import ops

    x, w, b, r = operands[geom]
    for name, kw in [("plain", {}),
                     ("relu_in+relu_out", dict(relu_in=True, relu_out=True)),
                     ("residual", dict(residual=r))]:
        out = ops.fused_conv3x3(x, w, b, **kw)
        ref = _ref(x, w, b, **kw)
        assert out.shape == ref.shape and out.dtype == torch.bfloat16
        assert out.is_contiguous(memory_format=torch.channels_last)
        err = (out.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{geom} {name}: max err {err:.4g} / max ref {scale:.4g} "
              f"= {err / scale:.3g}")
        assert err / scale < 2e-2, f"{geom} {name}: {err} vs {scale}"


@pytest.mark.parametrize("geom", GEOMS)
def test_exact_border_count(ext, geom):
    """All-ones input and weights: out = C x (in-bounds taps), exactly."""
    from distributed_rl_amd import ops

    H, W, C, COUT = geom
    x = _cl(torch.ones(N, C, H, W, device=DEV))
    w = _cl(torch.ones(COUT, C, 3, 3, device=DEV))
    out = ops.fused_conv3x3(x, w, None)
    th = torch.full((H,), 3.0, device=DEV)
    th[0] = th[-1] = 2.0
    tw = torch.full((W,), 3.0, device=DEV)
    tw[0] = tw[-1] = 2.0
    expect = (C * th[:, None] * tw[None, :]).expand(N, COUT, H, W)
    assert expect[0, 0, 0, 0] == 4 * C and expect[0, 0, 0, 1] == 6 * C \
        and expect[0, 0, 1, 1] == 9 * C
    assert torch.equal(out.float(), expect)


@pytest.mark.parametrize("geom", GEOMS)
def test_no_halo_reads(operands, geom):
    """x sits between two NaN images of one allocation: a tap read across
    an image border would pull a NaN into the output."""
    from distributed_rl_amd import ops

    x, w, b, _ = operands[geom]
    big = torch.full((N + 2, *x.shape[1:]), float("nan"), device=DEV,
                     dtype=torch.bfloat16).contiguous(
                         memory_format=torch.channels_last)
    big[1:-1] = x
    xs = big[1:-1]
    assert xs.is_contiguous(memory_format=torch.channels_last)
    assert xs.data_ptr() != big.data_ptr()
    out = ops.fused_conv3x3(xs, w, b)
    plain = ops.fused_conv3x3(x.clone(memory_format=torch.channels_last), w, b)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, plain)


@pytest.mark.parametrize("geom", GEOMS)
def test_flag_identities(operands, geom):
    from distributed_rl_amd import ops

    x, w, b, r = operands[geom]
    a = ops.fused_conv3x3(x, w, b, relu_in=True)
    a2 = ops.fused_conv3x3(torch.relu(x), w, b)
    assert torch.equal(a, a2)
    o = ops.fused_conv3x3(x, w, b)
    assert torch.equal(ops.fused_conv3x3(x, w, b, relu_out=True),
                       torch.relu(o))
    z = ops.fused_conv3x3(x, torch.zeros_like(w), torch.zeros_like(b),
                          residual=r)
    assert torch.equal(z, r)


@pytest.mark.parametrize("shape", [(11, 11, 32, 4), (42, 42, 16, 3)])
def test_block_backward_matches_eager(ext, shape):
    """Residual block as two fused convs vs fp32 eager autograd, with the
    criteria of test_gpu_conv.test_conv_backward_matches_eager."""
    from distributed_rl_amd import ops

    H, W, C, n = shape
    torch.manual_seed(7)
    x = _cl(torch.randn(n, C, H, W, device=DEV))
    w1, w2 = (_cl(torch.randn(C, C, 3, 3, device=DEV) * 0.05)
              for _ in range(2))
    b1, b2 = ((torch.randn(C, device=DEV) * 0.1).to(torch.bfloat16)
              for _ in range(2))
    g = _cl(torch.randn(n, C, H, W, device=DEV))

    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xl, w1l, b1l, w2l, b2l = leaves
    y = ops.fused_conv3x3(xl, w1l, b1l, relu_in=True, relu_out=True)
    out = ops.fused_conv3x3(y, w2l, b2l, residual=xl)
    mine = torch.autograd.grad(out, leaves, g)

    fl = [t.float().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xf, w1f, b1f, w2f, b2f = fl
    yf = F.conv2d(F.relu(xf), w1f, b1f, padding=1)
    of = xf + F.conv2d(F.relu(yf), w2f, b2f, padding=1)
    theirs = torch.autograd.grad(of, fl, g.float())

    fwd_err = (out.float() - of).abs().max().item() / of.abs().max().item()
    print(f"{shape}: block fwd rel err {fwd_err:.3g}")
    for m, t, name in zip(mine, theirs, ["gx", "gw1", "gb1", "gw2", "gb2"]):
        m, t = m.float(), t.float()
        scale = t.abs().max().item() + 1e-6
        mae = (m - t).abs().mean().item()
        frac_big = ((m - t).abs() > 0.1 * scale).float().mean().item()
        print(f"{shape} {name}: mae/scale {mae / scale:.3g} "
              f"frac_big {frac_big:.3g}")
        assert mae / scale < 5e-3, f"{name}: mae {mae} scale {scale}"
        assert frac_big < 0.01, f"{name}: {frac_big:.3%} entries off"


def _resnet_agent():
    from distributed_rl_amd.config import load_config
    from distributed_rl_amd.models import BaseAgent

    torch.manual_seed(5)
    ref = BaseAgent(load_config("impala_resnet").model_info).to(DEV)
    net = copy.deepcopy(ref).to(memory_format=torch.channels_last).to(
        torch.bfloat16)
    return ref, net


def _count_fused(monkeypatch):
    from distributed_rl_amd import ops

    calls = []
    real = ops.fused_conv3x3

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "fused_conv3x3", counting)
    return calls


def test_model_fused_path(ext, monkeypatch):
    """Forced on, the torso runs 14 of its 15 convs on the own kernel and
    lands as close to the fp32 model as the library bf16 path does (both
    round to bf16 after every layer; only accumulation order differs)."""
    ref, net = _resnet_agent()
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV))
    calls = _count_fused(monkeypatch)
    with torch.no_grad():
        y_ref = ref([x.float()])[0]
        monkeypatch.setenv("DRL_OWN_RESCONV", "1")
        y_fused = net([x])[0]
        n_fused = len(calls)
        monkeypatch.setenv("DRL_OWN_RESCONV", "0")
        y_lib = net([x])[0]
    assert n_fused == 14, f"fused path ran {n_fused} convs"
    assert len(calls) == n_fused, "DRL_OWN_RESCONV=0 must not use the kernel"
    err_fused = (y_fused.float() - y_ref).abs().max().item()
    err_lib = (y_lib.float() - y_ref).abs().max().item()
    print(f"model: fused err {err_fused:.4g}, library bf16 err {err_lib:.4g}")
    assert err_fused <= 2 * err_lib


def test_model_graph_capture(ext, monkeypatch):
    """One forward+backward of the forced-on model captured in a graph
    replays to identical outputs."""
    monkeypatch.setenv("DRL_OWN_RESCONV", "1")
    _, net = _resnet_agent()
    calls = _count_fused(monkeypatch)
    x = _cl(torch.rand(2, 4, 84, 84, device=DEV))
    params = list(net.parameters())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(net([x])[0].float().square().sum(), params)
    torch.cuda.current_stream().wait_stream(side)
    assert len(calls) == 28

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = net([x])[0]
        grads = torch.autograd.grad(y.float().square().sum(), params)
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append(y.clone())
    assert torch.isfinite(seen[0].float()).all()
    assert seen[0].abs().max() > 0
    assert torch.equal(seen[0], seen[1])
    # the gradients come from the library's weight-/input-gradient kernels,
    # whose atomic sums may differ in the last bit between replays
    for g in grads:
        assert torch.isfinite(g.float()).all()
