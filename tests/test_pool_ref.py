"""CPU oracles of the 3x3 stride-2 pad-1 max-pool (ops/torch_ref.py
maxpool3x3s2, maxpool3x3s2_taps, maxpool3x3s2_bwd) against F.max_pool2d and
its float64 autograd, the selection rule the HIP kernel implements, and the
CPU paths of ops.fused_maxpool3x3s2 and ImpalaResNet."""

import pytest
import torch
import torch.nn.functional as F

from distributed_rl_amd import ops
from distributed_rl_amd.ops import torch_ref

BF16 = torch.bfloat16

# (N, H, W, C): the shapes of tests/test_gpu_pool.py
SHAPES = [(1, 84, 84, 16), (2, 21, 21, 32), (3, 6, 5, 16), (2, 2, 3, 16),
          (1, 1, 1, 16)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
KINDS = ["randn", "ties", "special"]


def make_x(shape, kind, seed=3):
    """bf16 channels_last (N, C, H, W) input of one of the three kinds."""
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(seed + 7 * KINDS.index(kind))
    if kind == "randn":
        x = torch.randn(N, C, H, W, generator=gen)
    elif kind == "ties":
        x = torch.randint(-1, 2, (N, C, H, W), generator=gen).float()
    else:
        x = torch.randn(N, C, H, W, generator=gen)
        r = torch.rand(N, C, H, W, generator=gen)
        x[r < 0.10] = float("nan")
        x[(r >= 0.10) & (r < 0.15)] = float("inf")
        x[(r >= 0.15) & (r < 0.25)] = float("-inf")
        x[(r >= 0.25) & (r < 0.40)] = -0.0
        x[(r >= 0.40) & (r < 0.50)] = 0.0
    x = x.to(BF16).contiguous(memory_format=torch.channels_last)
    # one NaN pattern going in, the canonical quiet one
    x.view(torch.int16)[x.isnan()] = 0x7FC0
    return x


def rule_forward(x):
    """The kernel's selection rule, tap by tap: the first in-bounds tap
    initialises, a later one replaces iff v > m or v is NaN."""
    N, C, H, W = x.shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xf = x.float()
    m = torch.zeros(N, C, P, Q)
    tap = torch.zeros(N, C, P, Q, dtype=torch.uint8)
    have = torch.zeros(P, Q, dtype=torch.bool)
    p = torch.arange(P).view(P, 1)
    q = torch.arange(Q).view(1, Q)
    for kh in range(3):
        for kw in range(3):
            h, w = 2 * p - 1 + kh, 2 * q - 1 + kw
            live = (h >= 0) & (h < H) & (w >= 0) & (w < W)
            v = xf[:, :, h.clamp(0, H - 1), w.clamp(0, W - 1)]
            take = live & (~have | (v > m) | v.isnan())
            m = torch.where(take, v, m)
            tap = torch.where(take, torch.tensor(kh * 3 + kw,
                                                 dtype=torch.uint8), tap)
            have = have | live
    return m.to(x.dtype), tap


def bits(t):
    """t's bf16 bit patterns as int16, every NaN as 0x7FC0. Which NaN
    pattern the CPU library returns is a property of its copy loops, not of
    the pool: it round-trips bf16 through float and writes 0x7FC0 from its
    scalar loop and 0xFFFF from its vector loop for the same NaN input. All
    other values, -0 and the infinities included, compare bit for bit."""
    t = t.cpu()
    b = t.view(torch.int16).clone()
    b[t.isnan()] = 0x7FC0
    return b.contiguous()


def picked_bits(x, taps):
    """Raw int16 bits of x at the pixel each tap names (checked in bounds)."""
    N, C, H, W = x.shape
    P, Q = taps.shape[2:]
    h = 2 * torch.arange(P).view(P, 1) - 1 + (taps // 3).long()
    w = 2 * torch.arange(Q).view(1, Q) - 1 + (taps % 3).long()
    assert (h >= 0).all() and (h < H).all()
    assert (w >= 0).all() and (w < W).all()
    # gathered as int16: CPU bf16 copies may rewrite a NaN's payload
    return x.view(torch.int16).reshape(N, C, H * W).gather(
        2, (h * W + w).reshape(N, C, P * Q)).reshape(N, C, P, Q)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_taps(shape, kind):
    x = make_x(shape, kind)
    want = F.max_pool2d(x, 3, 2, 1)
    assert same_bits(torch_ref.maxpool3x3s2(x), want)
    out, taps = torch_ref.maxpool3x3s2_taps(x)
    assert same_bits(out, want)
    assert taps.dtype == torch.uint8 and taps.shape == want.shape
    assert int(taps.max()) <= 8
    # the tap names an in-bounds pixel that holds the output's bits
    picked = picked_bits(x, taps)
    assert torch.equal(picked, bits(want))
    # and the stated selection rule gives the library's values and taps
    r_out, r_taps = rule_forward(x)
    assert same_bits(r_out, want)
    assert torch.equal(r_taps, taps)


@pytest.mark.parametrize("kind", ["randn", "ties"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_matches_fp64_autograd(shape, kind):
    x = make_x(shape, kind)
    N, C, H, W = x.shape
    _, taps = torch_ref.maxpool3x3s2_taps(x)
    gen = torch.Generator().manual_seed(17)
    gout = torch.randn(taps.shape, generator=gen).to(BF16)
    gx = torch_ref.maxpool3x3s2_bwd(gout, taps, H, W)
    assert gx.dtype == torch.float32 and gx.shape == x.shape

    xd = x.double().requires_grad_(True)
    y = F.max_pool2d(xd, 3, 2, 1)
    (ref,) = torch.autograd.grad(y, xd, gout.double(), retain_graph=True)
    (S,) = torch.autograd.grad(y, xd, gout.double().abs())
    # fp32 sums of at most four bf16 terms
    assert ((gx.double() - ref).abs() <= 2.0 ** -22 * S).all()
    # and after the single rounding to bf16, the bound of the GPU test
    assert ((gx.to(BF16).double() - ref).abs() <= 2.0 ** -8 * S).all()


def test_fused_op_on_cpu_is_the_library():
    x = make_x((2, 21, 21, 32), "randn")
    assert same_bits(ops.fused_maxpool3x3s2(x), F.max_pool2d(x, 3, 2, 1))
    xf = x.float().requires_grad_(True)
    y = ops.fused_maxpool3x3s2(xf)
    (g,) = torch.autograd.grad(y.sum(), xf)
    xr = x.float().requires_grad_(True)
    (gr,) = torch.autograd.grad(F.max_pool2d(xr, 3, 2, 1).sum(), xr)
    assert torch.equal(g, gr)


@pytest.mark.parametrize("gate", [None, "0", "1"])
def test_cpu_model_unchanged(monkeypatch, gate):
    """A CPU ImpalaResNet is nn.Sequential over its body, whatever
    DRL_OWN_POOL says."""
    from distributed_rl_amd.models.base_agent import ImpalaResNet

    if gate is None:
        monkeypatch.delenv("DRL_OWN_POOL", raising=False)
    else:
        monkeypatch.setenv("DRL_OWN_POOL", gate)
    calls = []
    real = ops.fused_maxpool3x3s2
    monkeypatch.setattr(ops, "fused_maxpool3x3s2",
                        lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(2)
    net = ImpalaResNet({"iSize": 4, "channels": [16, 32, 32], "nBlocks": 2})
    x = torch.rand(2, 4, 84, 84)
    with torch.no_grad():
        want = torch.flatten(torch.relu(net.body(x)), 1)
        assert torch.equal(net(x), want)
        xb = x.to(BF16)
        netb = net.to(BF16)
        want_b = torch.flatten(torch.relu(netb.body(xb)), 1)
        assert torch.equal(netb(xb), want_b)
    assert not calls
