"""CPU side of the fused 3x3 pad-1 conv (ops.fused_conv3x3): the op's eager
dispatch and the IMPALA-ResNet torso's unchanged CPU path."""

import pytest
import torch
import torch.nn.functional as F

from distributed_rl_amd import ops
from distributed_rl_amd.models.base_agent import ImpalaResNet

# the flag combinations the model uses: section-entry conv, block c1, block c2
FLAG_SETS = [
    dict(relu_in=False, relu_out=False, residual=False),
    dict(relu_in=True, relu_out=True, residual=False),
    dict(relu_in=False, relu_out=False, residual=True),
    dict(relu_in=True, relu_out=False, residual=True),
]


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_fused_conv3x3_cpu_equals_composition(flags):
    torch.manual_seed(0)
    N, C, COUT, H, W = 2, 16, 16, 7, 5
    x = torch.randn(N, C, H, W)
    w = torch.randn(COUT, C, 3, 3) * 0.1
    b = torch.randn(COUT) * 0.1
    r = torch.randn(N, COUT, H, W) if flags["residual"] else None
    out = ops.fused_conv3x3(x, w, b, relu_in=flags["relu_in"],
                            relu_out=flags["relu_out"], residual=r)
    ref = F.conv2d(F.relu(x) if flags["relu_in"] else x, w, b, padding=1)
    if r is not None:
        ref = ref + r
    if flags["relu_out"]:
        ref = F.relu(ref)
    assert out.dtype == torch.float32
    assert torch.equal(out, ref)


def test_fused_conv3x3_cpu_no_bias_and_grad():
    torch.manual_seed(1)
    x = torch.randn(1, 8, 5, 5, requires_grad=True)
    w = torch.randn(8, 8, 3, 3, requires_grad=True)
    out = ops.fused_conv3x3(x, w, None, relu_in=True, residual=x)
    ref = F.conv2d(F.relu(x), w, None, padding=1) + x
    assert torch.equal(out, ref)
    out.sum().backward()
    assert x.grad is not None and w.grad is not None


@pytest.mark.parametrize("gate", [None, "0", "1"])
def test_impala_resnet_cpu_path_unchanged(monkeypatch, gate):
    """CPU input never takes the fused path, whatever DRL_OWN_RESCONV says."""
    if gate is None:
        monkeypatch.delenv("DRL_OWN_RESCONV", raising=False)
    else:
        monkeypatch.setenv("DRL_OWN_RESCONV", gate)
    torch.manual_seed(2)
    net = ImpalaResNet({"iSize": 4, "channels": [16, 32, 32], "nBlocks": 2})
    x = torch.rand(2, 4, 84, 84)
    with torch.no_grad():
        y = net(x)
        ref = torch.flatten(torch.relu(net.body(x)), 1)
    assert y.shape == (2, 32 * 11 * 11)
    assert torch.equal(y, ref)
