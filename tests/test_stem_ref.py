"""The stem-conv op and the model gate off the GPU: CPU tensors take the
eager reference, and DRL_OWN_STEM never applies to a CPU model."""

import torch
import torch.nn.functional as F


def test_op_on_cpu_is_conv2d():
    from distributed_rl_amd import ops

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 84, 84, generator=gen)
    w = torch.randn(16, 4, 3, 3, generator=gen) * 0.1
    b = torch.randn(16, generator=gen)
    assert torch.equal(ops.fused_stem_conv3x3(x, w, b),
                       F.conv2d(x, w, b, padding=1))
    assert torch.equal(ops.fused_stem_conv3x3(x, w, None),
                       F.conv2d(x, w, None, padding=1))
    # any geometry: the reference has no table
    x2 = torch.randn(1, 3, 7, 5, generator=gen)
    w2 = torch.randn(5, 3, 3, 3, generator=gen)
    assert torch.equal(ops.fused_stem_conv3x3(x2, w2, None),
                       F.conv2d(x2, w2, None, padding=1))


def test_cpu_model_ignores_the_gate(monkeypatch):
    from distributed_rl_amd import ops
    from distributed_rl_amd.models.base_agent import ImpalaResNet

    torch.manual_seed(5)
    net = ImpalaResNet({"iSize": 4, "channels": [16, 32, 32], "nBlocks": 2})
    x = torch.rand(2, 4, 84, 84)
    calls = []
    real = ops.fused_stem_conv3x3
    monkeypatch.setattr(ops, "fused_stem_conv3x3",
                        lambda *a: calls.append(1) or real(*a))
    with torch.no_grad():
        monkeypatch.delenv("DRL_OWN_STEM", raising=False)
        y_unset = net(x)
        monkeypatch.setenv("DRL_OWN_STEM", "1")
        y_on = net(x)
        y_on_bf16 = net.to(torch.bfloat16)(x.to(torch.bfloat16))
    assert torch.equal(y_on, y_unset)
    assert y_on_bf16.dtype == torch.bfloat16
    assert not calls
