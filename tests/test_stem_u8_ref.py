"""CPU side of the uint8 stem conv (K2e): the dequantisation table, the
exactness bounds the GPU tests rest on, and the eager reference itself."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_u8_cases as SC  # noqa: E402

from distributed_rl_amd import ops  # noqa: E402
from distributed_rl_amd.ops import torch_ref  # noqa: E402


def test_dequant_table():
    """All 256 values: multiples of 2^-15, at most 1, and the fp32 product
    with 1/255 rounds to the same bf16 as the division."""
    u8 = torch.arange(256, dtype=torch.uint8)
    x = (u8.float() / 255).bfloat16()
    assert torch.equal(x, (u8.float() * (1.0 / 255.0)).bfloat16())
    scaled = x.double() * 2 ** 15
    assert torch.equal(scaled, scaled.round()) and x.max() == 1 and x[0] == 0


@pytest.mark.parametrize("shape", SC.SHAPES, ids=SC.IDS)
def test_forward_sums_are_exact_in_fp32(shape):
    d = SC.case(shape)
    bound = torch_ref.stem_conv3x3_u8(d["frames"], d["w"].abs(), d["b"].abs())
    assert bound.max().item() <= 37
    f32 = torch_ref.stem_conv3x3_u8(d["frames"], d["w"].float(),
                                    d["b"].float())
    assert torch.equal(f32.double(), d["out"])
    assert torch.equal(ops.fused_stem_conv3x3_u8(d["frames"], d["w"], d["b"]),
                       d["out"])


@pytest.mark.parametrize("shape,regime", SC.WRW_CASES, ids=SC.WRW_IDS)
def test_gradient_sums_are_exact_in_fp32(shape, regime):
    d = SC.case(shape, regime)
    bound_gw, bound_gb = torch_ref.stem_conv3x3_u8_grads(d["frames"],
                                                         d["g"].abs())
    assert bound_gw.max().item() * SC.GRID[regime] < 2 ** 24
    assert bound_gb.max().item() * 4 < 2 ** 24
    # the reference against the sum written out
    x = (d["frames"].float() / 255).bfloat16().double()
    cols = F.unfold(x, 3, padding=1)                     # (N, C*9, HW)
    gm = d["g"].reshape(shape[0], SC.COUT, -1)
    gw = torch.einsum("nol,nkl->ok", gm, cols).view(SC.COUT, SC.C, 9)
    assert torch.equal(gw.permute(0, 2, 1).reshape(SC.COUT, 36), d["gw"])
    assert torch.equal(gm.sum((0, 2)), d["gb"])
