"""torch_ref.wrw_fold_ordered, the bit-exact reference of the ordered
weight-gradient fold (tests/test_gpu_wrw_fold.py), held on the CPU to an fp64
sum and to hand-worked cases that pin its summation order."""

import pytest
import torch

from distributed_rl_amd.ops import torch_ref

U = 2.0 ** -24  # fp32 unit roundoff


@pytest.mark.parametrize("planes", [1, 15, 16, 17, 63, 64, 65, 128])
@pytest.mark.parametrize("cout", [16, 64])
def test_fold_ref_close_to_fp64(planes, cout):
    g = torch.Generator().manual_seed(planes * 100 + cout)
    n_elem = 128
    part = torch.randn(planes, n_elem + 64, generator=g)
    b_part = torch.randn(planes, cout, generator=g)
    gw, gb = torch_ref.wrw_fold_ordered(part, n_elem, b_part)
    # every partial sum is bounded by sum|x|, and a value passes through at
    # most `adds` rounded additions: error <= adds * U * sum|x| (first order;
    # the factor 1.01 covers the higher-order terms at these sizes)
    p64 = part[:, :n_elem].double()
    adds = (planes + 15) // 16 + 16
    bound = 1.01 * adds * U * p64.abs().sum(0)
    assert ((gw.double() - p64.sum(0)).abs() <= bound).all()
    b64 = b_part.double()
    G = 256 // cout
    adds_b = (planes + G - 1) // G + G + 1
    bound_b = 1.01 * adds_b * U * b64.abs().sum(0)
    assert ((gb.double() - b64.sum(0)).abs() <= bound_b).all()
    assert gw.dtype == torch.float32 and gb.dtype == torch.float32
    assert gw.shape == (n_elem,) and gb.shape == (cout,)


def test_fold_ref_exact_on_integers():
    g = torch.Generator().manual_seed(1)
    part = torch.randint(-1000, 1000, (65, 64 + 64), generator=g).float()
    b_part = torch.randint(-1000, 1000, (256, 32), generator=g).float()
    gw, gb = torch_ref.wrw_fold_ordered(part, 64, b_part)
    assert torch.equal(gw, part[:, :64].sum(0))
    assert torch.equal(gb, b_part.sum(0))


def test_fold_ref_ignores_plane_padding():
    g = torch.Generator().manual_seed(2)
    part = torch.randn(17, 64 + 64, generator=g)
    a, _ = torch_ref.wrw_fold_ordered(part, 64)
    part[:, 64:] = float("nan")
    b, none = torch_ref.wrw_fold_ordered(part, 64)
    assert none is None and torch.equal(a, b)


def test_fold_ref_order_of_plane_groups():
    """Planes 0 and 16 share group 0, planes 1 and 17 group 1: 2^24 + 1
    rounds back to 2^24 inside group 0, the two ones of group 1 first make
    2, and 2^24 + 2 is exact. Plane order would lose all three ones."""
    part = torch.zeros(18, 64 + 64)
    part[0, 0] = 2.0 ** 24
    part[16, 0] = 1.0
    part[1, 0] = 1.0
    part[17, 0] = 1.0
    gw, _ = torch_ref.wrw_fold_ordered(part, 64)
    assert gw[0].item() == 2.0 ** 24 + 2.0
    seq = torch.zeros(())
    for k in range(18):
        seq = seq + part[k, 0]
    assert seq.item() == 2.0 ** 24
    assert torch.equal(gw[1:], torch.zeros(63))


def test_fold_ref_order_of_bias_groups():
    """cout 64: G = 4 groups; rows 0 and 4 share group 0, rows 1 and 5
    group 1 — the same construction as above."""
    b_part = torch.zeros(8, 64)
    b_part[0, 3] = 2.0 ** 24
    b_part[4, 3] = 1.0
    b_part[1, 3] = 1.0
    b_part[5, 3] = 1.0
    _, gb = torch_ref.wrw_fold_ordered(torch.zeros(1, 128), 64, b_part)
    assert gb[3].item() == 2.0 ** 24 + 2.0


def test_fold_ref_rounds_once_at_the_end():
    # 1 + 2^-9 + 2^-9 = 1 + 2^-8 is a tie between the bf16 neighbours 1 and
    # 1 + 2^-7: round-to-nearest-even gives 1. Rounding each plane to bf16
    # first would also give 1; rounding after only the first add (1 + 2^-9
    # -> 1) too; so use 1 + 2^-7 + 2^-9 + 2^-9 = 1 + 2^-7 + 2^-8, a tie that
    # goes up to the even 1 + 2^-6 only if both small terms survive in fp32
    part = torch.zeros(3, 128)
    part[0, 0] = 1.0 + 2.0 ** -7
    part[1, 0] = 2.0 ** -9
    part[2, 0] = 2.0 ** -9
    gw, _ = torch_ref.wrw_fold_ordered(part, 64, out_dtype=torch.bfloat16)
    assert gw.dtype == torch.bfloat16
    assert gw[0].float().item() == 1.0 + 2.0 ** -6
