"""CPU checks of the exact-grid cases (tests/resconv_hw_cases.py) that the
run-time H, W conv tests feed to the HIP kernels: the two bounds that make
every fp32 partial sum exact, from the inputs alone, and an fp32 evaluation
of the reference in two summation orders against float64."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resconv_hw_cases as RC  # noqa: E402

PAIRS = RC.FWD_PAIRS + [RC.STEM]


def _is_grid(t, step, bound):
    return bool(((t / step) == (t / step).round()).all()) and \
        t.abs().max().item() <= bound


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_inputs_on_the_grid_and_bounds(shape):
    H, W, N = shape
    for C, COUT in PAIRS:
        d = RC.make_case(H, W, N, C, COUT)
        for k in ("x", "g", "r"):
            assert _is_grid(d[k], 0.25, 2.0), k
            assert torch.equal(d[k].to(torch.bfloat16).double(), d[k])
        for k in ("w", "b"):
            assert _is_grid(d[k], 0.125, 1.0), k
            assert torch.equal(d[k].to(torch.bfloat16).double(), d[k])
        # forward / input gradient: units of 1/32, K <= 288 terms of <= 2,
        # plus bias and residual
        K = 9 * max(C, COUT)
        assert K <= 288
        assert (2.0 * 1.0 * K + 1.0 + 2.0) * 32 < 2 ** 24
        # weight gradient: units of 1/16, M terms of <= 4
        M = N * H * W
        assert M <= 2 ** 17 and 4.0 * M * 16 < 2 ** 24
        for k in ("out", "out_rr", "gx", "gx_masked"):
            assert _is_grid(d[k], 1 / 32, 2.0 * K + 3.0), k
        for k in ("gw", "gw_relu", "gb"):
            assert _is_grid(d[k], 1 / 16, 4.0 * M), k


def test_wrw_batches_meet_the_rules():
    """Every weight-gradient batch runs at least two m-blocks of at least
    two passes; ragged at the 32-row chunk wherever H*W allows."""
    rows_of = dict(RC.WRW_ROWS)
    rows_of[RC.STEM] = RC.STEM_WRW_ROWS
    for H, W, _ in RC.SHAPES:
        for pair, rows in rows_of.items():
            N = RC.wrw_batch(H, W, rows)
            M = N * H * W
            n_pass = (M + rows - 1) // rows
            mb = (n_pass + 7) // 8
            assert mb >= 2 and n_pass >= 2 * mb, (H, W, pair, N)
            assert M <= 2 ** 17
            if (H * W) % 32:
                assert M % 32 and M % rows, (H, W, pair, N)
    assert RC.wrw_batch(5, 7, 128) * 35 % 128


@pytest.mark.parametrize("shape", [(1, 9, 3), (5, 7, 9), (9, 12, 3)],
                         ids=["1x9", "5x7", "9x12"])
def test_fp32_in_two_orders_equals_fp64(shape):
    H, W, N = shape
    for C, COUT in PAIRS:
        d = RC.make_case(H, W, N, C, COUT)
        x, w, b, r = (d[k].float() for k in ("x", "w", "b", "r"))
        a = F.conv2d(x, w, b, padding=1) + r
        # the other order: tap by tap, last tap first, channels reversed
        xp = F.pad(x, (1, 1, 1, 1))
        acc = torch.zeros_like(a)
        for kh in (2, 1, 0):
            for kw in (2, 1, 0):
                win = xp[:, :, kh:kh + H, kw:kw + W].flip(1)
                acc += torch.einsum("nchw,oc->nohw", win,
                                    w[:, :, kh, kw].flip(1))
        acc = acc + r + b[None, :, None, None]
        assert torch.equal(a.double(), d["out"])
        assert torch.equal(acc.double(), d["out"])
        # weight gradient: fp32 row sums forwards and backwards
        g = d["g"].float()
        cols = F.unfold(x, 3, padding=1)                  # (N, C*9, HW)
        cols = cols.view(N, C, 9, H * W).permute(0, 3, 2, 1).reshape(
            N * H * W, 9 * C)                             # (M, (kh,kw,c))
        gm = g.permute(0, 2, 3, 1).reshape(N * H * W, COUT)
        gw_a = gm.t() @ cols
        gw_b = gm.flip(0).t() @ cols.flip(0)
        assert torch.equal(gw_a.double(), d["gw"])
        assert torch.equal(gw_b.double(), d["gw"])
