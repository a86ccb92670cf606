"""conv_wrw is conv_wrw_partials plus a one-job wrw_fold_grouped: the
partial planes and column-sum partials the first returns, folded on the CPU
by torch_ref.wrw_fold_ordered, must give conv_wrw's gw and gb bit for bit,
for fp32 workspaces and bf16 gradients, at all seven wrw geometries. gw
itself is held by the aten comparisons of tests/test_gpu_conv.py."""

import pytest
import torch

from distributed_rl_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (H, W, C, KH, KW, S, COUT, u8): the seven wrw geometries of kConvs
GEOMS = [
    (84, 84, 4, 8, 8, 4, 32, True),
    (84, 84, 4, 8, 8, 4, 32, False),
    (20, 20, 32, 4, 4, 2, 64, False),
    (9, 9, 64, 3, 3, 1, 64, False),
    (84, 84, 4, 8, 8, 4, 16, True),
    (84, 84, 4, 8, 8, 4, 16, False),
    (20, 20, 16, 4, 4, 2, 32, False),
]
# N = 1: fewer chunks than m-slices; N = 37: ragged last chunk, more than one
# chunk per block for conv1
BATCHES = [1, 37]


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _inputs(geom, N):
    H, W, C, KH, KW, S, COUT, u8 = geom
    P, Q = (H - KH) // S + 1, (W - KW) // S + 1
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 + N + COUT)
    if u8:
        x = torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8, device=DEV,
                          generator=g)
    else:
        x = torch.randn(N, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
    x = x.to(memory_format=torch.channels_last)
    gout = torch.randn(N, COUT, P, Q, device=DEV, generator=g).to(
        torch.bfloat16).to(memory_format=torch.channels_last)
    return x, gout


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N", BATCHES)
@pytest.mark.parametrize("geom", GEOMS,
                         ids=lambda g: f"{g[0]}x{g[2]}-{g[6]}"
                                       f"{'-u8' if g[7] else ''}")
def test_conv_wrw_is_partials_plus_ordered_fold(ext, geom, N, with_bias):
    H, W, C, KH, KW, S, COUT, _ = geom
    n_elem = COUT * KH * KW * C
    x, gout = _inputs(geom, N)
    part, mb, b_part = ext.conv_wrw_partials(x, gout, S, with_bias)
    assert part.shape == (mb, n_elem + ext.wrw_plane_pad())
    assert b_part.shape == ((256, COUT) if with_bias else (0,))
    for dtype in (torch.bfloat16, torch.float32):
        gw = torch.full((COUT, KH * KW * C), float("nan"), dtype=dtype,
                        device=DEV)
        gb = (torch.full((COUT,), float("nan"), dtype=dtype, device=DEV)
              if with_bias else torch.empty(0, device=DEV))
        ext.conv_wrw(x, gout, gw, gb, S)
        torch.cuda.synchronize()
        ref_w, ref_b = torch_ref.wrw_fold_ordered(
            part, n_elem, b_part if with_bias else None, dtype)
        assert torch.equal(gw.cpu().reshape(-1), ref_w)
        if with_bias:
            assert torch.equal(gb.cpu(), ref_b)
    if with_bias:
        # independent anchor for gb, test_conv_wrw_vs_aten's tolerance
        ref = gout.double().sum(dim=(0, 2, 3))
        assert torch.allclose(gb.double(), ref, rtol=2e-2, atol=2e-2)


def test_wrw_partials_rejects_before_launch(ext):
    x, gout = _inputs(GEOMS[3], 3)
    with pytest.raises(RuntimeError):  # gout of another batch
        ext.conv_wrw_partials(x, gout[:2].contiguous(
            memory_format=torch.channels_last), 1, True)
    with pytest.raises(RuntimeError):  # not channels_last
        ext.conv_wrw_partials(x.contiguous(), gout, 1, True)
    torch.cuda.synchronize()
