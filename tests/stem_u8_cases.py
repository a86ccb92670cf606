"""Shapes and inputs of the uint8 stem conv tests (K2e).

Weights, biases and gout are multiples of 1/4 in [-1, 1]; a dequantised
frame value is a multiple of 2^-15 and at most 1. Forward: every product is a
multiple of 2^-17 and |sum| <= 37, so fp32 sums are exact in any order.
Weight/bias gradient: exact while sum_m |g||x| / grid < 2^24, grid being the
product grid of the regime: 2^-17 for frames over 0..255 (regime "full", used
where N*H*W <= 128), 2^-2 for frames over {0, 255} (regime "binary", every
shape). test_stem_u8_ref.py asserts that bound from the data."""

import functools

import torch

C, COUT = 4, 16

# (N, H, W). (2, 13, 12): the kernels' plan at this width is 12 band rows in
# the forward and 6 in the weight gradient (ext.conv3x3c4_u8_plan, checked in
# test_rejections), so H = 13 leaves a last band of one row in both.
SHAPES = [(3, 1, 1), (3, 1, 9), (3, 9, 1), (2, 2, 2), (2, 5, 7), (2, 7, 5),
          (2, 3, 40), (2, 13, 12), (3, 36, 48), (2, 84, 84)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
WRW_CASES = [(s, r) for s in SHAPES for r in ("full", "binary")
             if r == "binary" or s[0] * s[1] * s[2] <= 128]
WRW_IDS = ["x".join(map(str, s)) + "-" + r for s, r in WRW_CASES]
GRID = {"full": 2.0 ** 17, "binary": 4.0}


def _quarters(shape, gen):
    return torch.randint(-4, 5, shape, generator=gen).double() / 4


@functools.lru_cache(maxsize=None)
def case(shape, regime="full"):
    """Inputs and fp64 references of one case, computed once and shared."""
    from distributed_rl_amd.ops import torch_ref

    N, H, W = shape
    gen = torch.Generator().manual_seed(10000 * N + 100 * H + W)
    frames = torch.randint(0, 256, (N, C, H, W), generator=gen,
                           dtype=torch.uint8)
    if regime == "binary":
        frames = (frames >> 7) * 255
    d = dict(frames=frames, w=_quarters((COUT, C, 3, 3), gen),
             b=_quarters((COUT,), gen), g=_quarters((N, COUT, H, W), gen))
    d["out"] = torch_ref.stem_conv3x3_u8(frames, d["w"], d["b"])
    d["gw"], d["gb"] = torch_ref.stem_conv3x3_u8_grads(frames, d["g"])
    return d
