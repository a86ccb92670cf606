"""Shared inputs of the run-time H, W conv tests (test_resconv_hw_ref.py on
the CPU, test_gpu_resconv_hw.py and test_gpu_stem_hw.py on the GPU).

Exact-grid inputs: x, gout and the residual are multiples of 1/4 in [-2, 2],
weights and bias multiples of 1/8 in [-1, 1] — all exact in bf16. Then
  * a forward or input-gradient dot over K <= 288 is a sum of multiples of
    1/32 bounded by 2 * 1 * 288 = 576 (+ bias 1 + residual 2): < 2^15 units;
  * a weight-gradient element over M <= 2^17 rows is a sum of multiples of
    1/16 bounded by 2 * 2 * M: <= 2^23 units.
Both stay below 2^24 units, so every fp32 partial sum is exact in any order
and the kernels must reproduce the float64 reference bit for bit.
"""

import torch

# (H, W, N): the smallest shapes at which the run-time row decode, bounds
# tests and tap offset can go wrong (one forward block is 256 rows)
SHAPES = [
    (1, 1, 5),     # only the centre tap is live; less than one fragment
    (1, 9, 3),     # every dy tap dead
    (9, 1, 3),     # every dx tap dead; H and W not interchangeable
    (2, 2, 70),    # every pixel a corner; ragged second block
    (5, 7, 9),     # non-square; 35 rows per image against 32 per wave
    (7, 5, 9),
    (3, 40, 3),    # W > 32: a whole fragment inside one image row
    (32, 32, 2),   # M an exact multiple of 256, no tail
    (36, 48, 1),   # DMLab 72x96 sections
    (9, 12, 3),
]
SHAPE_IDS = [f"{h}x{w}n{n}" for h, w, n in SHAPES]

FWD_PAIRS = [(16, 16), (16, 32), (32, 32), (32, 16)]  # (C, COUT)
# (C, COUT) -> rows per weight-gradient pass (32 * WRW_R of the entry)
WRW_ROWS = {(16, 16): 32, (16, 32): 128, (32, 32): 64}
STEM = (4, 16)
STEM_WRW_ROWS = 32

# the geometry table of conv_mfma.hip (kConv3Launches): (H, W, C, COUT, rows)
TABLE = [(42, 42, 16, 16, 32), (42, 42, 16, 32, 128), (21, 21, 32, 32, 64),
         (11, 11, 32, 32, 32)]
TABLE_FWD_ONLY = [(42, 42, 32, 16)]


def grid(shape, step, bound, gen):
    """Random multiples of `step` in [-bound, bound], float64."""
    n = int(round(bound / step))
    return torch.randint(-n, n + 1, shape, generator=gen).double() * step


def wrw_batch(H, W, rows):
    """Smallest N with at least two m-blocks of at least two passes each
    (9 <= passes: a block per 8 passes) and, where H*W allows it, a last
    pass that is ragged at the 32-row chunk (and so at the pass)."""
    hw = H * W
    n = (8 * rows) // hw + 1
    first = None
    while (n * hw + rows - 1) // rows <= 16:
        if first is None:
            first = n
        if (n * hw) % 32:
            return n
        n += 1
    return first if first is not None else n


def m_grid(M, rows, n_elem, plane_pad, resident):
    """The three m-grid rules of conv3x3p1_wrw: (blocks, wanted by the
    8-passes rule, plane cap)."""
    n_pass = (M + rows - 1) // rows
    want = (n_pass + 7) // 8
    cap = (16 << 20) // ((n_elem + plane_pad) * 4)
    return max(1, min(want, cap, resident)), want, cap


def make_case(H, W, N, C, COUT, seed=0):
    """Exact-grid operands (float64, NCHW, CPU) and their float64 results:
    out (bias + residual, no flags), out_rr (relu_in + relu_out, bias, no
    residual), gx / gx_masked (input gradient, masked where x <= 0),
    gw (COUT, 9C) in (kh, kw, c) order and gb, plain and with relu_in."""
    from distributed_rl_amd.ops import torch_ref

    gen = torch.Generator().manual_seed(1000 * H + 10 * W + C + COUT + seed)
    x = grid((N, C, H, W), 0.25, 2.0, gen)
    g = grid((N, COUT, H, W), 0.25, 2.0, gen)
    r = grid((N, COUT, H, W), 0.25, 2.0, gen)
    w = grid((COUT, C, 3, 3), 0.125, 1.0, gen)
    b = grid((COUT,), 0.125, 1.0, gen)
    d = dict(x=x, g=g, r=r, w=w, b=b)
    d["out"] = torch_ref.conv3x3_res(x, w, b, False, False, r)
    d["out_rr"] = torch_ref.conv3x3_res(x, w, b, True, True, None)

    def bwd(xin, want_x):
        return torch.ops.aten.convolution_backward(
            g, xin, w, [COUT], [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
            [want_x, True, True])

    gx, gw, gb = bwd(x, True)
    d["gx"] = gx
    # masked elements are written as +0 (a product would keep gx's sign)
    d["gx_masked"] = torch.where(x > 0, gx, torch.zeros_like(gx))
    d["gw"] = gw.permute(0, 2, 3, 1).reshape(COUT, 9 * C)
    d["gb"] = gb
    _, gw_r, _ = bwd(torch.relu(x), False)
    d["gw_relu"] = gw_r.permute(0, 2, 3, 1).reshape(COUT, 9 * C)
    return d
