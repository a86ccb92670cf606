"""The one conv forward binding and the shared argument checks
(ops/hip/conv_mfma.hip host code): every geometry at one job, rejection of
mismatched tensors, and the autograd contract of the one-job path."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16

# (H, W, C, KH, KW, S, COUT) — same table as tests/test_gpu_conv.py
SHAPES = [
    (84, 84, 4, 8, 8, 4, 32),
    (20, 20, 32, 4, 4, 2, 64),
    (9, 9, 64, 3, 3, 1, 64),
    (84, 84, 4, 8, 8, 4, 16),
    (20, 20, 16, 4, 4, 2, 32),
]
N = 3


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _job(shape, u8=False, n=N, seed=0):
    H, W, C, KH, KW, S, COUT = shape
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    if u8:
        x = _cl(torch.randint(0, 256, (n, C, H, W), dtype=torch.uint8,
                              device=DEV, generator=g))
    else:
        x = _cl(torch.randn(n, C, H, W, device=DEV, generator=g).to(BF16))
    w = _cl((torch.randn(COUT, C, KH, KW, device=DEV, generator=g) * 0.05
             ).to(BF16))
    b = (torch.randn(COUT, device=DEV, generator=g) * 0.1).to(BF16)
    return x, w, b


def _out(shape, n=N, dtype=BF16, fill=float("nan")):
    H, W, C, KH, KW, S, COUT = shape
    P, Q = (H - KH) // S + 1, (W - KW) // S + 1
    return _cl(torch.full((n, COUT, P, Q), fill, dtype=dtype, device=DEV))


ONE_JOB_CASES = [(s, False) for s in SHAPES] + [(SHAPES[0], True),
                                                (SHAPES[3], True)]


@pytest.mark.parametrize("shape,u8", ONE_JOB_CASES,
                         ids=lambda v: "x".join(map(str, v))
                         if isinstance(v, tuple) else f"u8{int(v)}")
def test_one_job_every_geometry(ext, shape, u8):
    """One job runs the single-job kernel of every table row, the two rows
    without a grouped variant included."""
    from distributed_rl_amd import ops

    S = shape[5]
    x, w, b = _job(shape, u8, seed=21)
    out = _out(shape)
    ext.conv_fwd_grouped([x], [w], [b], [out], S, False)
    ref_op = ops.fused_conv_relu(x, w, b, S)
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any()
    assert torch.equal(out, ref_op)
    xf = (x.float() / 255.0).to(BF16).float() if u8 else x.float()
    ref = F.relu(F.conv2d(xf, w.float(), b.float(), stride=S))
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err / scale < 2e-2, f"{shape}: max err {err} scale {scale}"


# ---------------------------------------------------------------------------
# argument rejection. Every bad tensor is larger or wider than the right one
# (never smaller, never on the host), so a call that slipped through a
# missing check would still stay inside its allocations.
# ---------------------------------------------------------------------------

G9 = SHAPES[2]  # 9x9x64 -> 64, k3 s1: P = Q = 7
IMPALA2 = SHAPES[4]


def _fwd_args():
    x, w, b = _job(G9, seed=31)
    return dict(x=x, w=w, b=b, out=_out(G9, fill=0.0), chw=False)


def _fwd_bad_fp32_input(a):
    a["x"] = _cl(a["x"].float())


def _fwd_bad_u8_chw(a):
    # channels_last u8 view of a buffer of twice the bytes the kernel reads
    buf = torch.zeros(2 * a["x"].numel(), dtype=torch.uint8, device=DEV)
    a["x"] = buf[: a["x"].numel()].view(N, 9, 9, 64).permute(0, 3, 1, 2)
    a["out"] = torch.zeros(N, 64 * 49, dtype=BF16, device=DEV)
    a["chw"] = True


def _fwd_bad_weight_c(a):
    a["w"] = _cl(torch.zeros(64, 128, 3, 3, dtype=BF16, device=DEV))


def _fwd_bad_fp32_out(a):
    a["out"] = _out(G9, dtype=torch.float32, fill=0.0)


def _fwd_bad_out_rows(a):
    a["out"] = _out(G9, n=N + 1, fill=0.0)


def _fwd_bad_out_nchw(a):
    a["out"] = torch.zeros(N, 64, 7, 7, dtype=BF16, device=DEV)


def _fwd_bad_bias_len(a):
    a["b"] = torch.zeros(2 * 64, dtype=BF16, device=DEV)


FWD_BAD = [_fwd_bad_fp32_input, _fwd_bad_u8_chw, _fwd_bad_weight_c,
           _fwd_bad_fp32_out, _fwd_bad_out_rows, _fwd_bad_out_nchw,
           _fwd_bad_bias_len]


@pytest.mark.parametrize("spoil", FWD_BAD, ids=lambda f: f.__name__[9:])
def test_fwd_rejects(ext, spoil):
    a = _fwd_args()
    ext.conv_fwd_grouped([a["x"]], [a["w"]], [a["b"]], [a["out"]], 1, False)
    spoil(a)
    with pytest.raises(RuntimeError):
        ext.conv_fwd_grouped([a["x"]], [a["w"]], [a["b"]], [a["out"]], 1,
                             a["chw"])
    torch.cuda.synchronize()


def test_fwd_rejects_five_jobs(ext):
    a = _fwd_args()
    outs = [_out(G9, fill=0.0) for _ in range(5)]
    with pytest.raises(RuntimeError):
        ext.conv_fwd_grouped([a["x"]] * 5, [a["w"]] * 5, [a["b"]] * 5, outs,
                             1, False)
    torch.cuda.synchronize()


def _wrw_args():
    x, _, _ = _job(G9, seed=41)
    gout = _out(G9, fill=0.5)
    return dict(x=x, gout=gout,
                gw=torch.zeros(64, 9 * 64, dtype=torch.float32, device=DEV),
                gb=torch.zeros(64, dtype=torch.float32, device=DEV))


def _wrw_bad_fp32_in(a):
    a["x"] = _cl(a["x"].float())


def _wrw_bad_fp32_gout(a):
    a["gout"] = _cl(a["gout"].float())


def _wrw_bad_gout_batch(a):
    a["gout"] = _out(G9, n=N + 1, fill=0.5)


def _wrw_bad_gb_dtype(a):
    # bf16 gw_ws with an fp32 gb_ws: the bf16 reduce would write half of it
    a["gw"] = torch.zeros(64, 9 * 64, dtype=BF16, device=DEV)


@pytest.mark.parametrize("spoil", [_wrw_bad_fp32_in, _wrw_bad_fp32_gout,
                                   _wrw_bad_gout_batch, _wrw_bad_gb_dtype],
                         ids=lambda f: f.__name__[9:])
def test_wrw_rejects(ext, spoil):
    a = _wrw_args()
    ext.conv_wrw(a["x"], a["gout"], a["gw"], a["gb"], 1)
    spoil(a)
    with pytest.raises(RuntimeError):
        ext.conv_wrw(a["x"], a["gout"], a["gw"], a["gb"], 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", ["fp32_dst", "dst_rows"])
def test_relu_mask_bwd_chw_rejects(ext, bad):
    C, PQ = 64, 49
    gout = torch.ones(N, C * PQ, dtype=BF16, device=DEV)
    outv = torch.ones(N, C * PQ, dtype=BF16, device=DEV)
    dst = _out(G9, fill=0.0)
    ext.relu_mask_bwd_chw(gout, outv, dst, C, PQ)
    dst = (_out(G9, dtype=torch.float32, fill=0.0) if bad == "fp32_dst"
           else _out(G9, n=N + 1, fill=0.0))
    with pytest.raises(RuntimeError):
        ext.relu_mask_bwd_chw(gout, outv, dst, C, PQ)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", ["fp32_gout", "w_t_twice"])
def test_dgrad_rejects(ext, bad):
    _, w, _ = _job(G9, seed=51)
    gout = _out(G9, fill=0.5)
    dx = _cl(torch.zeros(N, 64, 9, 9, dtype=BF16, device=DEV))
    w_t = torch.zeros(w.numel(), dtype=BF16, device=DEV)
    ext.conv_dgrad(gout, w, w_t, dx, 1)
    if bad == "fp32_gout":
        gout = _cl(gout.float())
    else:
        w_t = torch.zeros(2 * w.numel(), dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError):
        ext.conv_dgrad(gout, w, w_t, dx, 1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# autograd contract of the one-job path
# ---------------------------------------------------------------------------

G20 = SHAPES[1]  # 20x20x32 -> 64, k4 s2


def test_one_job_grads_equal_grouped_job0(ext):
    from distributed_rl_amd import ops

    S = G20[5]
    x0, w0, b0 = _job(G20, seed=61)
    x1, w1, b1 = _job(G20, seed=62)
    _, w2, b2 = _job(G20, seed=63)
    leaves = [t.detach().clone().requires_grad_(True) for t in (x0, w0, b0)]
    ref_leaves = [t.detach().clone().requires_grad_(True)
                  for t in (x0, w0, b0)]
    out = ops.fused_conv_relu(*leaves, S)
    refs = ops.fused_conv_relu_grouped(
        [ref_leaves[0], x1, x1], [ref_leaves[1], w1, w2],
        [ref_leaves[2], b1, b2], S)
    assert out.requires_grad and torch.equal(out, refs[0])
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    gout = _cl(torch.randn(out.shape, device=DEV, generator=g).to(BF16))
    out.backward(gout)
    refs[0].backward(gout)
    torch.cuda.synchronize()
    for a, b in zip(leaves, ref_leaves):
        assert a.grad is not None and torch.equal(a.grad, b.grad)


def test_one_job_no_grad_output_is_plain(ext):
    from distributed_rl_amd import ops

    x, w, b = (t.requires_grad_(True) for t in _job(G20, seed=64))
    with torch.no_grad():
        out = ops.fused_conv_relu(x, w, b, G20[5])
    assert out.requires_grad is False and out.grad_fn is None


def test_one_job_weight_only_grad(ext):
    from distributed_rl_amd import ops

    x, w, b = _job(G20, seed=65)
    w.requires_grad_(True)
    out = ops.fused_conv_relu(x, w, b, G20[5])
    out.backward(_cl(torch.ones_like(out)))
    torch.cuda.synchronize()
    assert w.grad is not None and w.grad.shape == w.shape
    assert x.grad is None and b.grad is None
