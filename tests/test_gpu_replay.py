"""The replay path's kernels (ops/hip/drl_kernels.hip: sum-tree update /
sample / min / weights / seed, gather_rows, seq_transpose_rows, dequant,
relu_mask_bwd) against exact references. Every operation in them but the
IS-weight power is one correctly rounded fp32 operation, 64-bit integer
arithmetic or a byte copy, so the assertions are bit equalities; the one
tolerance is the measured __powf bound of per_weights (docs/KERNELS.md, K10).
The last section spoils one argument per call and expects the host checks to
reject it before anything is launched."""

import math

import numpy as np
import pytest
import torch

from distributed_rl_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
TREE_TOP = 2048  # kTreeTop of drl_kernels.hip
M64 = (1 << 64) - 1
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


def _next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _seed_tensor(seed_u64):
    """The unsigned seed word as the int64 the device tensor stores."""
    s = seed_u64 & M64
    return torch.tensor([s - (1 << 64) if s >= 1 << 63 else s],
                        dtype=torch.int64, device=DEV)


def _seed_value(seed_t):
    return int(seed_t.item()) & M64


def _update(ext, tree, P, idx, prio):
    ext.sumtree_update(tree, _dev(idx, torch.int64),
                       _dev(prio, torch.float32), P)


# ---------------------------------------------------------------------------
# sum-tree update: every node, bit-exact
# ---------------------------------------------------------------------------


def _check_tree(tree_dev, P, capacity, expect_leaves, what):
    t = tree_dev.cpu().numpy()
    assert t.shape == (2 * P,) and t[0] == 0, what
    assert np.array_equal(_bits(t[P : P + capacity]), _bits(expect_leaves)), \
        f"{what}: leaves"
    assert not t[P + capacity :].any(), f"{what}: leaves at or above capacity"
    # every inner node is the fp32 sum of its two children ...
    assert np.array_equal(_bits(t[1:P]), _bits(t[2 : 2 * P : 2] + t[3 : 2 * P : 2])), \
        f"{what}: node != left + right"
    # ... which is the bottom-up build of the expected leaves
    ref = torch_ref.sumtree_build(expect_leaves, P)
    assert np.array_equal(_bits(t), _bits(ref)), f"{what}: tree != reference"
    return t


def _update_sets(capacity, P, rng):
    """(name, idx) in the order they are applied. With sub = P / top leaves
    under each node of the top level: fewer than `top` indices rebuild one
    subtree per index, `top` or more rebuild every subtree."""
    top = min(P, TREE_TOP)
    sub = P // top
    sets = [("m=1", np.array([capacity // 2])),
            ("full push", rng.permutation(capacity)),
            ("ends", np.unique([0, capacity - 1]))]
    j = max(1, (capacity // 2) // sub)
    if j * sub < capacity:
        sets.append(("subtree boundary", np.array([j * sub - 1, j * sub])))
    lo = sub if 2 * sub <= capacity else 0
    inside = lo + rng.permutation(min(sub, capacity - lo))
    sets.append(("one subtree", inside[: max(1, (3 * len(inside)) // 4)]))
    sets.append(("m=2047", rng.permutation(capacity)[:2047]))
    if capacity >= 2048:
        sets.append(("m=2048", rng.permutation(capacity)[:2048]))
    sets.append(("equal duplicates", rng.integers(0, capacity, 300)))
    return sets


# 1, 2, 64: small trees; 1000: P = 1024 < top, no mid level; 2048: depth 0
# boundary; 4096: first mid level; 5000: P = 8192, capacity not a power of
# two; 2^17: P / top = 64, 64-thread blocks; 2^19: P / top = 256, 256-thread
@pytest.mark.parametrize("capacity", [1, 2, 64, 1000, 2048, 4096, 5000,
                                      1 << 17, 1 << 19])
def test_sumtree_update_every_node(ext, capacity):
    rng = np.random.default_rng(capacity)
    P = _next_pow2(capacity)
    tree = torch.zeros(2 * P, dtype=torch.float32, device=DEV)
    expect = np.zeros(capacity, dtype=np.float32)
    for name, idx in _update_sets(capacity, P, rng):
        # a priority per leaf, so duplicate indices carry equal priorities
        table = (rng.random(capacity) * 10 + 0.01).astype(np.float32)
        before = expect.copy()
        expect[idx] = table[idx]
        _update(ext, tree, P, idx, table[idx])
        what = f"capacity {capacity}, {name} (m = {len(idx)})"
        t = _check_tree(tree, P, capacity, expect, what)
        untouched = np.ones(capacity, dtype=bool)
        untouched[idx] = False
        assert np.array_equal(_bits(t[P : P + capacity][untouched]),
                              _bits(before[untouched])), what
        assert np.array_equal(_bits(t[P + idx]), _bits(table[idx])), what


# ---------------------------------------------------------------------------
# sampler: exact
# ---------------------------------------------------------------------------

SAMPLE_CAPACITY = 5000


@pytest.fixture(scope="module")
def sample_trees(ext):
    """n_valid -> (device tree, its host copy), random fp32 priorities in
    leaves [0, n_valid) of a capacity-5000 tree, built by sumtree_update."""
    P = _next_pow2(SAMPLE_CAPACITY)
    out = {}
    for n_valid in (5000, 3001):
        rng = np.random.default_rng(n_valid)
        prio = (rng.random(n_valid) * 4 + 1e-3).astype(np.float32)
        tree = torch.zeros(2 * P, dtype=torch.float32, device=DEV)
        _update(ext, tree, P, np.arange(n_valid), prio)
        host = tree.cpu().numpy()
        assert np.array_equal(_bits(host),
                              _bits(torch_ref.sumtree_build(prio, P)))
        out[n_valid] = (tree, host)
    return P, out


def _round_up_seed(k):
    """First seed whose last stratum rounds float32(k - 1) + h up to k, which
    makes u == total: the draw the tail guard exists for."""
    for seed in range(2000):
        h = torch_ref.sumtree_hash01(seed, k - 1)
        if np.float32(k - 1) + np.float32(h) == np.float32(k):
            return seed
    raise AssertionError("no seed among 2000 rounds the last stratum up")


# 1000 is no power of two, so total / k rounds; the 512 case carries a seed
# word at or above 2^63 (a negative int64 in the tensor)
SAMPLE_KS = [(1, 11), (64, 0x5EED), (512, (1 << 63) + 0x1234567),
             (1000, 77), (131072, None)]


@pytest.mark.parametrize("n_valid", [5000, 3001])
@pytest.mark.parametrize("k,seed", SAMPLE_KS, ids=[str(k) for k, _ in SAMPLE_KS])
def test_sumtree_sample_exact(ext, sample_trees, n_valid, k, seed):
    P, trees = sample_trees
    tree, host = trees[n_valid]
    guard = seed is None
    if guard:
        seed = _round_up_seed(k)
    seed_t = _seed_tensor(seed)
    idx = torch.full((k,), -1, dtype=torch.int64, device=DEV)
    prob = torch.full((k,), float("nan"), dtype=torch.float32, device=DEV)
    ext.sumtree_sample(tree, P, n_valid, k, seed_t, idx, prob)
    idx, prob = idx.cpu().numpy(), prob.cpu().numpy()
    assert _seed_value(seed_t) == seed, "sampling must not move the seed"

    ref_idx, ref_prob = torch_ref.sumtree_sample(host, P, n_valid, k, seed)
    bad = np.flatnonzero(idx != ref_idx)
    assert bad.size == 0, (bad[:8], idx[bad[:8]], ref_idx[bad[:8]])
    assert np.array_equal(_bits(prob), _bits(ref_prob))

    # independent of the reference
    assert idx.min() >= 0 and idx.max() < n_valid
    assert (prob > 0).all()
    leaves = host[P : P + n_valid].astype(np.float64)
    cdf = np.cumsum(leaves)
    total = cdf[-1]
    eps = 1.01 * math.log2(P) * 2.0 ** -24 * total
    i = np.arange(k, dtype=np.float64)
    s_lo, s_hi = i * total / k, (i + 1) * total / k
    l_lo, l_hi = cdf[idx] - leaves[idx], cdf[idx]
    off = np.flatnonzero((l_lo > s_hi + eps) | (l_hi < s_lo - eps))
    assert off.size == 0, ("draw outside its stratum", off[:8])
    if guard:
        u_last = (np.float32(k - 1) + torch_ref.sumtree_hash01(seed, k - 1)) \
            * (host[1] / np.float32(k))
        assert u_last >= host[1], "the guard case left the set"
        assert idx[-1] == n_valid - 1


# ---------------------------------------------------------------------------
# leaf_min_pos
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n_valid", [1, 63, 65, 300001])
def test_leaf_min_pos_exact(ext, n_valid):
    rng = np.random.default_rng(n_valid)
    P = _next_pow2(n_valid + 1)
    leaves = (rng.random(n_valid) * 8 + 0.5).astype(np.float32)
    if n_valid > 1:
        leaves[rng.random(n_valid) < 0.2] = 0.0
        leaves[n_valid // 2] = 0.25  # a minimum that no zero can remove
    host = np.zeros(2 * P, dtype=np.float32)
    host[P : P + n_valid] = leaves
    host[P + n_valid] = 0.0625  # smaller, but outside [0, n_valid)
    tree = _dev(host)
    out = torch.full((1,), INF_BITS, dtype=torch.int32, device=DEV)
    ext.leaf_min_pos(tree, P, n_valid, out)
    want = leaves[leaves > 0].min()
    assert int(out.item()) == int(_bits(want)[0]), (out.item(), want)

    # nothing positive in range: the +inf bits stay
    host[P : P + n_valid] = 0.0
    out = torch.full((1,), INF_BITS, dtype=torch.int32, device=DEV)
    ext.leaf_min_pos(_dev(host), P, n_valid, out)
    assert int(out.item()) == INF_BITS


# ---------------------------------------------------------------------------
# per_weights
# ---------------------------------------------------------------------------

# Largest relative error of per_weights against fp64 measured over this
# test's inputs on an MI355X: 2.289e-7 at beta 0.4, 2.117e-7 at beta 1.0
# (docs/KERNELS.md, K10). The bound is four times that, and never above the
# 1e-3 of test_sumtree_is_weights_vs_oracle.
PER_WEIGHTS_MEASURED = 2.289e-7
PER_WEIGHTS_RTOL = min(4 * PER_WEIGHTS_MEASURED, 1e-3)


@pytest.mark.parametrize("beta", [0.4, 1.0])
def test_per_weights_vs_fp64(ext, beta):
    """One draw per leaf, priorities log-uniform over 1e-3 .. 1e3, so the
    draw of the minimum-priority leaf is in the batch and must weigh 1."""
    rng = np.random.default_rng(4)
    n = 4096
    P = n
    prio = (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    prio[17], prio[4000] = 1e-3, 1e3
    tree = torch.zeros(2 * P, dtype=torch.float32, device=DEV)
    _update(ext, tree, P, np.arange(n), prio)
    host = tree.cpu().numpy()
    total = host[1]
    prob = host[P:] / total  # fp32, as the sampler computes it
    min_bits = torch.full((1,), INF_BITS, dtype=torch.int32, device=DEV)
    ext.leaf_min_pos(tree, P, n, min_bits)
    assert int(min_bits.item()) == int(_bits(prio.min())[0])
    w = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    ext.per_weights(_dev(prob), min_bits, tree, n, beta, w)
    w = w.cpu().numpy().astype(np.float64)

    p64 = prob.astype(np.float64)
    max_w = (1.0 / (n * (float(prio.min()) / float(total)))) ** beta
    ref = (1.0 / (n * p64)) ** beta / max_w
    rel = np.abs(w - ref) / ref
    print(f"per_weights beta={beta}: max rel err {rel.max():.4g} "
          f"(bound {PER_WEIGHTS_RTOL:.4g}), weight of the min leaf "
          f"{w[17]!r}")
    assert rel.max() <= PER_WEIGHTS_RTOL
    assert int(np.argmin(prio)) == 17
    assert abs(w[17] - 1.0) <= PER_WEIGHTS_RTOL
    assert w.max() <= 1.0 + PER_WEIGHTS_RTOL


# ---------------------------------------------------------------------------
# bump_seed and graph replay
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("start", [0x5EED, (1 << 63) + 99, M64])
def test_bump_seed_exact(ext, start):
    seed_t = _seed_tensor(start)
    s = start
    for _ in range(5):
        ext.bump_seed(seed_t)
        s = torch_ref.sumtree_bump_seed(s)
        assert _seed_value(seed_t) == s


def _float_per(capacity, n, seed=1234):
    from distributed_rl_amd.replay.gpu_per import HipSumTreePER

    per = HipSumTreePER(capacity, {"x": ((), torch.float32)}, DEV, seed=seed)
    g = torch.Generator().manual_seed(capacity + n)
    prio = torch.rand(n, generator=g) * 3 + 0.01
    per.push({"x": torch.arange(float(n)).to(DEV)}, prio.to(DEV))
    return per


def test_graph_replay_bumps_the_seed(ext):
    """sample() captured once on one stream: every replay runs the in-kernel
    seed bump again, so replay j draws with the seed bumped j more times."""
    per = _float_per(5000, 5000)
    k = 256
    out = (torch.empty(k, dtype=torch.int64, device=DEV),
           torch.empty(k, dtype=torch.float32, device=DEV),
           torch.empty(k, dtype=torch.float32, device=DEV))
    per.sample(k, 0.4, with_data=False, out=out)  # eager, one bump
    torch.cuda.synchronize()
    host = per.tree.cpu().numpy()
    s = torch_ref.sumtree_bump_seed(1234)
    assert _seed_value(per.seed) == s
    assert np.array_equal(
        out[0].cpu().numpy(),
        torch_ref.sumtree_sample(host, per.P, 5000, k, s)[0])

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        per.sample(k, 0.4, with_data=False, out=out)
    seen = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        s = torch_ref.sumtree_bump_seed(s)
        assert _seed_value(per.seed) == s
        ref_idx, ref_prob = torch_ref.sumtree_sample(host, per.P, 5000, k, s)
        idx = out[0].cpu().numpy()
        assert np.array_equal(idx, ref_idx)
        assert np.array_equal(_bits(out[1].cpu().numpy()), _bits(ref_prob))
        seen.append(idx)
    assert not np.array_equal(seen[0], seen[1])
    assert not np.array_equal(seen[1], seen[2])
    assert not np.array_equal(seen[0], seen[2])


# ---------------------------------------------------------------------------
# end to end through HipSumTreePER
# ---------------------------------------------------------------------------


def test_per_push_wrap_update_sample(ext):
    from distributed_rl_amd.replay.gpu_per import HipSumTreePER

    cap = 1000
    schema = {"a": ((3,), torch.float32), "b": ((), torch.int64),
              "f": ((4, 12, 12), torch.uint8)}
    per = HipSumTreePER(cap, schema, DEV, seed=9)
    g = torch.Generator().manual_seed(5)
    expect = np.zeros(cap, dtype=np.float32)
    rows = torch.zeros(cap, dtype=torch.int64)  # which pushed row a slot holds
    serial = 0
    for n, start in ((700, 0), (600, 700)):
        prio = torch.rand(n, generator=g) + 0.05
        ids = torch.arange(serial, serial + n)
        cols = {"a": ids.float().view(n, 1).expand(n, 3).contiguous().to(DEV),
                "b": (ids * 3 + 1).to(DEV),
                "f": (ids % 251).to(torch.uint8).view(n, 1, 1, 1)
                .expand(n, 4, 12, 12).contiguous().to(DEV)}
        per.push(cols, prio.to(DEV))
        slots = (np.arange(n) + start) % cap  # the ring wraps in the 2nd push
        expect[slots] = prio.numpy()
        rows[torch.from_numpy(slots)] = ids
        serial += n
    assert len(per) == cap and per.write_pos == 300
    _check_tree(per.tree, per.P, cap, expect, "after the wrapping push")
    assert torch.equal(per.data["b"].cpu(), rows * 3 + 1)

    data, idx, w = per.sample(64, 0.4)
    table = (torch.rand(cap, generator=g) + 0.05)
    per.update(idx, table.to(DEV)[idx])
    idx_h = idx.cpu().numpy()
    expect[idx_h] = table.numpy()[idx_h]
    _check_tree(per.tree, per.P, cap, expect, "after update of a batch")

    data, idx, w = per.sample(256, 0.4)
    assert int(idx.min()) >= 0 and int(idx.max()) < cap
    for name, col in per.data.items():
        assert torch.equal(data[name], col.index_select(0, idx)), name
    assert torch.equal(data["b"].cpu(), rows[idx.cpu()] * 3 + 1)
    assert torch.isfinite(w).all() and float(w.max()) <= 1.0 + PER_WEIGHTS_RTOL


# ---------------------------------------------------------------------------
# gather_rows: 16-byte rows in chunks, one-chunk rows, ragged byte rows
# ---------------------------------------------------------------------------

GATHER_CAP = 37
POISON = 0xA5


def _random_column(shape, dtype, gen):
    if dtype == torch.bool:
        return torch.randint(0, 2, shape, generator=gen).bool().to(DEV)
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen)
    return raw.view(dtype).view(shape).to(DEV)


def _as_bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _guarded(k, guard, shape, dtype):
    """(buffer of k + guard poison rows, its first k rows)."""
    buf = torch.empty((k + guard, *shape), dtype=dtype, device=DEV)
    _as_bytes(buf).fill_(POISON)
    return buf, buf[:k]


@pytest.fixture(scope="module")
def gather_columns():
    gen = torch.Generator().manual_seed(21)
    cap = GATHER_CAP
    specs = [((1027 * 16,), torch.uint8),   # 16432 B: chunk-split, ragged last
             ((4, 12, 12), torch.uint8),    # 576 B: 16-byte pieces
             ((), torch.int64), ((), torch.float32), ((), torch.bool),
             ((7,), BF16),                  # 14 B: byte path
             ((5,), torch.uint8),           # 5 B: byte path
             ((4,), torch.float32)]         # the 8th column
    return [_random_column((cap, *shape), dtype, gen)
            for shape, dtype in specs]


@pytest.mark.parametrize("ncols", [7, 8])
@pytest.mark.parametrize("k", [1, 3, 600])
def test_gather_rows_exact(ext, gather_columns, k, ncols):
    cap = GATHER_CAP
    gen = torch.Generator().manual_seed(k)
    idx = torch.randint(0, cap, (k,), generator=gen)
    # duplicates, 0 and cap - 1 (k = 1 has room for the last row only)
    idx[: min(k, 3)] = torch.tensor([cap - 1, 0, cap - 1])[: min(k, 3)]
    idx = idx.to(DEV)
    srcs = gather_columns[:ncols]
    kept = [s.clone() for s in srcs]
    bufs = [_guarded(k, 2, s.shape[1:], s.dtype) for s in srcs]
    ext.gather_rows(idx, srcs, [d for _, d in bufs])
    for c, (src, (buf, dst)) in enumerate(zip(srcs, bufs)):
        assert torch.equal(_as_bytes(dst),
                           _as_bytes(src.index_select(0, idx))), f"column {c}"
        assert bool((_as_bytes(buf[k:]) == POISON).all()), f"guard of {c}"
        assert torch.equal(_as_bytes(src), _as_bytes(kept[c])), f"src {c}"


def test_replay_gather_goes_through_gather_rows(ext):
    """ReplayBase.gather on the device: same rows, index given as int32."""
    per = _float_per(64, 64)
    idx = torch.tensor([63, 0, 5, 5], dtype=torch.int32, device=DEV)
    got = per.gather(idx)
    assert torch.equal(got["x"], per.data["x"].index_select(0, idx))


# ---------------------------------------------------------------------------
# seq_transpose_rows and ops.seq_transpose
# ---------------------------------------------------------------------------

# row bytes: 16, 48, and 300 * 16 (more than one pass of 256 lanes)
ROW_BYTES = [16, 48, 300 * 16]


@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (5, 3)])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, BF16],
                         ids=["u8", "f32", "bf16"])
def test_seq_transpose_exact(ext, B, T, dtype):
    from distributed_rl_amd import ops

    gen = torch.Generator().manual_seed(B * 10 + T)
    esz = torch.empty(0, dtype=dtype).element_size()
    for rb in ROW_BYTES:
        n = rb // esz
        # one flat row, and the same bytes as a 2-D row
        for row_shape in ((n,), (2, n // 2)):
            src = _random_column((B, T, *row_shape), dtype, gen)
            want = _as_bytes(src.transpose(0, 1).contiguous())
            buf = torch.empty((T * B + 1, *row_shape), dtype=dtype,
                              device=DEV)
            _as_bytes(buf).fill_(POISON)
            dst = buf[: T * B].view(T, B, *row_shape)
            ext.seq_transpose_rows(src, dst)
            assert torch.equal(_as_bytes(dst), want), (rb, row_shape)
            assert bool((_as_bytes(buf[T * B :]) == POISON).all())
            out = ops.seq_transpose(src)
            assert out.shape == (T, B, *row_shape) and out.is_contiguous()
            assert torch.equal(_as_bytes(out), want), (rb, row_shape)


def test_seq_transpose_ragged_row_takes_the_fallback(ext):
    from distributed_rl_amd import ops

    gen = torch.Generator().manual_seed(3)
    src = _random_column((3, 5, 20), torch.uint8, gen)  # 20 B rows
    out = ops.seq_transpose(src)
    assert out.is_contiguous()
    assert torch.equal(out, src.transpose(0, 1).contiguous())


# ---------------------------------------------------------------------------
# dequant
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (3, 5, 7), (2, 84, 84)])
def test_dequant_nhwc_exact(ext, N, H, W):
    """Plane c holds (v + 64c) % 256, so a swapped or repeated channel shows;
    bf16(v * fl32(1/255)) equals the bf16 rounding of the exact quotient for
    all 256 bytes (tests/test_replay_ref.py), so equality is the demand."""
    from distributed_rl_amd import ops

    v = (torch.arange(N * H * W) % 256).view(N, 1, H, W)
    x = ((v + 64 * torch.arange(4).view(1, 4, 1, 1)) % 256).to(torch.uint8)
    if x.numel() >= 256:
        assert torch.unique(x).numel() == 256
    y = ops.dequant_frames_nhwc(x.to(DEV))
    assert y.dtype == BF16 and y.shape == x.shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    if H * W > 1:
        assert y.stride() == (4 * H * W, 1, 4 * W, 4)
    ref = (x.double() / 255).to(BF16)
    assert torch.equal(y.cpu().contiguous().view(torch.int16),
                       ref.view(torch.int16))


def test_dequant_f32_exact_odd_shape(ext):
    from distributed_rl_amd import ops

    # 420 elements: a multiple of 4 and of nothing larger the kernel uses
    x = ((torch.arange(420) * 89 + 3) % 256).to(torch.uint8).view(3, 5, 7, 4)
    assert torch.unique(x).numel() == 256
    y = ops.dequant_frames(x.to(DEV), torch.float32).cpu()
    assert y.shape == x.shape and y.dtype == torch.float32
    inv255 = torch.tensor(1.0, dtype=torch.float32) / 255
    want = x.float() * inv255
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert (y.double() - x.double() / 255).abs().max().item() <= 1e-7
    assert torch.allclose(y, torch_ref.dequant_frames(x.float()), atol=1e-7)


# ---------------------------------------------------------------------------
# relu_mask_bwd
# ---------------------------------------------------------------------------

# bf16 bit patterns. out: +0, -0, positive subnormals, +inf, negatives,
# positives, -inf, a negative subnormal. out = NaN is left out: the model's
# out is the ReLU output of finite convs, and the kernel's sign-bit test and
# `out > 0` disagree on NaN by construction (a positive NaN is kept).
OUT_POOL = [0x0000, 0x8000, 0x0001, 0x7F80, 0xBF80, 0x3F80, 0xFF80, 0x8001,
            0x007F, 0xC2F7, 0x0080, 0x7F7F]
# gout: NaNs of both signs and a payload, infinities, zeros, ordinary values
GOUT_POOL = [0x7FC0, 0x3FC0, 0xFF80, 0x7F80, 0xFFC0, 0xC000, 0x0000, 0x7FA1,
             0x7F7F, 0x8000, 0x0001, 0x4049, 0xBDCC]


def _pattern(n):
    i = torch.arange(n)
    out = torch.tensor(OUT_POOL)[i % len(OUT_POOL)]
    gout = torch.tensor(GOUT_POOL)[(i * 7 + i // len(OUT_POOL)) % len(GOUT_POOL)]
    return out, gout


def _bf16_from_bits(bits, shape, channels_last):
    # 0..65535 -> the int16 with the same 16 bits
    t = ((bits + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(shape)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.to(DEV).view(BF16)


# 4 and 1028 elements; two sizes above 2048 blocks * 256 lanes * 4 elements
# (2097152), where the grid-stride loop runs a second, partial time
RELU_SHAPES = [((1, 4), False), ((1, 4, 1, 1), True),
               ((257, 4), False), ((1, 4, 1, 257), True),
               ((4103, 512), False), ((2, 16, 129, 509), True)]


@pytest.mark.parametrize("shape,channels_last", RELU_SHAPES,
                         ids=["x".join(map(str, s)) for s, _ in RELU_SHAPES])
def test_relu_mask_bwd_exact(ext, shape, channels_last):
    n = int(np.prod(shape))
    out_bits, gout_bits = _pattern(n)
    out = _bf16_from_bits(out_bits, shape, channels_last)
    gout = _bf16_from_bits(gout_bits, shape, channels_last)
    assert out.stride() == gout.stride()
    dst = torch.empty_like(gout)
    dst.view(torch.int16).fill_(0x5A5A)
    ext.relu_mask_bwd(gout, out, dst)
    # fp32 compare of the bf16 values on the host; kept elements carry
    # gout's bits (NaN payloads, infinities, -0 included), masked ones +0
    keep = out.cpu().float() > 0
    assert not out.cpu().float().isnan().any()
    want = torch.where(keep, gout.cpu().view(torch.int16),
                       torch.zeros((), dtype=torch.int16))
    got = dst.cpu().view(torch.int16)
    assert torch.equal(got, want)
    if n >= len(OUT_POOL) * len(GOUT_POOL):
        g = gout.cpu().float()
        assert bool((keep & g.isnan()).any()) and bool((~keep & g.isnan()).any())
        assert bool((keep & g.isinf()).any()) and bool((~keep & g.isinf()).any())


# ---------------------------------------------------------------------------
# host-side rejection: one spoiled argument per call, thrown before launch
# ---------------------------------------------------------------------------


def _i64(n, dev=DEV):
    return torch.zeros(n, dtype=torch.int64, device=dev)


def _f32(n, dev=DEV):
    return torch.zeros(n, dtype=torch.float32, device=dev)


def _u8(*shape, dev=DEV):
    return torch.zeros(shape, dtype=torch.uint8, device=dev)


GATHER_BAD = {
    "idx int32": lambda: (torch.zeros(3, dtype=torch.int32, device=DEV),
                          [_u8(10, 16)], [_u8(3, 16)]),
    "idx strided": lambda: (_i64(6)[::2], [_u8(10, 16)], [_u8(3, 16)]),
    "idx on host": lambda: (_i64(3, "cpu"), [_u8(10, 16)], [_u8(3, 16)]),
    "src on host": lambda: (_i64(3), [_u8(10, 16, dev="cpu")], [_u8(3, 16)]),
    "dst on host": lambda: (_i64(3), [_u8(10, 16)], [_u8(3, 16, dev="cpu")]),
    "dst dtype": lambda: (_i64(3), [_u8(10, 16)],
                          [torch.zeros(3, 16, dtype=torch.int8, device=DEV)]),
    "src strided": lambda: (_i64(3), [_u8(10, 32)[:, :16]], [_u8(3, 16)]),
    "dst strided": lambda: (_i64(3), [_u8(10, 16)], [_u8(3, 32)[:, :16]]),
    "dst rows": lambda: (_i64(3), [_u8(10, 16)], [_u8(4, 16)]),
    "dst row bytes": lambda: (_i64(3), [_u8(10, 16)], [_u8(3, 32)]),
    "src empty": lambda: (_i64(3), [_u8(0, 16)], [_u8(3, 16)]),
    "second column": lambda: (_i64(3), [_u8(10, 16), _u8(10, 5)],
                              [_u8(3, 16), _u8(2, 5)]),
    "nine columns": lambda: (_i64(3), [_u8(10, 16)] * 9, [_u8(3, 16)] * 9),
    "no dst": lambda: (_i64(3), [_u8(10, 16)], []),
}


@pytest.mark.parametrize("case", sorted(GATHER_BAD))
def test_gather_rows_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.gather_rows(*GATHER_BAD[case]())


TRANSPOSE_BAD = {
    "src 1-D": lambda: (_u8(16), _u8(16)),
    "dst dtype": lambda: (_u8(3, 5, 16),
                          torch.zeros(5, 3, 16, dtype=torch.int8, device=DEV)),
    "dst on host": lambda: (_u8(3, 5, 16), _u8(5, 3, 16, dev="cpu")),
    "src on host": lambda: (_u8(3, 5, 16, dev="cpu"), _u8(5, 3, 16)),
    "dst not swapped": lambda: (_u8(3, 5, 16), _u8(3, 5, 16)),
    "dst row": lambda: (_u8(3, 5, 16), _u8(5, 3, 32)),
    "dst strided": lambda: (_u8(3, 5, 16), _u8(5, 3, 32)[:, :, :16]),
    "src strided": lambda: (_u8(3, 5, 32)[:, :, :16], _u8(5, 3, 16)),
    "ragged row": lambda: (_u8(3, 5, 20), _u8(5, 3, 20)),
}


@pytest.mark.parametrize("case", sorted(TRANSPOSE_BAD))
def test_seq_transpose_rows_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.seq_transpose_rows(*TRANSPOSE_BAD[case]())


UPDATE_BAD = {
    "tree f64": lambda: (torch.zeros(16, dtype=torch.float64, device=DEV),
                         _i64(2), _f32(2), 8),
    "tree on host": lambda: (_f32(16, "cpu"), _i64(2), _f32(2), 8),
    "tree not 2P": lambda: (_f32(16), _i64(2), _f32(2), 16),
    "tree strided": lambda: (_f32(32)[::2], _i64(2), _f32(2), 8),
    "P not a power of two": lambda: (_f32(12), _i64(2), _f32(2), 6),
    "P zero": lambda: (_f32(0), _i64(2), _f32(2), 0),
    "lengths differ": lambda: (_f32(16), _i64(3), _f32(2), 8),
    "idx int32": lambda: (_f32(16),
                          torch.zeros(2, dtype=torch.int32, device=DEV),
                          _f32(2), 8),
    "idx strided": lambda: (_f32(16), _i64(4)[::2], _f32(2), 8),
    "idx on host": lambda: (_f32(16), _i64(2, "cpu"), _f32(2), 8),
    "prio f64": lambda: (_f32(16), _i64(2),
                         torch.zeros(2, dtype=torch.float64, device=DEV), 8),
    "prio strided": lambda: (_f32(16), _i64(2), _f32(4)[::2], 8),
    "prio on host": lambda: (_f32(16), _i64(2), _f32(2, "cpu"), 8),
}


@pytest.mark.parametrize("case", sorted(UPDATE_BAD))
def test_sumtree_update_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.sumtree_update(*UPDATE_BAD[case]())


def _ones_tree():
    """P = 8, every leaf 1: a tree a mistaken launch could still walk."""
    return _dev(torch_ref.sumtree_build(np.ones(8, dtype=np.float32), 8))


# (tree, P, n_valid, k, seed, out_idx, out_prob)
SAMPLE_BAD = {
    "n_valid zero": lambda: (_ones_tree(), 8, 0, 4, _i64(1), _i64(4), _f32(4)),
    "n_valid above P": lambda: (_ones_tree(), 8, 9, 4, _i64(1), _i64(4),
                                _f32(4)),
    "k zero": lambda: (_ones_tree(), 8, 8, 0, _i64(1), _i64(0), _f32(0)),
    "tree not 2P": lambda: (_ones_tree(), 16, 8, 4, _i64(1), _i64(4),
                            _f32(4)),
    "tree on host": lambda: (_ones_tree().cpu(), 8, 8, 4, _i64(1), _i64(4),
                             _f32(4)),
    "seed int32": lambda: (_ones_tree(), 8, 8, 4,
                           torch.zeros(1, dtype=torch.int32, device=DEV),
                           _i64(4), _f32(4)),
    "seed two words": lambda: (_ones_tree(), 8, 8, 4, _i64(2), _i64(4),
                               _f32(4)),
    "seed on host": lambda: (_ones_tree(), 8, 8, 4, _i64(1, "cpu"), _i64(4),
                             _f32(4)),
    "out_idx int32": lambda: (_ones_tree(), 8, 8, 4, _i64(1),
                              torch.zeros(4, dtype=torch.int32, device=DEV),
                              _f32(4)),
    "out_idx short": lambda: (_ones_tree(), 8, 8, 4, _i64(1), _i64(3),
                              _f32(4)),
    "out_idx strided": lambda: (_ones_tree(), 8, 8, 4, _i64(1), _i64(8)[::2],
                                _f32(4)),
    "out_prob f64": lambda: (_ones_tree(), 8, 8, 4, _i64(1), _i64(4),
                             torch.zeros(4, dtype=torch.float64, device=DEV)),
    "out_prob short": lambda: (_ones_tree(), 8, 8, 4, _i64(1), _i64(4),
                               _f32(3)),
    "out_prob on host": lambda: (_ones_tree(), 8, 8, 4, _i64(1), _i64(4),
                                 _f32(4, "cpu")),
}


@pytest.mark.parametrize("case", sorted(SAMPLE_BAD))
def test_sumtree_sample_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.sumtree_sample(*SAMPLE_BAD[case]())


def _i32(n, dev=DEV):
    return torch.full((n,), INF_BITS, dtype=torch.int32, device=dev)


# (tree, P, n_valid, out_bits)
MIN_BAD = {
    "out_bits int64": lambda: (_ones_tree(), 8, 8, _i64(1)),
    "out_bits two words": lambda: (_ones_tree(), 8, 8, _i32(2)),
    "out_bits on host": lambda: (_ones_tree(), 8, 8, _i32(1, "cpu")),
    "n_valid zero": lambda: (_ones_tree(), 8, 0, _i32(1)),
    "n_valid above P": lambda: (_ones_tree(), 8, 9, _i32(1)),
    "tree f64": lambda: (_ones_tree().double(), 8, 8, _i32(1)),
    "tree not 2P": lambda: (_ones_tree(), 4, 4, _i32(1)),
}


@pytest.mark.parametrize("case", sorted(MIN_BAD))
def test_leaf_min_pos_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.leaf_min_pos(*MIN_BAD[case]())


# (prob, min_bits, tree, n_valid, beta, out_w)
WEIGHTS_BAD = {
    "prob f64": lambda: (torch.zeros(4, dtype=torch.float64, device=DEV),
                         _i32(1), _ones_tree(), 8, 0.4, _f32(4)),
    "prob on host": lambda: (_f32(4, "cpu"), _i32(1), _ones_tree(), 8, 0.4,
                             _f32(4)),
    "prob strided": lambda: (_f32(8)[::2], _i32(1), _ones_tree(), 8, 0.4,
                             _f32(4)),
    "min_bits f32": lambda: (_f32(4), _f32(1), _ones_tree(), 8, 0.4, _f32(4)),
    "min_bits empty": lambda: (_f32(4), _i32(0), _ones_tree(), 8, 0.4,
                               _f32(4)),
    "tree on host": lambda: (_f32(4), _i32(1), _ones_tree().cpu(), 8, 0.4,
                             _f32(4)),
    "tree f64": lambda: (_f32(4), _i32(1), _ones_tree().double(), 8, 0.4,
                         _f32(4)),
    "n_valid zero": lambda: (_f32(4), _i32(1), _ones_tree(), 0, 0.4, _f32(4)),
    "out_w short": lambda: (_f32(4), _i32(1), _ones_tree(), 8, 0.4, _f32(3)),
    "out_w f64": lambda: (_f32(4), _i32(1), _ones_tree(), 8, 0.4,
                          torch.zeros(4, dtype=torch.float64, device=DEV)),
    "out_w on host": lambda: (_f32(4), _i32(1), _ones_tree(), 8, 0.4,
                              _f32(4, "cpu")),
}


@pytest.mark.parametrize("case", sorted(WEIGHTS_BAD))
def test_per_weights_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.per_weights(*WEIGHTS_BAD[case]())


def test_bump_seed_rejects(ext):
    with pytest.raises(RuntimeError):
        ext.bump_seed(torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ext.bump_seed(_i64(1, "cpu"))
    with pytest.raises(RuntimeError):
        ext.bump_seed(_i64(2))


def _bf(*shape, dev=DEV):
    return torch.zeros(shape, dtype=BF16, device=dev)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# (gout, out, dst)
RELU_BAD = {
    "dst f32": lambda: (_bf(2, 8), _bf(2, 8),
                        torch.zeros(2, 8, dtype=torch.float32, device=DEV)),
    "out f16": lambda: (_bf(2, 8),
                        torch.zeros(2, 8, dtype=torch.float16, device=DEV),
                        _bf(2, 8)),
    "gout f32": lambda: (torch.zeros(2, 8, dtype=torch.float32, device=DEV),
                         _bf(2, 8), _bf(2, 8)),
    "dst smaller": lambda: (_bf(2, 8), _bf(2, 8), _bf(1, 8)),
    "out larger": lambda: (_bf(2, 8), _bf(4, 8), _bf(2, 8)),
    "same count, other shape": lambda: (_bf(2, 8), _bf(2, 8), _bf(4, 4)),
    "out strides": lambda: (_cl(_bf(2, 4, 3, 3)), _bf(2, 4, 3, 3),
                            _cl(_bf(2, 4, 3, 3))),
    "dst strides": lambda: (_cl(_bf(2, 4, 3, 3)), _cl(_bf(2, 4, 3, 3)),
                            _bf(2, 4, 3, 3)),
    "gout transposed": lambda: (_bf(8, 4).t(), _bf(4, 8), _bf(4, 8)),
    "not dense": lambda: (_bf(2, 16)[:, ::2], _bf(2, 16)[:, ::2],
                          _bf(2, 16)[:, ::2]),
    "dst on host": lambda: (_bf(2, 8), _bf(2, 8), _bf(2, 8, dev="cpu")),
    "gout on host": lambda: (_bf(2, 8, dev="cpu"), _bf(2, 8), _bf(2, 8)),
    "count not a multiple of 4": lambda: (_bf(2, 3), _bf(2, 3), _bf(2, 3)),
}


@pytest.mark.parametrize("case", sorted(RELU_BAD))
def test_relu_mask_bwd_rejects(ext, case):
    with pytest.raises(RuntimeError):
        ext.relu_mask_bwd(*RELU_BAD[case]())


def test_dequant_nhwc_rejects(ext):
    x = _u8(2, 4, 3, 3)
    with pytest.raises(RuntimeError):
        ext.dequant_nhwc(x, _cl(_bf(2, 4, 3, 4)))
    with pytest.raises(RuntimeError):
        ext.dequant_nhwc(x, _cl(_bf(2, 4, 3, 3, dev="cpu")))
    with pytest.raises(RuntimeError):
        ext.dequant_nhwc(x, _bf(2, 4, 3, 3))


def test_linear_relu_backward_with_a_permuted_gradient(ext):
    """A dense but transposed incoming gradient: the backward must mask the
    logical elements, not walk two differently strided buffers in step."""
    from distributed_rl_amd import ops

    K, N, B = 3136, 1024, 8  # the one size linear_relu is built for
    assert ops.linear_relu_supported(K, N)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(B, K, generator=gen).to(BF16).to(DEV).requires_grad_(True)
    w = (torch.randn(N, K, generator=gen) * 0.05).to(BF16).to(DEV)
    b = torch.zeros(N, dtype=BF16, device=DEV)
    y = ops.fused_linear_relu(x, w, b)
    g = torch.randn(N, B, generator=gen).to(BF16).to(DEV).t()  # dense, permuted
    (gx,) = torch.autograd.grad(y, x, g)
    want = (g * (y > 0)).double().mm(w.double())
    err = (gx.double() - want).abs().max().item()
    # bf16 result: half an ulp, 2^-9 of the element; fp32 accumulation of
    # 1024 products whose absolute sum is about sqrt(1024) times the result:
    # 1024 * 2^-24 * 32 = 2^-9 again. Twice their sum; a gradient masked at
    # the wrong elements is off by the size of the result itself.
    assert err <= 2 ** -7 * want.abs().max().item()
