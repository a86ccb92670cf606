"""CPU oracles of the sum-tree kernels (ops/torch_ref.py sumtree_build,
sumtree_hash01, sumtree_bump_seed, sumtree_sample) against independent
implementations: Python big integers for the hash and the seed step, a
float64 cumulative sum + searchsorted for the descent, the pairwise-summation
error bound for the root. tests/test_gpu_replay.py holds the device kernels
to these oracles bit for bit."""

import math

import numpy as np
import pytest
import torch

from distributed_rl_amd.ops import torch_ref

M64 = (1 << 64) - 1


def hash01_bigint(seed, i):
    """splitmix64 counter hash with Python integers, masked by hand."""
    z = ((seed & M64) + 0x9E3779B97F4A7C15 * (1 + i)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    # a 24-bit integer and its product with 2^-24 are exact in fp32
    return (z >> 40) / 16777216.0


HASH_SEEDS = [0, 1, 7, 165, 0x5EED, (1 << 63) - 1, 1 << 63, (1 << 63) + 12345,
              M64 - 1, M64, 0x9E3779B97F4A7C15, 6364136223846793005]
HASH_COUNTERS = [0, 1, 2, 3, 63, 64, 255, 256, 1000, 4095, 65535, 65536,
                 131071, 131072, (1 << 24) - 1, (1 << 24) + 1, (1 << 31) - 1,
                 (1 << 31), (1 << 32) - 1]


def test_hash01_matches_bigint():
    n = 0
    for seed in HASH_SEEDS:
        got = torch_ref.sumtree_hash01(seed, np.array(HASH_COUNTERS))
        assert got.dtype == np.float32 and got.shape == (len(HASH_COUNTERS),)
        for j, i in enumerate(HASH_COUNTERS):
            want = hash01_bigint(seed, i)
            assert float(got[j]) == want, (seed, i, float(got[j]), want)
            assert 0.0 <= float(got[j]) < 1.0
            n += 1
    assert n >= 200
    # a scalar counter, and a seed given as the negative int64 the device
    # tensor shows for a word at or above 2^63
    assert float(torch_ref.sumtree_hash01(7, 5)) == hash01_bigint(7, 5)
    neg = torch.tensor([(1 << 63) + 12345 - (1 << 64)], dtype=torch.int64)
    assert float(torch_ref.sumtree_hash01(int(neg.item()), 9)) == \
        hash01_bigint((1 << 63) + 12345, 9)


def test_hash01_range_over_a_long_run():
    h = torch_ref.sumtree_hash01(165, np.arange(1 << 17))
    assert h.min() >= 0.0 and h.max() < 1.0
    # 24-bit outputs: the mean of 131072 uniform draws is within 5 sigma
    assert abs(float(h.astype(np.float64).mean()) - 0.5) < 5 / math.sqrt(12 * (1 << 17))


@pytest.mark.parametrize("start", [0, 0x5EED, (1 << 63) - 1, (1 << 63) + 99,
                                   M64])
def test_bump_seed_matches_int64_wraparound(start):
    """The LCG mod 2^64 against torch's int64 arithmetic, which wraps: the
    two agree as 64-bit words over a run of bumps."""
    s = start
    t = torch.tensor([start - (1 << 64) if start >= 1 << 63 else start],
                     dtype=torch.int64)
    for _ in range(5):
        s = torch_ref.sumtree_bump_seed(s)
        t = t * 6364136223846793005 + 1442695040888963407
        assert 0 <= s <= M64
        assert s == int(t.item()) % (1 << 64)


def _next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


# (capacity, n_valid, k, seed); seed 165 with k = 131072 makes the last
# stratum's float32(i) + h round up to k, so u == total: the tail guard case
SAMPLE_CASES = [(5000, 5000, 512, 7), (5000, 3001, 131072, 165),
                (8192, 8192, 131072, 165), (1, 1, 4, 3), (3, 2, 64, 1)]


@pytest.mark.parametrize("capacity,n_valid,k,seed", SAMPLE_CASES)
def test_sample_matches_searchsorted_oracle(capacity, n_valid, k, seed):
    """Integer priorities 1..15 make every fp32 node sum and every u -= lv of
    the descent exact, so the descent must land on the leaf the float64
    cumulative sum names for the same fp32 u — for every draw."""
    rng = np.random.default_rng(1000 + capacity + n_valid)
    P = _next_pow2(capacity)
    leaves = np.zeros(capacity, dtype=np.float32)
    leaves[:n_valid] = rng.integers(1, 16, n_valid).astype(np.float32)
    tree = torch_ref.sumtree_build(leaves, P)
    assert float(tree[1]) == float(leaves.astype(np.float64).sum())

    idx, prob = torch_ref.sumtree_sample(tree, P, n_valid, k, seed)
    assert idx.dtype == np.int64 and prob.dtype == np.float32

    i = np.arange(k)
    h = torch_ref.sumtree_hash01(seed, i)
    total = np.float32(tree[1])
    u = (i.astype(np.float32) + h) * (total / np.float32(k))
    assert u.dtype == np.float32
    cdf = np.cumsum(leaves[:n_valid].astype(np.float64))
    raw = np.searchsorted(cdf, u.astype(np.float64), side="right")
    want = np.minimum(raw, n_valid - 1)
    assert np.array_equal(idx, want), np.flatnonzero(idx != want)[:10]
    assert np.array_equal(
        prob, leaves[want] / total), "prob is leaf / root in fp32"
    assert idx.min() >= 0 and idx.max() < n_valid
    if k == 131072:
        # the guard case must stay in the set
        assert int((u >= total).sum()) >= 1
        assert int((raw >= n_valid).sum()) >= 1
        assert idx[-1] == n_valid - 1


def test_sample_tail_guard_clamps_a_draw_that_leaves_the_valid_range():
    """u == total walks right at every level and ends on leaf P - 1; with
    n_valid < P that leaf is empty and the clamp must bring it back."""
    P, n_valid, k, seed = 8192, 3001, 131072, 165
    leaves = np.ones(n_valid, dtype=np.float32)
    tree = torch_ref.sumtree_build(leaves, P)
    u_last = (np.float32(k - 1) + torch_ref.sumtree_hash01(seed, k - 1)) * \
        (tree[1] / np.float32(k))
    assert u_last >= tree[1]
    idx, prob = torch_ref.sumtree_sample(tree, P, n_valid, k, seed)
    assert idx[-1] == n_valid - 1 and prob[-1] > 0


@pytest.mark.parametrize("n,P", [(1, 1), (2, 2), (3, 4), (1000, 1024),
                                 (5000, 8192), (1 << 16, 1 << 16)])
def test_build_nodes_and_root_bound(n, P):
    rng = np.random.default_rng(n)
    leaves = (rng.random(n) * 10 + 1e-3).astype(np.float32)
    tree = torch_ref.sumtree_build(leaves, P)
    assert tree.dtype == np.float32 and tree.shape == (2 * P,)
    assert tree[0] == 0
    assert np.array_equal(tree[P : P + n], leaves)
    assert not tree[P + n :].any()
    # every node is the fp32 sum of its children, one node at a time
    for node in range(1, P):
        assert tree[node] == np.float32(tree[2 * node] + tree[2 * node + 1])
    # pairwise summation of positive terms: log2(P) roundings on every path
    sum64 = float(leaves.astype(np.float64).sum())
    bound = 1.01 * max(math.log2(P), 0) * 2.0 ** -24 * sum64
    assert abs(float(tree[1]) - sum64) <= bound, (float(tree[1]), sum64, bound)


def test_dequant_roundings_agree_for_every_byte():
    """What lets the device dequant tests demand equality: for all 256 bytes
    bf16(v * fl32(1/255)), bf16(fl32(v / 255)) and bf16 of the float64
    quotient are the same bf16, and the fp32 product is within 1e-7 of the
    quotient."""
    v = torch.arange(256)
    inv255 = torch.tensor(1.0, dtype=torch.float32) / 255
    prod = v.float() * inv255
    a = prod.to(torch.bfloat16)
    b = (v.float() / 255).to(torch.bfloat16)
    c = (v.double() / 255).to(torch.bfloat16)
    # round to nearest even on the exact rational v / 255, in integers:
    # bf16 has 8 significant bits
    for x in range(1, 256):
        e = math.floor(math.log2(x / 255))
        while (x << 64) < (255 << (64 + e)):  # guard the float log2
            e -= 1
        while (x << 64) >= (255 << (65 + e)):
            e += 1
        # x/255 = m * 2^(e-7) with m in [128, 256)
        num, den = x << (7 - e), 255
        m, r = divmod(num, den)
        if 2 * r > den or (2 * r == den and m & 1):
            m += 1
        assert float(c[x]) == m * 2.0 ** (e - 7), x
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    assert torch.equal(b.view(torch.int16), c.view(torch.int16))
    assert (prod.double() - v.double() / 255).abs().max().item() <= 1e-7


def test_oversized_push_keeps_the_last_capacity_rows():
    """ReplayBase.push trims a batch larger than the ring to its last
    `capacity` rows and writes them from write_pos on; HipSumTreePER takes
    push and _ring_indices from ReplayBase unchanged, so TorchPER shows the
    contract (the plain wrap is in tests/test_per_semantics.py)."""
    from distributed_rl_amd.replay.gpu_per import HipSumTreePER
    from distributed_rl_amd.replay.per import ReplayBase, TorchPER

    assert HipSumTreePER.push is ReplayBase.push
    assert HipSumTreePER._ring_indices is ReplayBase._ring_indices
    per = TorchPER(8, {"x": ((), torch.float32)})
    per.push({"x": torch.arange(3.0)}, torch.ones(3))
    per.push({"x": torch.arange(100.0, 113.0)},
             torch.arange(100.0, 113.0))
    assert len(per) == 8 and per.write_pos == 3 and per.count == 11
    # rows 105..112 survive, written from slot 3 on, wrapping
    want = torch.tensor([110.0, 111, 112, 105, 106, 107, 108, 109])
    assert torch.equal(per.data["x"], want)
    assert torch.equal(per.priorities, want)
