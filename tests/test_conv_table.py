"""The conv geometry table (ops/hip/conv_mfma.hip kConvs) as seen through
the one support query. Needs the built extension but no GPU
(`python -m distributed_rl_amd.ops.build` cross-compiles it)."""

import pytest

# (H, W, C, KH, KW, S, COUT), u8, grouped, chw_out, chw_out grouped
TABLE = [
    ((84, 84, 4, 8, 8, 4, 32), True, True, False, False),
    ((84, 84, 4, 8, 8, 4, 32), False, True, False, False),
    ((20, 20, 32, 4, 4, 2, 64), False, True, False, False),
    ((9, 9, 64, 3, 3, 1, 64), False, True, True, True),
    ((84, 84, 4, 8, 8, 4, 16), True, False, False, False),
    ((84, 84, 4, 8, 8, 4, 16), False, False, False, False),
    ((20, 20, 16, 4, 4, 2, 32), False, False, True, False),
]


@pytest.fixture(scope="module")
def ops():
    from distributed_rl_amd import ops

    if ops.hip_ext(required=False) is None:
        pytest.skip("HIP extension not built")
    return ops


@pytest.mark.parametrize("row", TABLE,
                         ids=lambda r: "x".join(map(str, r[0])) + f"-u8{int(r[1])}")
def test_support_matrix(ops, row):
    geom, u8, grouped, chw, chw_grouped = row
    expect = {(False, 1): True, (False, 3): grouped,
              (True, 1): chw, (True, 3): chw_grouped}
    for (chw_out, njobs), want in expect.items():
        got = ops.conv_supported(*geom, u8, chw_out=chw_out, njobs=njobs)
        assert got is want, (geom, u8, chw_out, njobs)
    assert ops.conv_supported(*geom, u8) is True  # defaults: NHWC, one job
    assert ops.hip_ext().conv_wrw_supported(*geom, u8) is True


def test_near_misses_unsupported(ops):
    ext = ops.hip_ext()
    # wrong stride
    assert not ops.conv_supported(84, 84, 4, 8, 8, 2, 32, True)
    assert not ops.conv_supported(9, 9, 64, 3, 3, 2, 64, False, chw_out=True)
    assert not ext.conv_wrw_supported(20, 20, 32, 4, 4, 1, 64, False)
    # u8 on bf16-only rows
    assert not ops.conv_supported(20, 20, 32, 4, 4, 2, 64, True)
    assert not ops.conv_supported(9, 9, 64, 3, 3, 1, 64, True, chw_out=True)
    assert not ext.conv_wrw_supported(9, 9, 64, 3, 3, 1, 64, True)
    # COUT 48
    assert not ops.conv_supported(84, 84, 4, 8, 8, 4, 48, True)
    assert not ext.conv_wrw_supported(84, 84, 4, 8, 8, 4, 48, False)
    # more jobs than one launch takes, and none
    assert ops.conv_supported(9, 9, 64, 3, 3, 1, 64, False, njobs=4)
    assert not ops.conv_supported(9, 9, 64, 3, 3, 1, 64, False, njobs=5)
    assert not ops.conv_supported(9, 9, 64, 3, 3, 1, 64, False, njobs=0)
    # transposed kernel extent / input extent
    assert not ops.conv_supported(84, 84, 4, 8, 4, 4, 32, True)
    assert not ops.conv_supported(84, 80, 4, 8, 8, 4, 32, True)
