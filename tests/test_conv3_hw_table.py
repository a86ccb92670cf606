"""The run-time H, W entries of the 3x3 pad-1 convs (ops/hip/conv_mfma.hip
kConv3HwLaunches, kStemHwLaunches) as seen through the support queries.
Needs the built extension but no GPU (`python -m distributed_rl_amd.ops.build`
cross-compiles it)."""

import pytest

SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (32, 32), (64, 64), (36, 48),
         (72, 96), (200, 3)]


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd import ops

    e = ops.hip_ext(required=False)
    if e is None:
        pytest.skip("HIP extension not built")
    return e


def test_forward_at_any_size(ext):
    assert ext.conv3x3p1_supported(64, 64, 16, 16) is True
    for H, W in SIZES:
        for C, COUT in [(16, 16), (16, 32), (32, 32), (32, 16)]:
            assert ext.conv3x3p1_supported(H, W, C, COUT) is True
        for C, COUT in [(8, 16), (16, 8), (4, 16), (16, 4), (64, 64),
                        (16, 48)]:
            assert ext.conv3x3p1_supported(H, W, C, COUT) is False
    for H, W in [(0, 5), (5, 0), (-1, 4)]:
        assert ext.conv3x3p1_supported(H, W, 16, 16) is False
        assert ext.conv3x3p1_wrw_supported(H, W, 16, 16) is False


def test_wrw_at_any_size(ext):
    for H, W in SIZES:
        for C, COUT in [(16, 16), (16, 32), (32, 32)]:
            assert ext.conv3x3p1_wrw_supported(H, W, C, COUT) is True
        # forward-only pair: the input gradient of a 16 -> 32 conv
        assert ext.conv3x3p1_wrw_supported(H, W, 32, 16) is False
        assert ext.conv3x3p1_wrw_supported(H, W, 8, 16) is False


def test_what_the_table_tests_pin(ext):
    assert ext.conv3x3p1_supported(84, 84, 4, 16) is False
    assert ext.conv3x3p1_supported(84, 84, 16, 4) is False
    assert ext.conv3x3p1_wrw_supported(42, 42, 32, 16) is False
    assert ext.conv3x3p1_wrw_supported(84, 84, 4, 16) is False


def test_stem(ext):
    assert ext.conv3x3c4_hw_supported(4, 16) is True
    for C, COUT in [(4, 32), (8, 16), (16, 16), (3, 16)]:
        assert ext.conv3x3c4_hw_supported(C, COUT) is False
    # the table bindings keep rejecting everything but 84x84
    assert ext.conv3x3c4_supported(64, 64, 4, 16) is False
    assert ext.conv3x3c4_wrw_supported(64, 64, 4, 16) is False
    assert ext.conv3x3c4_supported(84, 84, 4, 16) is True


def test_python_queries():
    from distributed_rl_amd import ops

    if ops.hip_ext(required=False) is None:
        pytest.skip("HIP extension not built")
    assert ops.conv3x3_supported(64, 64, 16, 16)
    assert ops.conv3x3_supported(5, 7, 32, 16)
    assert not ops.conv3x3_supported(5, 7, 8, 16)
    assert ops.stem_conv_supported(64, 64, 4, 16)
    assert ops.stem_conv_supported(84, 84, 4, 16)
    assert ops.stem_conv_supported(1, 9, 4, 16)
    assert not ops.stem_conv_supported(42, 42, 16, 16)
    assert not ops.stem_conv_supported(64, 64, 4, 32)
    assert not ops.stem_conv_supported(0, 64, 4, 16)
    assert ops._STEM_DEFAULT is False


def test_any_hw_keyword_has_a_default(ext):
    """Existing positional calls are unaffected: any_hw is trailing and
    defaults to False."""
    for name in ("conv3x3p1_fwd", "conv3x3p1_wrw", "conv3x3p1_dgrad"):
        assert "any_hw: bool = False" in getattr(ext, name).__doc__, name
