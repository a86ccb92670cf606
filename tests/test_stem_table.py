"""The stem conv's one-entry geometry table (ops/hip/conv_mfma.hip
kStemLaunches) as seen through its support queries. Needs the built
extension but no GPU (`python -m distributed_rl_amd.ops.build`
cross-compiles it)."""

import pytest

STEM = (84, 84, 4, 16)  # (H, W, C, COUT): cfg/impala_resnet.json's first conv
OTHERS = [(42, 42, 16, 16), (84, 84, 4, 32), (84, 84, 8, 16)]


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd import ops

    e = ops.hip_ext(required=False)
    if e is None:
        pytest.skip("HIP extension not built")
    return e


def test_stem_geometry(ext):
    assert ext.conv3x3c4_supported(*STEM) is True
    assert ext.conv3x3c4_wrw_supported(*STEM) is True


@pytest.mark.parametrize("geom", OTHERS, ids=lambda g: "x".join(map(str, g)))
def test_nothing_else(ext, geom):
    assert ext.conv3x3c4_supported(*geom) is False
    assert ext.conv3x3c4_wrw_supported(*geom) is False


def test_stem_stays_out_of_the_conv3_table(ext):
    assert ext.conv3x3p1_supported(*STEM) is False
    assert ext.conv3x3p1_wrw_supported(*STEM) is False


def test_python_query():
    from distributed_rl_amd import ops

    if ops.hip_ext(required=False) is None:
        pytest.skip("HIP extension not built")
    assert ops.stem_conv_supported(*STEM)
    assert not ops.stem_conv_supported(42, 42, 16, 16)
    assert ops._STEM_DEFAULT is False
