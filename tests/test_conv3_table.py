"""The 3x3 pad-1 geometry table (ops/hip/conv_mfma.hip kConv3Launches) as
seen through its support queries. Needs the built extension but no GPU
(`python -m distributed_rl_amd.ops.build` cross-compiles it)."""

import pytest

# (H, W, C, COUT) — cfg/impala_resnet.json at 84x84
GEOMS = [(42, 42, 16, 16), (42, 42, 16, 32), (21, 21, 32, 32),
         (11, 11, 32, 32)]


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd import ops

    e = ops.hip_ext(required=False)
    if e is None:
        pytest.skip("HIP extension not built")
    return e


def test_wrw_geometries(ext):
    for g in GEOMS:
        assert ext.conv3x3p1_wrw_supported(*g) is True, g
    # the first conv stays on the library
    assert ext.conv3x3p1_wrw_supported(84, 84, 4, 16) is False
    # forward-only entry: the input gradient of the 16->32 conv
    assert ext.conv3x3p1_wrw_supported(42, 42, 32, 16) is False


def test_mirrored_forward_geometries(ext):
    """Every geometry's input gradient is the forward kernel at
    (H, W, COUT, C); 42x42 32->16 exists for that alone."""
    assert ext.conv3x3p1_supported(42, 42, 32, 16) is True
    for (H, W, C, COUT) in GEOMS:
        assert ext.conv3x3p1_supported(H, W, COUT, C) is True
    assert ext.conv3x3p1_supported(84, 84, 16, 4) is False
