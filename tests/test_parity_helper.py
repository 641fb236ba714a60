"""parity.f32_obs_mismatch on synthetic arrays (no GPU): what it must reject and admit, per layout.

Distances (and the ally flag) get 1 float32 ulp and nothing else; angles and cos/sin also get 1e-14
absolute (cancellation towards 0); only angle columns get the sign flip at +-pi."""
import numpy as np
import pytest

from parity import OBS_LAYOUTS, f32_obs_mismatch

LAYOUTS = sorted(OBS_LAYOUTS)
PI32 = np.float32(np.pi)


def base(layout):
    """A [3, 5, width] float64 observation of ordinary values: r = 1.0 exactly, angles / cos / sin 1.0."""
    c = OBS_LAYOUTS[layout]
    ref = np.ones((3, 5, len(c["exact"]) + len(c["angle"]) + len(c["cs"])), np.float64)
    return ref, ref.astype(np.float32)


def ulps(x, k):
    return (np.float32(x).view(np.int32) + np.int32(k)).view(np.float32)


def r_cols(layout):
    return [c for c in OBS_LAYOUTS[layout]["exact"]]


def loose_cols(layout):
    return list(OBS_LAYOUTS[layout]["angle"] + OBS_LAYOUTS[layout]["cs"])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_equal_arrays_count_zero(layout):
    ref, gpu = base(layout)
    assert f32_obs_mismatch(gpu, ref, layout) == 0
    gpu[0, 0, 0] = -0.0
    ref[0, 0, 0] = 0.0
    assert f32_obs_mismatch(gpu, ref, layout) == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", [2, -2, 16, -16])
def test_r_more_than_one_ulp_is_rejected(layout, k):
    """16 ulp at r = 1 is 1e-6: the modulo-2pi rule admitted it in every column."""
    for col in r_cols(layout):
        ref, gpu = base(layout)
        gpu[1, 2, col] = ulps(1.0, k)
        with pytest.raises(AssertionError):
            f32_obs_mismatch(gpu, ref, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_angle_off_by_1e_7_at_one_is_rejected(layout):
    """f32(1 - 1e-7) is 2 ulps below 1.0 (the ulp below 1 is 6e-8); 1e-7 is far above 1e-14."""
    for col in loose_cols(layout):
        ref, gpu = base(layout)
        gpu[2, 4, col] = np.float32(1.0 - 1e-7)
        assert abs(int(gpu[2, 4, col].view(np.int32)) - int(np.float32(1.0).view(np.int32))) == 2
        with pytest.raises(AssertionError):
            f32_obs_mismatch(gpu, ref, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_ulp_is_admitted_and_counted(layout):
    ref, gpu = base(layout)
    n = 0
    for col in range(gpu.shape[-1]):
        gpu[0, col % 5, col] = ulps(1.0, 1 if col % 2 else -1)
        n += 1
    assert f32_obs_mismatch(gpu, ref, layout) == n


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sign_flip_at_pi_only_in_angle_columns(layout):
    c = OBS_LAYOUTS[layout]
    for col in c["angle"]:
        for g, r in ((PI32, -PI32), (-PI32, PI32), (ulps(PI32, -2), -np.pi), (-ulps(PI32, 1), ulps(PI32, -1))):
            ref, gpu = base(layout)
            gpu[1, 1, col] = g
            ref[1, 1, col] = r
            assert f32_obs_mismatch(gpu, ref, layout) == 1
        for g, r in ((ulps(PI32, -3), -PI32), (PI32, -ulps(PI32, -3)), (np.float32(3.0), np.float32(-3.0))):
            ref, gpu = base(layout)
            gpu[1, 1, col] = g
            ref[1, 1, col] = r
            with pytest.raises(AssertionError):
                f32_obs_mismatch(gpu, ref, layout)
    for col in c["exact"] + c["cs"]:
        ref, gpu = base(layout)
        gpu[1, 1, col] = PI32
        ref[1, 1, col] = -PI32
        with pytest.raises(AssertionError):
            f32_obs_mismatch(gpu, ref, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cancellation_near_zero(layout):
    """1.0e-10 against 1.00005e-10 (5e-15 apart, ~400 float32 ulps): admitted in an angle or cos/sin
    column, rejected as a distance."""
    for col in loose_cols(layout):
        ref, gpu = base(layout)
        gpu[0, 3, col] = np.float32(1.0e-10)
        ref[0, 3, col] = 1.00005e-10
        assert f32_obs_mismatch(gpu, ref, layout) == 1
        gpu[0, 3, col] = np.float32(-1.0e-15)  # across zero as well
        ref[0, 3, col] = 2.0e-15
        assert f32_obs_mismatch(gpu, ref, layout) == 1
        gpu[0, 3, col] = np.float32(3.0e-14)
        with pytest.raises(AssertionError):
            f32_obs_mismatch(gpu, ref, layout)
    for col in r_cols(layout):
        ref, gpu = base(layout)
        gpu[0, 3, col] = np.float32(1.0e-10)
        ref[0, 3, col] = 1.00005e-10
        with pytest.raises(AssertionError):
            f32_obs_mismatch(gpu, ref, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_nan_is_rejected(layout):
    for col in range(len(OBS_LAYOUTS[layout]["exact"]) + len(loose_cols(layout))):
        ref, gpu = base(layout)
        gpu[0, 0, col] = np.nan
        with pytest.raises(AssertionError):
            f32_obs_mismatch(gpu, ref, layout)


def test_layout_is_required_and_checked():
    ref, gpu = base("tdm")
    with pytest.raises(TypeError):
        f32_obs_mismatch(gpu, ref)
    with pytest.raises(AssertionError):
        f32_obs_mismatch(gpu, ref, "flock_cart")  # 4 columns, not 6
    with pytest.raises(KeyError):
        f32_obs_mismatch(gpu, ref, "polar")
