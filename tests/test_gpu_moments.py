"""Temporal luminance moments on the GPU (include/mcpt.h: mcpt_temporal_accumulate_moments, mcpt_moments_variance): the kMoments
instantiations of k_temporal_accumulate and k_moments_variance give the bits of the host build of the same header functions
(tests/native/moments_driver.cpp) on the inputs of tests/test_moments_cpu.py -- the random frames, the seams, the values that are not finite
-- at 8 x 8, 13 x 17 and 24 x 40, where a window of radius 3 crosses 16 x 16 block edges in both axes, and with radius 4 there.  A NaN the
rule forms (the luminance of a NaN colour) may differ in its payload between the two processors; every other value is compared bit for
bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moments_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = mc.SHAPES + [(24, 40)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return mc.build_driver(tmp_path_factory.mktemp("moments_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


def _windows(shape):
    return mc.WINDOWS + ([(3, 4)] if shape == (24, 40) else [])


@pytest.mark.parametrize("switches", mc.SWITCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_host_build_random_frames(hip, tiny, driver, shape, switches):
    H, W = shape
    args, history, aov = mc.frame_case(H, W, switches)
    got = tiny.temporal_accumulate_moments(*args, max_history=8, **history)
    want = mc.host_accumulate(driver, hip, *args, history=history, max_history=8)
    if not any(switches):
        want[2][...] = 0  # (both switches off: the entry point reports no flags)
    assert mc.same(got[0], want[0]) and mc.bits_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert mc.same(got[3], want[3]), int((got[3].view(np.uint32) != want[3].view(np.uint32)).sum())
    # the colour, the length and the flags are mcpt_temporal_accumulate_ex's
    color, motion, normal, prev_color, prev_depth, prev_len, prev_normal, prev_moments = args
    rng = np.random.default_rng(7)
    var, pvar = rng.random((H, W)).astype(f32), rng.random((H, W)).astype(f32)
    ex = tiny.temporal_accumulate_ex(color, var, motion, normal, prev_color, pvar, prev_depth, prev_len, prev_normal, max_history=8, **history)
    assert mc.bits_equal(got[0], ex[0]) and mc.bits_equal(got[1], ex[2]) and np.array_equal(got[2], ex[3])
    for min_len, radius in _windows(shape):
        for flags in (want[2], None):
            v = tiny.moments_variance(want[3], want[1], aov, flags=flags, min_len=min_len, radius=radius)
            assert mc.bits_equal(v, mc.host_variance(driver, hip, want[3], want[1], flags, aov, min_len=min_len, radius=radius)), (min_len, radius)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_host_build_seams(hip, tiny, driver, shape):
    H, W = shape
    rng = np.random.default_rng(61)
    mom, _ = mc.noise_moments(H, W, rng)
    length = np.ones((H, W), f32)
    for name, aov, near in mc.seam_cases(H, W):
        sz = 0.1 if name == "depth" else 0.0
        for min_len, radius in _windows(shape):
            v = tiny.moments_variance(mom, length, aov, min_len=min_len, radius=radius, sigma_z=sz)
            assert mc.bits_equal(v, mc.host_variance(driver, hip, mom, length, None, aov, min_len=min_len, radius=radius, sigma_z=sz)), (name, radius)
        if name == "lone":
            assert mc.bits_equal(v[near], mom[near][:, 1])


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_host_build_values_that_are_not_finite(hip, tiny, driver, shape):
    """Stored moments that are not finite on used taps, colours that are not finite, clamped pixels."""
    H, W = shape
    rng = np.random.default_rng(71 + H)
    color, motion, normal, prev_color, prev_depth, prev_len, prev_normal, prev_moments = mc.accumulate_case(H, W, seed=3)
    motion[..., 0:2] = np.round(motion[..., 0:2] * 2) / 2
    prev_len = np.maximum(prev_len, 1).astype(f32)
    bad = rng.random((H, W)) < 0.2
    prev_moments[bad, rng.integers(0, 2, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), int(bad.sum()))
    color[rng.random((H, W)) < 0.1, 0] = np.inf
    color[0, 0, 2] = np.nan
    args = (color, motion, normal, prev_color, prev_depth, prev_len, prev_normal, prev_moments)
    history = dict(color_clamp=True, clamp_k=0.5)
    got = tiny.temporal_accumulate_moments(*args, max_history=8, **history)
    want = mc.host_accumulate(driver, hip, *args, history=history, max_history=8)
    assert mc.same(got[0], want[0]) and mc.bits_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and mc.same(got[3], want[3])
    l = mc.lum(color)
    restarted = (want[1] > 1) & ~np.isfinite(prev_moments).all(-1) & (motion[..., 0] == 0) & (motion[..., 1] == 0)
    assert restarted.any() and mc.bits_equal(got[3][restarted], np.stack([l, l * l], -1)[restarted])
    assert (want[2] & 2).any() and (~np.isfinite(want[3]).all(-1)).any()
    aov = mc.aov_case(H, W, seed=3)
    for min_len, radius in _windows(shape):
        v = tiny.moments_variance(want[3], want[1], aov, flags=want[2], min_len=min_len, radius=radius)
        assert mc.bits_equal(v, mc.host_variance(driver, hip, want[3], want[1], want[2], aov, min_len=min_len, radius=radius)), (min_len, radius)
        assert np.array_equal(np.isinf(v), ~np.isfinite(want[3]).all(-1))
