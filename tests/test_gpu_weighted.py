"""History weighted by sample counts on the GPU (include/mcpt.h: mcpt_temporal_accumulate_weighted, mcpt_temporal_history_weight,
mcpt_render_adaptive_weighted): k_temporal_accumulate<.., .., true> and k_history_weight give the bits of the CPU build of the same header
functions (tests/native/weighted_driver.cpp) at 8 x 8, 17 x 13 (partial tiles) and 64 x 64 (several blocks), every flavour, with a count
plane and with a uniform count; the argument checks come first; and a weight-guided adaptive frame is mcpt_render_adaptive_guided with a null
plane, never samples a pixel more than the unguided rule, equals mcpt_render at every pixel's count, and in round 0 stops the pixels that
the frame guide N stops when H = (N - 1) S0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import bits_equal  # noqa: E402
from test_adaptive_sequence_cpu import CASES  # noqa: E402
from test_weighted_cpu import SWITCHES, build_driver, host_accumulate_weighted, host_history_weight, weighted_case  # noqa: E402
from test_gpu_adaptive import _assert_exact, _mid_threshold  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(8, 8), (13, 17), (64, 64)]  # (H, W)
S0, CAP = 4, 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("weighted_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


# ---------------------------------------------------------------- 1. the kernels against the CPU build
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_weighted_device_equals_host_build(hip, tiny, driver, case, shape):
    H, W = shape
    args, opts, values = weighted_case(case, H, W)
    color, variance, motion, normal, count, prev_color, prev_variance, prev_depth, prev_len, prev_normal, prev_weight = args
    for nt, cc in SWITCHES:
        hist = dict(normal_test=nt, color_clamp=cc, **values)
        for cnt in (count, 4.0):
            a = list(args)
            a[4] = cnt
            got = tiny.temporal_accumulate_weighted(*a, **hist, **opts)
            want = host_accumulate_weighted(driver, hip, *a, history=hist, **opts)
            for k, name in enumerate(("color", "variance", "len", "flags", "weight")):
                if name == "flags":
                    assert np.array_equal(got[k], want[k]), (nt, cc, name)
                else:
                    assert bits_equal(got[k], want[k]), (nt, cc, name, int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum()))
        hw = tiny.history_weight(motion, prev_color, prev_depth, prev_len, prev_weight, normal, prev_normal, normal_test=nt,
                                 normal_min=values.get("normal_min", 0.0), **opts)
        assert bits_equal(hw, host_history_weight(driver, hip, motion, normal, prev_color, prev_depth, prev_len, prev_normal, prev_weight,
                                                  history=dict(normal_test=nt, normal_min=values.get("normal_min", 0.0)), **opts)), (nt, cc)
    # the normal arrays are not read without the test (null)
    a = list(args)
    a[3] = a[9] = None
    got = tiny.temporal_accumulate_weighted(*a, color_clamp=True, **opts)
    want = host_accumulate_weighted(driver, hip, *a, history=dict(color_clamp=1), **opts)
    assert all(bits_equal(got[k], want[k]) for k in (0, 1, 2, 4)) and np.array_equal(got[3], want[3])


# ---------------------------------------------------------------- 2. argument checks with a live scene
def test_argument_checks(hip, tiny):
    H = W = 8
    z3, z1, z4 = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W, 4), f32)
    good = np.full((H, W), 4, np.int32)
    out = tiny.temporal_accumulate_weighted(z3, z1, z4, None, good, z3, z1, z1, z1, None, z1)
    assert (out[4] == 4).all() and (out[2] == 1).all()
    for bad in (0, -1):
        c = good.copy()
        c[H - 1, W - 1] = bad
        with pytest.raises(hip.McptError) as e:
            tiny.temporal_accumulate_weighted(z3, z1, z4, None, c, z3, z1, z1, z1, None, z1)
        assert e.value.code == 1 and "count" in str(e.value)
    for u in (0.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(hip.McptError) as e:
            tiny.temporal_accumulate_weighted(z3, z1, z4, None, u, z3, z1, z1, z1, None, z1)
        assert e.value.code == 1 and "uniform_count" in str(e.value), u
    with pytest.raises(hip.McptError) as e:
        tiny.temporal_accumulate_weighted(z3, z1, z4, None, good, z3, z1, z1, z1, None, z1, normal_test=True)
    assert e.value.code == 1 and "normal" in str(e.value)
    for kw in (dict(max_history=4097), dict(depth_tol=-1.0)):
        with pytest.raises(hip.McptError) as e:
            tiny.temporal_accumulate_weighted(z3, z1, z4, None, good, z3, z1, z1, z1, None, z1, **kw)
        assert e.value.code == 1
        with pytest.raises(hip.McptError) as e:
            tiny.history_weight(z4, z3, z1, z1, z1, **kw)
        assert e.value.code == 1 and "mcpt_temporal_history_weight" in str(e.value)
    with pytest.raises(hip.McptError) as e:
        tiny.history_weight(z4, z3, z1, z1, z1, normal_test=True)
    assert e.value.code == 1 and "normal" in str(e.value)
    for mh in (-1, 4097):
        with pytest.raises(hip.McptError) as e:
            tiny.render_adaptive_weighted(2, 0.1, z1, max_history=mh, spp=4)
        assert e.value.code == 1 and "max_history" in str(e.value)
    with pytest.raises(hip.McptError) as e:
        tiny.render_adaptive_weighted(2, 0.1, z1, spp=6)
    assert e.value.code == 1 and "mcpt_render_adaptive_weighted" in str(e.value)


# ---------------------------------------------------------------- 3. the weight-guided adaptive frame
@pytest.fixture(scope="module")
def cornell(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(32, 32, CAP))
    _, _, e0, _, _ = hs.render_adaptive(S0, 1e30, spp=S0, seed=1)
    yield hs, _mid_threshold(e0, 0.5)
    hs.close()


def test_null_plane_is_render_adaptive_guided(cornell):
    hs, thr = cornell
    want = hs.render_adaptive_guided(S0, thr, None, spp=CAP, seed=1)
    for mh in (0, 1, 4096):
        got = hs.render_adaptive_weighted(S0, thr, None, max_history=mh, spp=CAP, seed=1)
        assert bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and bits_equal(got[2], want[2]) and bits_equal(got[3], want[3])
        assert got[4]["active_pixels"] == want[4]["active_pixels"] and got[5].samples == want[5].samples
    assert len(np.unique(want[1])) >= 2
    # a plane of weights that give no history is the plain rule too
    for plane in (np.zeros((32, 32), f32), np.full((32, 32), np.nan, f32), np.full((32, 32), -5, f32)):
        got = hs.render_adaptive_weighted(S0, thr, plane, spp=CAP, seed=1)
        assert bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and bits_equal(got[2], want[2])


def test_weight_guided_frame_never_samples_more_and_is_exact(cornell):
    hs, thr = cornell
    rng = np.random.default_rng(41)
    Hw = (rng.random((32, 32)) * 200 + 0.5).astype(f32)
    _, plain_spp, plain_err, _, _, _ = hs.render_adaptive_guided(S0, thr, None, spp=CAP, seed=1)
    fb, spp, err, var, info, st = hs.render_adaptive_weighted(S0, thr, Hw, spp=CAP, seed=1)
    assert (spp <= plain_spp).all() and (spp < plain_spp).any()
    levels = _assert_exact(hs, fb, spp, seed=1)
    assert len(levels) >= 2, levels
    assert int(spp.sum()) == st.samples
    same = spp == plain_spp
    assert np.array_equal(err[same], plain_err[same], equal_nan=True)  # err is the unscaled estimate


def test_round_zero_equals_the_frame_guide(cornell):
    """dilate 0 and H = (N - 1) S0: in round 0 weight_guide is ((N - 1) S0 + S0) / S0 = N exactly, the frame guide's factor, so the same
    pixels stop at S0."""
    hs, thr = cornell
    for N in (2, 5, 32):
        _, frames_spp, _, _, _, _ = hs.render_adaptive_guided(S0, thr, np.full((32, 32), N, f32), dilate=0, spp=CAP, seed=1)
        _, weight_spp, _, _, _, _ = hs.render_adaptive_weighted(S0, thr, np.full((32, 32), (N - 1) * S0, f32), dilate=0, spp=CAP, seed=1)
        assert np.array_equal(frames_spp == S0, weight_spp == S0), N
        assert (weight_spp >= frames_spp).all()  # later rounds: the weight guide tightens as n doubles, the frame guide does not
        if N == 2:
            assert (frames_spp == S0).any() and (frames_spp > S0).any()
