"""Filtered history on the GPU (include/mcpt.h: mcpt_denoise_feedback, mcpt_sequence_create_feedback, mcpt_sequence_history):
k_dn_feedback gives the bits of the host build of dn::feedback_pixel and leaves the filter's output alone; a null or zeroed switch is
mcpt_denoise and mcpt_sequence_create_features; a feedback sequence is the composition of the separate calls with the previous frame's
feedback as prev_color and prev_variance, with propagated variance and with moments, under the host builder and under PLOC; refusals and
resets leave the fed history as they should; and what the feedback does to the error and the flicker of a one-sample sequence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feedback_cases import BAD, ITERATIONS, KS, SHAPES, build_driver, feedback_case, host_feedback, same_bits  # noqa: E402
from test_gpu_sequence import ALL, SHORT, translate  # noqa: E402
from test_temporal_cpu import bits_equal  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("feedback_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


# ---------------------------------------------------------------- 1. the device against the host build
@pytest.mark.parametrize("shape", SHAPES + [(64, 64)])  # (17 and 33 cross the 16 x 16 tiles and the 256-lane blocks)
def test_device_equals_host_build(hip, tiny, driver, shape):
    H, W = shape
    for bad in BAD:
        color, variance, aov = feedback_case(H, W, bad)
        plain = tiny.denoise(color, variance, aov)
        for k in KS:
            out, fc, fv = tiny.denoise_feedback(color, variance, aov, iteration=k)
            want_out, want_fc, want_fv, _ = host_feedback(driver, hip, color, variance, aov, k)
            assert same_bits(fc, want_fc), (bad, k, int((fc.view(np.uint32) != want_fc.view(np.uint32)).sum()))
            assert same_bits(fv, want_fv), (bad, k, int((fv.view(np.uint32) != want_fv.view(np.uint32)).sum()))
            assert same_bits(out, want_out) and same_bits(out, plain), (bad, k)
        assert same_bits(fc, plain)  # behind the last iteration the fed colour is the output
        if bad is not None:
            y, x = H // 2, W // 2
            assert same_bits(fc[y, x], color[y, x]) and same_bits(fv[y, x], variance[y, x])
    # other options, and the switch off: mcpt_denoise, the feedback arrays untouched
    o = dict(iterations=3, sigma_n=7.0, sigma_l=1.0)
    for k in (1, 3):
        out, fc, fv = tiny.denoise_feedback(color, variance, aov, iteration=k, **o)
        want_out, want_fc, want_fv, _ = host_feedback(driver, hip, color, variance, aov, k, **o)
        assert same_bits(fc, want_fc) and same_bits(fv, want_fv) and same_bits(out, want_out), k
    for f in ("null", hip.FeedbackOpts()):
        out, fc, fv = tiny.denoise_feedback(color, variance, aov, feedback=f)
        assert same_bits(out, plain) and not fc.any() and not fv.any()


# ---------------------------------------------------------------- 2. off is the parent
def test_null_or_zeroed_feedback_is_sequence_create_features(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    scenes = [hip.HipScene(sd) for _ in range(3)]
    kw = dict(filter=True, normal_test=True, color_clamp=True, moments=True, features=hip.FeatureOpts(centre=1))
    seqs = [hip.HipSequence(scenes[0], **kw), hip.HipSequence(scenes[1], feedback="null", **kw),
            hip.HipSequence(scenes[2], feedback=hip.FeedbackOpts(), **kw)]
    for k in range(6):
        rs = []
        for hs, s in zip(scenes, seqs):
            hs.update([(SHORT, translate(-32.0 * k, 0, 0))])
            rs.append(s.frame(want=ALL, spp=1, seed=k + 1))
        for r in rs[1:]:
            for key in ALL:
                assert np.array_equal(r[key].view(np.uint8), rs[0][key].view(np.uint8)), (k, key)
        for s in seqs[1:]:
            assert np.array_equal(s.flags(), seqs[0].flags()) and bits_equal(s.moments(), seqs[0].moments())
        # without feedback the history the next frame reads is the accumulated frame and its variance
        for s, r in zip(seqs, rs):
            hc, hv = s.history()
            assert bits_equal(hc, r["accumulated"]) and bits_equal(hv, r["variance"]), k
    assert rs[0]["len"].max() == 6 and (rs[0]["motion"][..., 0:2] != 0).any()
    for x in seqs + scenes:
        x.close()


# ---------------------------------------------------------------- 3. on is the separate-call loop
@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("kind", ["variance", "moments"])
def test_feedback_sequence_is_the_composition_of_the_calls(pkg, hip, kind, builder):
    """Six frames of Cornell 64 x 64 with the short box moved before each; the history of the separate calls is the previous frame's
    mcpt_denoise_feedback colour (and variance).  With the host builder the separate calls run on a second handle, with PLOC on the
    sequence's own handle before its frame (tests/test_gpu_sequence.py).
      variance  2 spp, the variance propagated through the blend, the normal test and the colour clamp on, feedback behind iteration 1;
      moments   1 spp with moments, centre features and specular motion at depth 2, both rejections on, feedback behind iteration 2."""
    H = W = 64
    sd = pkg.scenes.cornell_demo(W, H, 4)
    a = hip.HipScene(sd, builder=builder)
    b = a if builder == "ploc" else hip.HipScene(sd, builder=builder)
    rej = dict(normal_test=True, color_clamp=True)
    mom = kind == "moments"
    if mom:
        K, depth, spp = 2, 2, 1
        seq = a.sequence(filter=True, specular_depth=depth, specular_motion=True, moments=True, centre_features=True, feedback=K, **rej)
    else:
        K, depth, spp = 1, 0, 2
        seq = a.sequence(filter=True, aov_spp=2, feedback=K, **rej)
    hc, hv = seq.history(variance=not mom)
    assert not hc.any() and (mom or not hv.any())  # before the first frame everything is 0
    hist, length, moments = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W, 2), f32)
    hist_var, prev_depth, prev_normal = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    moved = fed_differs = False
    for k in range(6):
        b.snapshot()
        move = [(SHORT, translate(-32.0 * k, 0, 0))]
        info = b.update(move)
        assert info["path"] == (1 if builder == "ploc" else 0)
        if a is not b:
            a.update(move)
        if mom:
            aov = b.render_aovs(seed=k + 1, specular_depth=depth, centre=True)
            motion = b.render_motion(seed=k + 1, specular_depth=depth, centre=True)
            normal = np.ascontiguousarray(aov[..., 3:6])
            fb, _ = b.render(spp=spp, seed=k + 1)
            acc, acc_len, flags, moments = b.temporal_accumulate_moments(fb, motion, normal, hist, prev_depth, length, prev_normal, moments, **rej)
            acc_var = b.moments_variance(moments, acc_len, aov, flags=flags)
        else:
            aov = b.render_aovs(aov_spp=2, seed=k + 1)
            motion = b.render_motion(seed=k + 1, aov_spp=2)
            normal = np.ascontiguousarray(aov[..., 3:6])
            rd = b.render_denoised(spp=spp, seed=k + 1, aov_spp=2)
            fb = rd["fb"]
            acc, acc_var, acc_len, flags = b.temporal_accumulate_ex(fb, rd["variance"], motion, normal, hist, hist_var, prev_depth, length,
                                                                    prev_normal, **rej)
        den, fc, fv = b.denoise_feedback(acc, acc_var, aov, iteration=K)
        r = seq.frame(want=ALL, spp=spp, seed=k + 1)
        assert r["info"]["frame_index"] == k
        assert bits_equal(r["aov"], aov) and bits_equal(r["motion"], motion) and bits_equal(r["fb"], fb), k
        assert bits_equal(r["accumulated"], acc) and bits_equal(r["len"], acc_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        assert np.array_equal(seq.flags(), flags), k
        hc, hv = seq.history(variance=not mom)
        assert bits_equal(hc, fc), k
        if mom:
            assert bits_equal(seq.moments(), moments), k
            with pytest.raises(hip.McptError) as e:
                seq.history()
            assert e.value.code == 1 and "mcpt_sequence_history" in str(e.value)
        else:
            assert bits_equal(hv, fv), k
        moved |= bool((motion[..., 0:2] != 0).any())
        fed_differs |= not bits_equal(fc, acc)
        hist, length, hist_var, prev_depth, prev_normal = fc, acc_len, fv, aov[..., 6].copy(), normal
    assert moved and fed_differs and length.max() == 6
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 4. the fed history is safe
def test_refusals_and_resets(pkg, hip, tiny):
    for kw in (dict(feedback=hip.FeedbackOpts(iteration=9)), dict(feedback=hip.FeedbackOpts(iteration=1), filter=False),
               dict(feedback=hip.FeedbackOpts(iteration=3), iterations=2), dict(feedback=hip.FeedbackOpts(iteration=1), weighted=True),
               dict(feedback=hip.FeedbackOpts(iteration=1), adaptive=dict(min_spp=2, threshold=0.05))):
        with pytest.raises(hip.McptError) as e:
            hip.HipSequence(tiny, **kw)
        assert e.value.code == 1 and "mcpt_sequence_create" in str(e.value), kw
    seq = tiny.sequence(filter=True, aov_spp=2, feedback=1)
    r1 = seq.frame(want=ALL, spp=2, seed=1)
    seq.frame(want=("len",), spp=2, seed=2)
    hc, hv = seq.history()
    assert hc.any() and hv.any()
    other = pkg.scenes.make_camera(9, 8, 40, (278, 273, -800), (278, 273, 0))  # the wrong width
    for kw in (dict(camera=other, spp=2), dict(spp=0), dict(spp=2, nranks=2)):
        with pytest.raises(hip.McptError) as e:
            seq.frame(want=("len",), seed=3, **kw)
        assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value), kw
        c2, v2 = seq.history()
        assert bits_equal(c2, hc) and bits_equal(v2, hv), kw
    r3 = seq.frame(want=("len",), spp=2, seed=3)
    assert r3["info"]["frame_index"] == 2 and r3["len"].max() == 3  # the history went on from where it was
    # the first frame after a reset is the first frame of a fresh sequence: the fed planes are not read
    seq.reset()
    r = seq.frame(want=ALL, spp=2, seed=1)
    for key in ALL:
        assert np.array_equal(r[key].view(np.uint8), r1[key].view(np.uint8)), key
    got = seq.history()
    seq.close()  # (one sequence per scene at a time)
    fresh = tiny.sequence(filter=True, aov_spp=2, feedback=1)
    fresh.frame(want=("len",), spp=2, seed=1)
    for g, want in zip(got, fresh.history()):
        assert bits_equal(g, want)
    fresh.close()


# ---------------------------------------------------------------- 5. quality
def _tone(img):
    with np.errstate(invalid="ignore"):
        return np.clip(img.astype(np.float64), 0, 1) ** 0.45


def _rms(d):
    return float(np.sqrt(np.nanmean(d * d)))


def quality_figures(hs, ref, base, feedback):
    """Eight frames x 1 spp (seeds base+1 .. base+8) of a moments sequence on centre features: the tone-curve RMSE of the last denoised
    frame against ref, and the flicker: the RMS of the frame-to-frame differences of the tone-mapped denoised output over the last four
    frames (three differences)."""
    seq = hs.sequence(filter=True, moments=True, centre_features=True, feedback=feedback)
    last = []
    for k in range(8):
        r = seq.frame(want=("denoised",), spp=1, seed=base + k + 1)
        last = (last + [_tone(r["denoised"])])[-4:]
    seq.close()
    return _rms(last[-1] - _tone(ref)), _rms(np.stack([last[i + 1] - last[i] for i in range(3)]))


# Measured on the MI355X over five seed sets (seeds b+1..b+8, b = 0, 100, 200, 300, 400), feedback 1 over no feedback:
#   RMSE    0.9318 0.9277 0.9296 0.9173 0.9291   (0.0672 against 0.0722 for seeds 1..8)
#   flicker 0.9363 0.9343 0.9277 0.9297 0.9298   (0.0291 against 0.0310)
# Each bound is the worst of its five plus their spread (0.9318 + 0.0145, 0.9363 + 0.0086), and below 1 in any case.
RMSE_BOUND = 0.9463
FLICKER_BOUND = 0.9449


def test_feedback_quality_at_one_sample(pkg, hip):
    """Static Cornell demo 96 x 96 against a 4096-spp render of another seed (the protocol of tests/test_gpu_sequence_moments.py); the same
    sequence without feedback is the yardstick."""
    W = H = 96
    hs = hip.HipScene(pkg.scenes.cornell_demo(W, H, 4))
    ref, _ = hs.render(spp=4096, seed=99)
    on, off = quality_figures(hs, ref, 0, 1), quality_figures(hs, ref, 0, 0)
    print("8 frames x 1 spp, feedback 1 against none: tone-curve RMSE %.5f / %.5f = %.4f, flicker %.5f / %.5f = %.4f"
          % (on[0], off[0], on[0] / off[0], on[1], off[1], on[1] / off[1]))
    assert on[0] / off[0] < RMSE_BOUND
    assert on[1] / off[1] < FLICKER_BOUND
    hs.close()
