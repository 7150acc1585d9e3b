"""Filtered history without a GPU (include/mcpt.h: mcpt_feedback_opts, mcpt_denoise_feedback, mcpt_sequence_create_feedback,
mcpt_sequence_history): the host build of csrc/mcpt_denoise.h (tests/native/feedback_driver.cpp, g++ -ffp-contract=off) -- prep, k
iterations, dn::feedback_pixel -- gives the bits of a numpy float32 restatement (tests/feedback_cases.py); behind the last iteration the
feedback colour is the filter's output; on a flat noisy surface a history that is fed back is closer to the truth than one that is not; the
struct has the header's size and the calls refuse invalid options before they touch a device.  tests/test_gpu_feedback.py checks the
kernel against the host build bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feedback_cases import BAD, ITERATIONS, KS, SHAPES, build_driver, feedback_case, host_feedback, ref_feedback, same_bits  # noqa: E402
from test_denoise_cpu import BAD_OPTS, host_denoise  # noqa: E402
from test_denoise_cpu import build_driver as build_denoise_driver  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("feedback_cpu"))


@pytest.fixture(scope="module")
def denoise_driver(tmp_path_factory):
    return build_denoise_driver(tmp_path_factory.mktemp("feedback_dn"))


# ---------------------------------------------------------------- 1. the host build against the restatement
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_build_matches_the_float32_restatement(hip, driver, shape, k):
    H, W = shape
    for bad in BAD:
        color, variance, aov = feedback_case(H, W, bad)
        out, fc, fv, rec = host_feedback(driver, hip, color, variance, aov, k)
        want_out, want_fc, want_fv = ref_feedback(color, variance, aov, k)
        assert same_bits(fc, want_fc), (bad, int((fc.view(np.uint32) != want_fc.view(np.uint32)).sum()))
        assert same_bits(fv, want_fv), (bad, int((fv.view(np.uint32) != want_fv.view(np.uint32)).sum()))
        assert same_bits(out, want_out), bad
        # the rule itself on the host build's own records after iteration k
        A = np.where(aov[..., 0:3] > f32(1e-3), aov[..., 0:3], f32(1e-3)).astype(f32)
        la = (f32(0.2126) * A[..., 0] + f32(0.7152) * A[..., 1]) + f32(0.0722) * A[..., 2]
        ok = rec[..., 3] >= 0
        assert same_bits(fc, np.where(ok[..., None], rec[..., 0:3] * A, color))
        assert same_bits(fv, np.where(ok, rec[..., 3] * (la * la), variance))
        y, x = H // 2, W // 2
        if bad is not None:  # the unusable pixel passes colour and variance through with their bits
            assert not ok[y, x]
            assert same_bits(fc[y, x], color[y, x]) and same_bits(fv[y, x], variance[y, x]) and same_bits(out[y, x], color[y, x])
            if H * W > 1:
                assert ok.sum() == H * W - 1 and np.isfinite(fc[ok]).all() and np.isfinite(fv[ok]).all()
        else:
            assert ok.all() and (fv >= 0).all()
        # a null variance array: the colour alone, the same bits
        _, fc2, none, _ = host_feedback(driver, hip, color, variance, aov, k, want_variance=False)
        assert none is None and same_bits(fc2, fc)
    if H * W > 1:  # the iteration filters: the fed colour is neither the input nor (before the last iteration) the output
        assert not same_bits(fc, color)
    if (H, W) == (17, 33):  # (in 3 x 5 the later steps reach no neighbour on the same surface)
        assert same_bits(fc, out) == (k == ITERATIONS)


@pytest.mark.parametrize("opts", [dict(iterations=3, sigma_n=7.0, sigma_l=1.0), dict(iterations=8, sigma_n=1024.0, sigma_z=0.25)])
def test_host_build_matches_the_restatement_with_other_options(hip, driver, opts):
    color, variance, aov = feedback_case(17, 33, "nan")
    for k in (1, 2, opts["iterations"]):
        out, fc, fv, _ = host_feedback(driver, hip, color, variance, aov, k, **opts)
        o = dict(opts)
        o["sigma_n"] = int(o["sigma_n"])
        want_out, want_fc, want_fv = ref_feedback(color, variance, aov, k, **o)
        assert same_bits(fc, want_fc) and same_bits(fv, want_fv) and same_bits(out, want_out), k


# ---------------------------------------------------------------- 2. the last iteration is the output
@pytest.mark.parametrize("shape", SHAPES)
def test_last_iteration_equals_the_denoised_output(hip, driver, denoise_driver, shape):
    H, W = shape
    for bad in BAD:
        color, variance, aov = feedback_case(H, W, bad)
        full = host_denoise(denoise_driver, hip, color, variance, aov)
        for k in KS:
            out, fc, _, _ = host_feedback(driver, hip, color, variance, aov, k)
            assert same_bits(out, full), (bad, k)  # the feedback changes nothing of the filter
        assert same_bits(fc, full), bad
    # off: the filter alone, and the feedback arrays are untouched
    out, fc, fv, _ = host_feedback(driver, hip, color, variance, aov, 0)
    assert same_bits(out, full) and not fc.any() and not fv.any()


# ---------------------------------------------------------------- 3. the recurrence on a flat surface
TRUE, SIGMA, FRAMES, SEEDS = 0.25, 0.1, 8, (1, 2, 3, 4, 5)

# history RMSE with feedback 1 over without, after eight frames, measured with this test's own host builds for seeds 1..5 (DESIGN section
# 8m): 0.1850 0.1974 0.1887 0.2105 0.1906.  The bound is the worst of them plus their spread (0.2105 + 0.0255), and below 1 in any case.
RECURRENCE_BOUND = 0.236


def _flat_sequence(L, hip, seed, feedback):
    """Eight frames of a flat 32 x 32 plane (albedo 0.5, depth 10, normal (0,0,1), true colour 0.25) with i.i.d. noise of sigma 0.1 per
    channel, zero motion, through fb_accumulate and fb_denoise; the history is the fed colour and variance (feedback k > 0) or the
    accumulated ones.  Returns the RMSE of the last history and of the last denoised frame against the truth."""
    H = W = 32
    rng = np.random.default_rng(seed)
    aov = np.zeros((H, W, 8), f32)
    aov[..., 0:3], aov[..., 5], aov[..., 6], aov[..., 7] = 0.5, 1.0, 10.0, 1.0
    motion = np.zeros((H, W, 4), f32)
    motion[..., 2], motion[..., 3] = 10.0, 1.0
    depth = np.ascontiguousarray(aov[..., 6])
    wsum = f32(0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2)
    var = np.full((H, W), wsum * f32(SIGMA * SIGMA), f32)  # the luminance variance of a frame's colour, known
    hist, hvar, hlen = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
    to, do, fo = hip.temporal_opts(), hip.denoise_opts(), hip.FeedbackOpts(iteration=feedback)
    p = lambda a: a.ctypes.data  # noqa: E731
    for _ in range(FRAMES):
        frame = (TRUE + SIGMA * rng.standard_normal((H, W, 3))).astype(f32)
        acc, avar, alen = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
        assert L.fb_accumulate(W, H, p(frame), p(var), p(motion), p(hist), p(hvar), p(depth), p(hlen), C.addressof(to), p(acc), p(avar), p(alen)) == 0
        out, fc, fv = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
        assert L.fb_denoise(W, H, p(acc), p(avar), p(aov), C.addressof(do), C.addressof(fo), p(out), p(fc), p(fv), None) == 0
        hist, hvar, hlen = (fc, fv, alen) if feedback else (acc, avar, alen)
    assert (alen == FRAMES).all()
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - TRUE) ** 2)))  # noqa: E731
    return rmse(hist), rmse(out)


def test_feedback_compounds_on_a_flat_surface(hip, driver):
    ratios = []
    for seed in SEEDS:
        on, den_on = _flat_sequence(driver, hip, seed, 1)
        off, den_off = _flat_sequence(driver, hip, seed, 0)
        ratios.append(on / off)
        print("flat 32 x 32, sigma %.2f, %d frames, seed %d: history RMSE with feedback %.5f, without %.5f (sigma / sqrt(8) = %.5f), ratio %.4f; "
              "denoised RMSE %.5f against %.5f" % (SIGMA, FRAMES, seed, on, off, SIGMA / np.sqrt(FRAMES), on / off, den_on, den_off))
        assert abs(off / (SIGMA / np.sqrt(FRAMES)) - 1) < 0.1  # the control: the plain running mean of eight frames
    print("ratios %s, worst %.4f, spread %.4f" % (" ".join("%.4f" % r for r in ratios), max(ratios), max(ratios) - min(ratios)))
    assert RECURRENCE_BOUND < 1
    assert max(ratios) < RECURRENCE_BOUND


# ---------------------------------------------------------------- 4. the interface
def test_struct_size_and_header(hip):
    assert C.sizeof(hip.FeedbackOpts) == 32 and hip.FeedbackOpts.reserved.offset == 4
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "typedef struct { int32_t iteration; int32_t reserved[7]; } mcpt_feedback_opts;   /* 32 bytes; iteration 0 = off, else 1..8 */" in h
    for name in ("mcpt_denoise_feedback", "mcpt_sequence_create_feedback", "mcpt_sequence_history"):
        assert ("int %s(" % name) in h and name in hip.EXPORTS
    assert "The history stays unfiltered: the filter is an output, not a feedback --" in h and "dn::feedback_pixel" in h


def _fb(hip, iteration=1, word=None):
    o = hip.FeedbackOpts(iteration=iteration)
    if word is not None:
        o.reserved[word] = 1
    return o


def test_denoise_feedback_checks_come_before_any_device_call(hip):
    """Every refusal happens before the library touches a device (there is none on the machines that run this test) and before it reads the
    scene: the handle is not a scene."""
    L = hip.lib()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    W = H = 8
    buf = lambda n: C.cast((C.c_float * n)(), C.c_void_p)  # noqa: E731
    col, var, aov, out, fc, fv = buf(W * H * 3), buf(W * H), buf(W * H * 8), buf(W * H * 3), buf(W * H * 3), buf(W * H)

    def call(f, opts=None, scene=fake, w=W, h=H, c=col, v=var, a=aov, o=out, fcol=fc, fvar=fv, null_opts=False):
        d = opts if opts is not None else hip.denoise_opts()
        return L.mcpt_denoise_feedback(scene, w, h, c, v, a, None if null_opts else C.byref(d), None if f is None else C.byref(f), o, fcol, fvar)

    # everything mcpt_denoise refuses, with every setting of the switch
    for f in (None, _fb(hip, 0), _fb(hip, 1)):
        for kw in (dict(scene=None), dict(c=None), dict(v=None), dict(a=None), dict(o=None), dict(null_opts=True), dict(w=0), dict(h=-1)):
            assert call(f, **kw) == 1, kw
            assert b"mcpt_denoise_feedback" in L.mcpt_last_error()
        for kw in BAD_OPTS:
            assert call(f, opts=hip.denoise_opts(**kw)) == 1, kw
        bad = hip.denoise_opts()
        bad.reserved[1] = 1
        assert call(f, opts=bad) == 1
    # the iteration: outside 0..8, or above the resolved iterations (0 resolves to 5)
    for k in (-1, 9, 100, 6, 7, 8):
        assert call(_fb(hip, k)) == 1 and b"feedback" in L.mcpt_last_error(), k
    for it, k in ((1, 2), (3, 4), (7, 8)):
        assert call(_fb(hip, k), opts=hip.denoise_opts(iterations=it)) == 1, (it, k)
    for word in range(7):
        assert call(_fb(hip, 1, word)) == 1 and call(_fb(hip, 0, word)) == 1, word
        assert b"reserved" in L.mcpt_last_error()
    assert call(_fb(hip, 1), fcol=None) == 1 and b"feedback_color_host" in L.mcpt_last_error()


def test_sequence_feedback_checks_come_before_any_device_call(hip):
    L = hip.lib()
    fake = C.c_void_p(0x1000)
    W, H = 4, 3
    h = C.c_void_p()

    def create(f, filter=1, iterations=0, adaptive=None, weighted=None, moments=None, features=None, scene=fake, w=W, aov_spp=0):
        o = hip.SequenceOpts(filter=filter)
        o.denoise.iterations = iterations
        o.denoise.aov_spp = aov_spp
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        return L.mcpt_sequence_create_feedback(scene, w, H, C.byref(o), None, ref(adaptive), None, ref(weighted), ref(moments), ref(features),
                                               ref(f), C.byref(h))

    rule = hip.sequence_adaptive(min_spp=2, threshold=0.05)
    # everything mcpt_sequence_create_features refuses, with every setting of the switch
    for f in (None, _fb(hip, 0), _fb(hip, 1)):
        assert create(f, scene=None) == 1 and create(f, w=0) == 1
        assert create(f, aov_spp=-1) == 1 and create(f, aov_spp=65537) == 1
        assert create(f, iterations=9) == 1 and create(f, filter=2) == 1
        assert create(f, adaptive=rule, moments=hip.moments_opts()) == 1
        assert create(f, features=hip.FeatureOpts(centre=2)) == 1 and create(f, features=hip.FeatureOpts(centre=1), aov_spp=2) == 1
        assert b"mcpt_sequence_create" in L.mcpt_last_error()
    for k in (-1, 9, 100):
        assert create(_fb(hip, k)) == 1 and b"feedback" in L.mcpt_last_error(), k
    for word in range(7):
        assert create(_fb(hip, 1, word)) == 1 and create(_fb(hip, 0, word)) == 1, word
        assert b"reserved" in L.mcpt_last_error()
    for k in (1, 5):
        assert create(_fb(hip, k), filter=0) == 1 and b"filter" in L.mcpt_last_error(), k
    for it, k in ((0, 6), (1, 2), (3, 4), (7, 8)):
        assert create(_fb(hip, k), iterations=it) == 1 and b"feedback" in L.mcpt_last_error(), (it, k)
    assert create(_fb(hip, 1), adaptive=rule) == 1 and b"adaptive" in L.mcpt_last_error()
    assert create(_fb(hip, 1), weighted=hip.SequenceWeighted(weighted=1)) == 1 and b"weighted" in L.mcpt_last_error()
    assert h.value is None
    # mcpt_sequence_history
    col = (C.c_float * (W * H * 3))()
    assert L.mcpt_sequence_history(None, col, None) == 1 and b"mcpt_sequence_history" in L.mcpt_last_error()
    assert L.mcpt_sequence_history(fake, None, None) == 1
