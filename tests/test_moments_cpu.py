"""Temporal luminance moments without a GPU (include/mcpt.h: mcpt_moments_opts, mcpt_temporal_accumulate_moments, mcpt_moments_variance,
mcpt_sequence_create_moments, mcpt_sequence_moments): the ctypes struct has the header's layout; the host compilation of the kMoments
flavour of tp::reuse_pixel and of mo::variance_pixel (tests/native/moments_driver.cpp, g++ -ffp-contract=off) follows the rules of
include/mcpt.h -- numpy float32 restatements in the header's order, bit for bit; the colour, the length and the flags are those of the host
build of tp::accumulate_pixel_ex; the two estimators are calibrated against noise of known variance; no window crosses a seam; values that
are not finite stay where they are; every entry point refuses invalid arguments before it touches a device; and a stand-alone program
(tests/native/moments_main.cpp) runs the same headers under AddressSanitizer and UBSan.  tests/test_gpu_moments.py checks that the kernels
give the host build's bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moments_cases as mc  # noqa: E402
from test_history_cpu import build_driver as build_history_driver, host_accumulate_ex  # noqa: E402

ROOT = mc.ROOT
f32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return mc.build_driver(tmp_path_factory.mktemp("moments_cpu"))


@pytest.fixture(scope="module")
def history_driver(tmp_path_factory):
    return build_history_driver(tmp_path_factory.mktemp("moments_hist_cpu"))


def test_struct_layout_and_header(hip):
    T = hip.MomentsOpts
    assert C.sizeof(T) == 32
    assert (T.enabled.offset, T.min_len.offset, T.radius.offset, T.sigma_z.offset, T.reserved.offset, T.reserved.size) == (0, 4, 8, 12, 16, 16)
    assert bytes(hip.MomentsOpts()) == bytes(32)
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    for text in ("} mcpt_moments_opts;     /* 32 bytes */", "q = mu2 - mu1*mu1;   q = q > 0 ? q : 0;   v = q / (N - 1.f)", "sig2 = q * (cnt / (cnt - 1.f))",
                 "v = sig2 / (clamped ? 1.f : N)", "out_mu1 = hm1 + (m1 - hm1) * k"):
        assert text in h, text
    for name in ("mcpt_temporal_accumulate_moments", "mcpt_moments_variance", "mcpt_sequence_create_moments", "mcpt_sequence_moments"):
        assert ("int %s(" % name) in h and name in hip.EXPORTS
    L = hip.lib()
    for name in ("mcpt_temporal_accumulate_moments", "mcpt_moments_variance", "mcpt_sequence_create_moments", "mcpt_sequence_moments"):
        assert getattr(L, name) is not None


def test_option_defaults_and_ranges_host_build(hip, driver):
    ints, vals = (C.c_int * 2)(), (C.c_float * 1)()

    def resolve(o):
        return driver.mo_resolve(C.addressof(o), ints, vals)

    assert resolve(hip.MomentsOpts()) == 0 and (ints[0], ints[1], vals[0]) == (4, 3, 1.0)
    assert resolve(hip.moments_opts(True, 2, 1, 0.25)) == 0 and (ints[0], ints[1], vals[0]) == (2, 1, 0.25)
    assert resolve(hip.moments_opts(True, 4096, 4, 3.0)) == 0 and (ints[0], ints[1]) == (4096, 4)
    for kw in (dict(min_len=1), dict(min_len=-1), dict(min_len=4097), dict(radius=5), dict(radius=-1), dict(sigma_z=-1.0),
               dict(sigma_z=float("nan")), dict(sigma_z=float("inf"))):
        assert resolve(hip.moments_opts(True, **kw)) == 1, kw
    for e in (2, -1):
        o = hip.moments_opts()
        o.enabled = e
        assert resolve(o) == 1, e
    for k in range(4):
        o = hip.moments_opts()
        o.reserved[k] = 1
        assert resolve(o) == 1, k


@pytest.mark.parametrize("window", mc.WINDOWS)
@pytest.mark.parametrize("switches", mc.SWITCHES)
@pytest.mark.parametrize("shape", mc.SHAPES)
def test_host_build_equals_numpy(hip, driver, history_driver, shape, switches, window):
    """1. and 2.: both rules against their restatements, bit for bit; colour, length and flags against the host build of accumulate_pixel_ex."""
    H, W = shape
    min_len, radius = window
    args, history, aov = mc.frame_case(H, W, switches)
    got = mc.host_accumulate(driver, hip, *args, history=history, max_history=8)
    want = mc.numpy_accumulate(*args, max_history=8, **{k: (int(v) if isinstance(v, bool) else v) for k, v in history.items()})
    assert mc.bits_equal(got[0], want[0]) and mc.bits_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert mc.bits_equal(got[3], want[3]), int((got[3].view(np.uint32) != want[3].view(np.uint32)).sum())
    # the case does what it is for: history taken and refused, taps outside, holes, both sides of min_len
    assert (got[1] > 1).any() and (got[1] == 1).any() and (got[1] >= min_len).any() and ((got[1] > 1) & (got[1] < 4)).any()
    # 2. the colour rule is untouched: accumulate_pixel_ex on the same inputs, with variances it alone reads
    color, motion, normal, prev_color, prev_depth, prev_len, prev_normal, prev_moments = args
    rng = np.random.default_rng(7)
    var, pvar = rng.random((H, W)).astype(f32), rng.random((H, W)).astype(f32)
    ex = host_accumulate_ex(history_driver, hip, color, var, motion, normal, prev_color, pvar, prev_depth, prev_len, prev_normal, history=history,
                            max_history=8)
    assert mc.bits_equal(got[0], ex[0]) and mc.bits_equal(got[1], ex[2]) and np.array_equal(got[2], ex[3])
    if switches[1]:
        assert (got[2] & 2).any()
    # 1b. the variance from what the accumulation left
    for flags in (got[2], None):
        v = mc.host_variance(driver, hip, got[3], got[1], flags, aov, min_len=min_len, radius=radius)
        assert mc.bits_equal(v, mc.numpy_variance(got[3], got[1], flags, aov, min_len=min_len, radius=radius))
    assert np.isinf(v[H // 2, W // 3])  # (the pixel with the NaN colour)
    assert np.isfinite(np.delete(v.reshape(-1), (H // 2) * W + W // 3)).all() and (v >= 0).all()


def _identity_motion(H, W, depth=5.0):
    motion = np.zeros((H, W, 4), f32)
    motion[..., 2] = depth
    motion[..., 3] = 1
    return motion


def _run_static(driver, hip, frames, max_history=32, history=None):
    """A static sequence through the host build: yields (out, len, flags, moments) after each frame."""
    H, W = frames[0].shape[:2]
    motion, depth = _identity_motion(H, W), np.full((H, W), 5, f32)
    pc, pn, pm = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W, 2), f32)
    for c in frames:
        out = mc.host_accumulate(driver, hip, c, motion, None, pc, depth, pn, None, pm, history=history, max_history=max_history)
        pc, pn, pm = out[0], out[1], out[3]
        yield out


def _colour_of_short_luminance():
    """A colour (0, g, 0) whose float32 luminance 0.7152f * g is k / 16 exactly, and that luminance: the first k in 8..15 some float g near
    (k / 16) / 0.7152 reaches (the products step by more than an ulp of the target, so not every k is reached)."""
    for k in range(8, 16):
        target = f32(k) / f32(16)
        g = f32(target / f32(0.7152))
        for _ in range(8):
            g = np.nextafter(g, f32(0), dtype=f32)
        for _ in range(17):
            if f32(f32(0.7152) * g) == target:
                c = np.array([0, g, 0], f32)
                assert mc.lum(c) == target
                return c, target
            g = np.nextafter(g, f32(2), dtype=f32)
    raise AssertionError("no float32 g with 0.7152f * g == k / 16")


def test_constant_frames_have_zero_variance(hip, driver):
    """3. A constant sequence gives v == 0 exactly at every length, on both branches.  The colour's luminance is a multiple of 1/16 exactly, so that every
    window sum is exact (k * l and k * l * l for k <= 49 are floats): with a luminance of full precision the window means round, and the
    spatial branch leaves a residue of an ulp or so of l^2, as any float estimator of this form does.  On the temporal branch the zero is
    exact for every colour: fl(l*l) - fl(l*l)."""
    H, W = 9, 11
    aov = mc.flat_aov(H, W)
    aov[2:4, 3:6, 7] = 0                          # an uncovered block,
    aov[6:, :, 3:6] = np.array([1, 0, 0], f32)    # a crease,
    aov[..., 6] += np.where(np.arange(W) >= 7, f32(3), f32(0))  # and a depth step: every pixel still has company in its window
    c, l = _colour_of_short_luminance()
    exact = np.broadcast_to(c, (H, W, 3)).copy()
    for n, out in enumerate(_run_static(driver, hip, [exact] * 7, max_history=5), 1):
        assert (out[1] == min(n, 5)).all()
        assert (out[3][..., 0] == l).all() and (out[3][..., 1] == l * l).all()
        for min_len in (2, 4):
            v = mc.host_variance(driver, hip, out[3], out[1], None, aov, min_len=min_len, radius=3)
            assert (v == 0).all(), (n, min_len)
    grey = np.full((H, W, 3), 0.37, f32)
    for n, out in enumerate(_run_static(driver, hip, [grey] * 6), 1):
        if n >= 2:
            v = mc.host_variance(driver, hip, out[3], out[1], None, aov, min_len=2, radius=1)
            assert (v == 0).all(), n


def test_temporal_calibration(hip, driver):
    """4. 64 x 64, static, 8 frames of grey noise x ~ N(0.5, 0.1^2), iid per pixel and frame: after frame 8 (min_len 4, max_history 32) every
    pixel is on the temporal branch and the mean of v is within 5 % of 0.01 / 8.  The estimator q N / (N - 1) / N is unbiased; one pixel's
    relative deviation is sqrt(2 / 7), so the mean over 4096 pixels deviates by 0.8 %: 5 % is six deviations."""
    H = W = 64
    rng = np.random.default_rng(20171)
    frames = [mc.noise_moments(H, W, rng)[1] for _ in range(8)]
    out = list(_run_static(driver, hip, frames, max_history=32))[-1]
    assert (out[1] == 8).all()
    v = mc.host_variance(driver, hip, out[3], out[1], None, mc.flat_aov(H, W), min_len=4, radius=3)
    mean = float(v.astype(np.float64).mean())
    print("temporal calibration: mean v %.6e, expected %.6e, ratio %.4f" % (mean, 0.01 / 8, mean / (0.01 / 8)))
    assert abs(mean / (0.01 / 8) - 1) < 0.05


def test_spatial_calibration(hip, driver):
    """5. 128 x 128, one frame of the same noise (N = 1 everywhere), a flat plane, radius 3: the mean of v over the pixels at least 3 from
    the border is within 5 % of 0.01.  The Bessel factor 49 / 48 makes the estimator unbiased; about (122 / 7)^2 windows are independent and
    each deviates by sqrt(2 / 48): 1.2 %."""
    H = W = 128
    mom, _ = mc.noise_moments(H, W, np.random.default_rng(20172))
    v = mc.host_variance(driver, hip, mom, np.ones((H, W), f32), None, mc.flat_aov(H, W), min_len=4, radius=3)
    mean = float(v[3:-3, 3:-3].astype(np.float64).mean())
    print("spatial calibration: mean v %.6e, expected 1e-2, ratio %.4f" % (mean, mean / 0.01))
    assert abs(mean / 0.01 - 1) < 0.05


@pytest.mark.parametrize("radius", [1, 3])
def test_no_window_crosses_a_seam(hip, driver, radius):
    """6. Changing every moment on the far side of a coverage seam, a seam of orthogonal normals or a depth step larger than the gate leaves
    the near side's v bit for bit; a pixel whose window has no other member gets its second moment."""
    H, W = 10, 14
    rng = np.random.default_rng(61)
    mom, _ = mc.noise_moments(H, W, rng)
    other, _ = mc.noise_moments(H, W, rng)
    length = np.ones((H, W), f32)
    for name, aov, near in mc.seam_cases(H, W):
        sz = 0.1 if name == "depth" else 0.0  # (|grad| is 2 beside the step of 4: 0.1 * 2 * 3 + 0.009 stays below it)
        v0 = mc.host_variance(driver, hip, mom, length, None, aov, min_len=4, radius=radius, sigma_z=sz)
        changed = np.where(near[..., None], mom, other * f32(3))
        v1 = mc.host_variance(driver, hip, changed, length, None, aov, min_len=4, radius=radius, sigma_z=sz)
        assert mc.bits_equal(v0[near], v1[near]), name
        assert not mc.bits_equal(v0[~near], v1[~near]), name
        if name == "lone":
            assert mc.bits_equal(v0[near], mom[near][:, 1])
        else:
            assert (v0[near] != mom[near][:, 1]).all(), name  # (every near pixel has company)


def test_values_that_are_not_finite(hip, driver):
    """7. A stored moment that is not finite on a used tap restarts that pixel's moments; a neighbour whose moments are not finite is left
    out of windows; a pixel whose colour is not finite gets a v that is not finite and disturbs no neighbour; a clamped pixel takes the
    spatial branch with divisor 1.  What a restart does not do is move the pixel to the spatial branch by itself: colour, len and flags are
    mcpt_temporal_accumulate_ex's bit for bit, so nothing tells mcpt_moments_variance that the moments are one frame old, and the rule
    sends a pixel with finite moments and N >= min_len to the temporal branch, where (l, l*l) gives 0.  Part a pins that: the restarted
    pixel is on the spatial branch while N < min_len and gets exactly 0 from the temporal branch otherwise (it takes a
    luminance whose square overflows to get there)."""
    H, W = 8, 9
    rng = np.random.default_rng(71)
    frames = [mc.noise_moments(H, W, rng)[1] for _ in range(5)]
    outs = list(_run_static(driver, hip, frames))
    out, length, _, mom = outs[-2]
    assert (length == 4).all()
    # a. the restart: identity motion, so pixel (2, 3) reads the one tap (2, 3)
    motion, depth = _identity_motion(H, W), np.full((H, W), 5, f32)
    for bad in (np.nan, np.inf, -np.inf):
        for ch in (0, 1):
            pm = mom.copy()
            pm[2, 3, ch] = bad
            got = mc.host_accumulate(driver, hip, frames[-1], motion, None, out, depth, length, None, pm, max_history=32)
            ref = outs[-1]
            l = mc.lum(frames[-1])
            assert mc.bits_equal(got[3][2, 3], np.array([l[2, 3], l[2, 3] * l[2, 3]], f32))
            keep = np.ones((H, W), bool)
            keep[2, 3] = False
            assert mc.bits_equal(got[3][keep], ref[3][keep])
            assert mc.bits_equal(got[0], ref[0]) and mc.bits_equal(got[1], ref[1])  # (colour and length do not see the moments)
            assert mc.bits_equal(got[3], mc.numpy_accumulate(frames[-1], motion, None, out, depth, length, None, pm, max_history=32)[3])
            aov0 = mc.flat_aov(H, W)
            v_long = mc.host_variance(driver, hip, got[3], got[1], None, aov0, min_len=8, radius=1)  # N = 5 < 8: the spatial branch
            v_short = mc.host_variance(driver, hip, got[3], got[1], None, aov0, min_len=4, radius=1)
            assert got[1][2, 3] == 5 and v_long[2, 3] > 0 and v_short[2, 3] == 0
            assert mc.bits_equal(v_long, mc.numpy_variance(got[3], got[1], None, aov0, min_len=8, radius=1))
    # b. a neighbour that is not finite is left out: the window of (4, 4) without (4, 5) is the window with it uncounted
    aov = mc.flat_aov(H, W)
    short = np.ones((H, W), f32)
    pm = mom.copy()
    pm[4, 5, 1] = np.inf
    v = mc.host_variance(driver, hip, pm, short, None, aov, min_len=4, radius=1)
    assert np.isinf(v[4, 5]) and np.isfinite(np.delete(v.reshape(-1), 4 * W + 5)).all()
    win = [(y, x) for y in (3, 4, 5) for x in (3, 4, 5) if (y, x) != (4, 5)]
    s1 = s2 = f32(0)
    for y, x in win:
        s1, s2 = f32(s1 + mom[y, x, 0]), f32(s2 + mom[y, x, 1])
    a, b = f32(s1 / f32(8)), f32(s2 / f32(8))
    q = f32(b - f32(a * a))
    assert v[4, 4] == f32(max(q, f32(0)) * f32(f32(8) / f32(7)))
    assert mc.bits_equal(v, mc.numpy_variance(pm, short, None, aov, min_len=4, radius=1))
    far = np.ones((H, W), bool)
    far[3:6, 4:7] = False
    assert mc.bits_equal(v[far], mc.host_variance(driver, hip, mom, short, None, aov, min_len=4, radius=1)[far])
    # c. a colour that is not finite: its moments and its v are not finite, no neighbour's changes
    for bad in (np.nan, np.inf):
        c = frames[-1].copy()
        c[5, 2, 1] = bad
        got = mc.host_accumulate(driver, hip, c, motion, None, out, depth, length, None, mom, max_history=32)
        assert not np.isfinite(got[3][5, 2]).any() and got[1][5, 2] == 1
        for min_len in (2, 8):  # (the neighbours on the temporal branch, then on the spatial one)
            v = mc.host_variance(driver, hip, got[3], got[1], None, aov, min_len=min_len, radius=3)
            assert np.isinf(v[5, 2]) and v[5, 2] > 0
            clean = mc.host_variance(driver, hip, outs[-1][3], got[1], None, aov, min_len=min_len, radius=3)
            keep = np.ones((H, W), bool)
            keep[5, 2] = False
            if min_len == 2:
                assert mc.bits_equal(v[keep], clean[keep])
            assert np.isfinite(v[keep]).all()
            assert mc.bits_equal(v, mc.numpy_variance(got[3], got[1], None, aov, min_len=min_len, radius=3))
    # d. a clamped pixel: the spatial branch, divided by 1 and not by N
    length5, mom5 = outs[-1][1], outs[-1][3]
    flags = np.zeros((H, W), np.uint8)
    flags[3, 3] = 2
    flags[6, 6] = 1  # (the normal-test bit alone changes nothing)
    v = mc.host_variance(driver, hip, mom5, length5, flags, aov, min_len=4, radius=1)
    plain = mc.host_variance(driver, hip, mom5, length5, None, aov, min_len=4, radius=1)
    spatial = mc.host_variance(driver, hip, mom5, np.ones((H, W), f32), None, aov, min_len=4, radius=1)
    assert v[3, 3] == spatial[3, 3] and v[3, 3] != plain[3, 3]
    flags[3, 3] = 0
    flags[6, 6] = 0
    keep = np.ones((H, W), bool)
    keep[3, 3] = False
    assert mc.bits_equal(v[keep], plain[keep])
    short5 = np.full((H, W), 3, f32)  # a short history that is not clamped: the same sig2 over N
    assert mc.host_variance(driver, hip, mom5, short5, None, aov, min_len=4, radius=1)[3, 3] == f32(spatial[3, 3] / f32(3))


def test_argument_checks_come_before_any_device_call(pkg, hip):
    """8. Every refusal below happens before the library touches a device (there is none on the machines that run this test) and before it
    reads the scene: the handle is not a scene and not mapped memory."""
    L = hip.lib()
    fake = C.c_void_p(0x1000)
    W, H = 4, 3
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    col, mo, nrm = np.zeros((H, W, 3), f32), np.zeros((H, W, 4), f32), np.zeros((H, W, 3), f32)
    pc, z, n, pn, pm = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32), np.zeros((H, W, 2), f32)
    out, out_len, flags, out_m = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), np.uint8), np.zeros((H, W, 2), f32)
    aov, out_v = np.zeros((H, W, 8), f32), np.zeros((H, W), f32)
    ok, on = hip.temporal_opts(), hip.history_opts(True, True)
    # ---- mcpt_temporal_accumulate_moments: 0 scene, 1 W, 2 H, 3 color, 4 motion, 5 normal, 6 prev_color, 7 prev_depth, 8 prev_len,
    # 9 prev_normal, 10 prev_moments, 11 opts, 12 history_opts, 13 out_color, 14 out_len, 15 out_flags, 16 out_moments
    full = [fake, W, H, p(col), p(mo), p(nrm), p(pc), p(z), p(n), p(pn), p(pm), C.byref(ok), C.byref(on), p(out), p(out_len), p(flags), p(out_m)]
    acc = L.mcpt_temporal_accumulate_moments
    for k in (0, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 16):
        args = list(full)
        args[k] = None
        assert acc(*args) == 1, k
        assert b"mcpt_temporal_accumulate_moments" in L.mcpt_last_error()
    for k in (5, 9):
        args = list(full)
        args[k] = None
        assert acc(*args) == 1 and b"normal" in L.mcpt_last_error(), k
    for w, h in ((0, H), (W, 0), (-1, H), (1 << 15, 1 << 15)):
        args = list(full)
        args[1], args[2] = w, h
        assert acc(*args) == 1, (w, h)
    for kw in (dict(max_history=-1), dict(max_history=4097), dict(depth_tol=-1.0), dict(depth_tol=float("nan"))):
        args = list(full)
        o = hip.temporal_opts(**kw)
        args[11] = C.byref(o)
        assert acc(*args) == 1, kw
    for kw in (dict(normal_test=2), dict(color_clamp=-1), dict(normal_min=1.5), dict(clamp_k=float("nan"))):
        args = list(full)
        o = hip.history_opts(**kw)
        args[12] = C.byref(o)
        assert acc(*args) == 1, kw

    # ---- mcpt_moments_variance: 0 scene, 1 W, 2 H, 3 moments, 4 len, 5 flags (nullable), 6 aov, 7 opts, 8 out
    good = hip.moments_opts()
    full = [fake, W, H, p(pm), p(n), p(flags), p(aov), C.byref(good), p(out_v)]
    fn = L.mcpt_moments_variance
    for k in (0, 3, 4, 6, 7, 8):
        args = list(full)
        args[k] = None
        assert fn(*args) == 1, k
        assert b"mcpt_moments_variance" in L.mcpt_last_error()
    for w, h in ((0, H), (W, 0), (-1, H), (1 << 15, 1 << 15)):
        args = list(full)
        args[1], args[2] = w, h
        assert fn(*args) == 1, (w, h)

    def bad_moments():
        for kw in (dict(min_len=1), dict(min_len=-4), dict(min_len=4097), dict(radius=5), dict(radius=-1), dict(sigma_z=-0.5),
                   dict(sigma_z=float("nan")), dict(sigma_z=float("inf"))):
            yield hip.moments_opts(True, **kw)
        for e in (2, -1):
            o = hip.moments_opts()
            o.enabled = e
            yield o
        for k in range(4):
            o = hip.moments_opts()
            o.reserved[k] = 1
            yield o

    for o in bad_moments():
        args = list(full)
        args[7] = C.byref(o)
        assert fn(*args) == 1 and b"option" in L.mcpt_last_error()

    # ---- mcpt_sequence_create_moments: every refusal of mcpt_sequence_create_weighted, the options, and the combinations
    h = C.c_void_p()

    def create(o, md, ho=on, ad=None, mo_=None, wd=None, scene=fake, w=W, hh=H, outp=h):
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        return L.mcpt_sequence_create_moments(scene, w, hh, ref(o), ref(ho), ref(ad), ref(mo_), ref(wd), ref(md), ref(outp))

    seq_ok = hip.SequenceOpts(filter=1)
    for md in (None, hip.MomentsOpts(), hip.moments_opts(), hip.moments_opts(True, 2, 1, 0.5)):
        assert create(seq_ok, md, scene=None) == 1 and b"mcpt_sequence_create" in L.mcpt_last_error()
        assert create(None, md) == 1 and create(seq_ok, md, outp=None) == 1
        assert create(seq_ok, md, w=0) == 1 and create(seq_ok, md, hh=0) == 1 and create(seq_ok, md, w=1 << 15, hh=1 << 15) == 1
        assert create(hip.SequenceOpts(filter=2), md) == 1
        bad_t = hip.SequenceOpts(filter=1)
        bad_t.temporal.max_history = 4097
        assert create(bad_t, md) == 1
        bad_d = hip.SequenceOpts(filter=1)
        bad_d.denoise.iterations = 9
        assert create(bad_d, md) == 1
        assert create(seq_ok, md, ho=hip.history_opts(normal_test=2)) == 1
        assert create(seq_ok, md, ad=hip.sequence_adaptive(1, 0.1)) == 1
        assert create(seq_ok, md, mo_=hip.SequenceMotion(specular_motion=2)) == 1
        assert create(seq_ok, md, wd=hip.SequenceWeighted(weighted=2)) == 1
    for o in bad_moments():
        assert create(seq_ok, o) == 1 and b"moments" in L.mcpt_last_error()
    # out-of-range options are refused with the switch off too
    assert create(seq_ok, hip.moments_opts(False, radius=9)) == 1
    # enabled 1 with an adaptive rule, or with weighted 1
    on_ = hip.moments_opts()
    assert create(seq_ok, on_, ad=hip.sequence_adaptive(4, 0.1)) == 1 and b"adaptive" in L.mcpt_last_error()
    assert create(seq_ok, on_, ad=hip.sequence_adaptive(2, 0.1, guided=True)) == 1
    assert create(seq_ok, on_, wd=hip.SequenceWeighted(weighted=1)) == 1 and b"weighted" in L.mcpt_last_error()
    assert h.value is None
    # mcpt_sequence_moments: null arguments (a sequence without moments needs a device to exist: tests/test_gpu_sequence_moments.py)
    assert L.mcpt_sequence_moments(None, p(out_m)) == 1 and b"mcpt_sequence_moments" in L.mcpt_last_error()
    assert L.mcpt_sequence_moments(fake, None) == 1


def _sanitizer_runtime_present(tmp):
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    exe = os.path.join(tmp, "probe")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_sanitizer_program(tmp_path):
    """9. tests/native/moments_main.cpp, a program of its own, under AddressSanitizer and UBSan: the host build of both rules over the frame
    shapes of the tests on exactly-sized heap arrays, with huge, infinite and NaN motions, moments that are not finite, clamped pixels,
    coverage seams and every window radius.  Nothing is loaded into this process."""
    tmp = str(tmp_path)
    if not _sanitizer_runtime_present(tmp):
        pytest.skip("g++ cannot link an AddressSanitizer / UBSan program here")
    exe = os.path.join(tmp, "moments_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", mc.CSRC,
                           os.path.join(ROOT, "tests", "native", "moments_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 17, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
