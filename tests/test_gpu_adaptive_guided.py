"""Guided adaptive frames on the GPU (include/mcpt.h: mcpt_temporal_history_len, mcpt_render_adaptive_guided,
mcpt_render_adaptive_denoised): k_history_len gives the bits of the CPU build of tp::history_len_pixel; the guided counts and estimates
follow a numpy float64 restatement of the rule with per-pixel thresholds, from per-sample renders, and never exceed the unguided ones; every
pixel of a guided frame equals a plain render at its count; a null or all-ones guide is mcpt_render_adaptive; the variance of an adaptive
frame is step 2 of mcpt_render_denoised at each pixel's own count; the denoised adaptive frame is the composition of the separate calls;
and the host executable writes the frames the library call gives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import SHAPES, bits_equal  # noqa: E402
from test_adaptive_sequence_cpu import CASES, build_driver, guide_args, host_history_len  # noqa: E402
from test_gpu_adaptive import HOST, MODELS, _assert_exact, _estimate, _mid_threshold, _samples  # noqa: E402
from test_gpu_denoise import _ulps  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
GUIDE_VALUES = np.array([np.nan, 0, 1, 2, 5, 32, 4096], f32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("guide_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


def tiled_guide(H, W):
    """GUIDE_VALUES tiled over the frame in pixel order (7 is coprime to the widths used, so every row and column sees every value)."""
    return np.resize(GUIDE_VALUES, H * W).reshape(H, W).copy()


# ---------------------------------------------------------------- 1. the kernel against the CPU build
@pytest.mark.parametrize("shape", SHAPES + [(64, 64)])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_history_len_device_equals_host_build(hip, tiny, driver, case, shape):
    H, W = shape
    args, opts, values = case[1](H, W)
    motion, normal, prev_color, prev_depth, prev_len, prev_normal = guide_args(args)
    for nt in (0, 1):
        nm = values.get("normal_min", 0.0)
        got = tiny.history_len(motion, prev_color, prev_depth, prev_len, normal, prev_normal, normal_test=nt, normal_min=nm, **opts)
        want = host_history_len(driver, hip, motion, normal, prev_color, prev_depth, prev_len, prev_normal, history=dict(normal_test=nt, normal_min=nm),
                                **opts)
        assert bits_equal(got, want), (nt, int((got != want).sum()))
    # the normal arrays are not read without the test (null)
    assert bits_equal(tiny.history_len(motion, prev_color, prev_depth, prev_len, **opts),
                      host_history_len(driver, hip, motion, None, prev_color, prev_depth, prev_len, None, history=None, **opts))


# ---------------------------------------------------------------- 2. guided counts against numpy
def _expected_counts_guided(V, S0, smax, thr, rel_floor, dilate, guide=None):
    """test_gpu_adaptive._expected_counts with per-pixel thresholds: thr * sqrt(g) in float64, g = guide where guide >= 1, else 1.
    Returns (spp, err, the estimates evaluated, the thresholds they were compared with)."""
    V64 = V.astype(np.float64)
    c1, c2 = np.cumsum(V64, axis=0), np.cumsum(V64 * V64, axis=0)  # (sequential: sample order)
    H, W = V.shape[1:3]
    with np.errstate(invalid="ignore"):
        g = np.ones((H, W), np.float64) if guide is None else np.where(guide >= 1, guide, f32(1)).astype(np.float64)
    thr_px = np.float64(f32(thr)) * np.sqrt(g)
    spp = np.zeros((H, W), np.int64)
    err = np.zeros((H, W), f32)
    active = np.ones((H, W), bool)
    n, evaluated, compared = S0, [], []
    while True:
        e = _estimate(c1, c2, n, rel_floor)
        evaluated.append(e[active])
        compared.append(thr_px[active])
        hot = active & (e > thr_px)
        go = hot.copy()
        if dilate:
            p = np.pad(hot, 1)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    go |= p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        go &= active & (2 * n <= smax)
        spp[active] = n
        err[active] = e[active].astype(f32)
        spp[go] = 2 * n
        active = go
        if not active.any():
            return spp, err, np.concatenate(evaluated), np.concatenate(compared)
        n *= 2


@pytest.fixture(scope="module")
def rule_run(pkg, hip):
    """cornell_demo 40 x 32 without the sky cull (every pixel takes part in the rounds): the per-sample renders, computed once."""
    old = os.environ.get("MCPT_SKY_CULL")
    os.environ["MCPT_SKY_CULL"] = "0"  # (read when the scene is created)
    try:
        hs = hip.HipScene(pkg.scenes.cornell_demo(40, 32, 32))
    finally:
        if old is None:
            del os.environ["MCPT_SKY_CULL"]
        else:
            os.environ["MCPT_SKY_CULL"] = old
    V = _samples(hs, 32, seed=3)
    yield hs, V
    hs.close()


@pytest.mark.parametrize("dilate", [0, 1])
def test_guided_stopping_rule_matches_numpy(rule_run, dilate):
    hs, V = rule_run
    S0, smax, rf = 4, 32, 1e-3
    H, W = V.shape[1:3]
    V64 = V.astype(np.float64)
    e0 = _estimate(np.cumsum(V64, 0), np.cumsum(V64 * V64, 0), S0, rf)
    thr = _mid_threshold(e0, 0.5)
    guide = tiled_guide(H, W)
    want_spp, want_err, evaluated, compared = _expected_counts_guided(V, S0, smax, thr, rf, dilate, guide)
    fin = np.isfinite(evaluated)
    assert not (np.abs(evaluated[fin] - compared[fin]) <= 1e-9 * compared[fin]).any(), "an estimate lies at its threshold: pick another seed"
    fb, spp, err, var, info, st = hs.render_adaptive_guided(S0, thr, guide, rel_floor=rf, dilate=dilate, spp=smax, seed=3)
    assert np.array_equal(spp, want_spp), int((spp != want_spp).sum())
    assert np.array_equal(err, want_err, equal_nan=True)
    assert len(np.unique(spp)) >= 3
    assert int(spp.sum()) == st.samples
    # monotonicity: no pixel has more samples than without the guide, and some have fewer
    _, plain_spp, plain_err, _, _ = hs.render_adaptive(S0, thr, rel_floor=rf, dilate=dilate, spp=smax, seed=3)
    plain_want, _, plain_eval, plain_cmp = _expected_counts_guided(V, S0, smax, thr, rf, dilate, None)
    pf = np.isfinite(plain_eval)
    assert not (np.abs(plain_eval[pf] - plain_cmp[pf]) <= 1e-9 * plain_cmp[pf]).any()
    assert np.array_equal(plain_spp, plain_want)
    assert (spp <= plain_spp).all()
    assert (spp < plain_spp).any()
    # err is the unscaled estimate: where both runs stopped at one count it is the same number
    same = spp == plain_spp
    assert np.array_equal(err[same], plain_err[same], equal_nan=True)


# ---------------------------------------------------------------- 3. bit-identity at the final count
@pytest.mark.parametrize("case", ["cornell_demo", "chess_dof"])
def test_guided_pixels_equal_uniform_renders_at_their_count(pkg, hip, case):
    if case == "cornell_demo":
        sd = pkg.scenes.cornell_demo(64, 64, 32)
    else:
        sd = pkg.scenes.chess_scene(width=160, height=90, spp=32)
        assert int(sd.camera["use_dof"]) == 1
    hs = hip.HipScene(sd)
    H, W = (64, 64) if case == "cornell_demo" else (90, 160)
    S0, smax = 4, 32
    _, _, e0, _, _ = hs.render_adaptive(S0, 1e30, spp=S0, seed=7)
    thr = _mid_threshold(e0, 0.25)
    guide = tiled_guide(H, W)
    fb, spp, err, var, info, st = hs.render_adaptive_guided(S0, thr, guide, dilate=1, spp=smax, seed=7)
    levels = _assert_exact(hs, fb, spp, seed=7)
    assert len(levels) >= 3, levels
    assert int(spp.sum()) == st.samples
    _, plain_spp, _, _, _ = hs.render_adaptive(S0, thr, dilate=1, spp=smax, seed=7)
    assert (spp <= plain_spp).all() and (spp < plain_spp).any()
    hs.close()


# ---------------------------------------------------------------- 4. null and all-ones guide
def test_null_and_all_ones_guide_are_render_adaptive(pkg, hip):
    sd = pkg.scenes.chess_scene(width=96, height=54, spp=16)  # (the sky cull finishes part of this frame)
    hs = hip.HipScene(sd)
    S0, smax = 4, 16
    _, _, e0, _, _ = hs.render_adaptive(S0, 1e30, spp=S0, seed=2)
    thr = _mid_threshold(e0, 0.4)
    fb, spp, err, info, st = hs.render_adaptive(S0, thr, spp=smax, seed=2)
    assert len(np.unique(spp)) >= 2
    for guide in (None, np.ones((54, 96), f32)):
        g_fb, g_spp, g_err, g_var, g_info, g_st = hs.render_adaptive_guided(S0, thr, guide, spp=smax, seed=2)
        assert np.array_equal(g_fb.view(np.uint32), fb.view(np.uint32))
        assert np.array_equal(g_spp, spp) and np.array_equal(g_err.view(np.uint32), err.view(np.uint32))
        assert g_info["rounds"] == info["rounds"] and g_info["active_pixels"] == info["active_pixels"] and g_st.samples == st.samples
    # a rank's share: unowned pixels are 0 in every output, the variance included
    kw = dict(seed=4, tile_size=16, rank=1, nranks=3)
    g_fb, g_spp, g_err, g_var, _, _ = hs.render_adaptive_guided(S0, thr, None, spp=smax, **kw)
    assert (g_spp == 0).any() and (g_var[g_spp == 0] == 0).all() and (g_fb[g_spp == 0] == 0).all()
    hs.close()


# ---------------------------------------------------------------- 5. the variance
def test_variance_is_the_restatement_at_each_pixels_count(rule_run):
    hs, V = rule_run
    S0, smax, rf = 4, 32, 1e-3
    H, W = V.shape[1:3]
    v = V.astype(np.float64)
    e0 = _estimate(np.cumsum(v, 0), np.cumsum(v * v, 0), S0, rf)
    thr = _mid_threshold(e0, 0.5)
    fb, spp, err, var, info, st = hs.render_adaptive_guided(S0, thr, tiled_guide(H, W), rel_floor=rf, dilate=1, spp=smax, seed=3)
    assert len(np.unique(spp)) >= 3
    s1, s2 = np.zeros(v.shape[1:]), np.zeros(v.shape[1:])
    want = np.zeros((H, W), f32)
    w = np.array([0.2126, 0.7152, 0.0722])
    for k in range(smax):  # in sample order, as k_accumulate<true>
        s1 = s1 + v[k]
        s2 = s2 + v[k] * v[k]
        n = k + 1
        if not (spp == n).any():
            continue
        with np.errstate(all="ignore"):
            m = s1 / n
            q = s2 / n - m * m
            vc = np.where(q < 0, 0.0, q) * n / (n - 1) / n
            lum = np.zeros((H, W))
            for c in range(3):
                lum = lum + (w[c] * w[c]) * vc[..., c]
        want = np.where(spp == n, lum.astype(f32), want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(var), fin)
    # the bound of test_gpu_denoise.test_variance_restatement: the two double evaluations agree but for the final rounding to float
    assert _ulps(var[fin], want[fin]).max() <= 1
    assert (var > 0).any()


def test_variance_at_s0_is_render_denoised(pkg, hip):
    sd = pkg.scenes.chess_scene(width=64, height=36, spp=8)
    hs = hip.HipScene(sd)
    for S0, smax in ((8, 8), (4, 16)):
        fb, spp, err, var, info, st = hs.render_adaptive_guided(S0, 1e30, None, spp=smax, seed=5)
        assert (spp == S0).all()
        r = hs.render_denoised(spp=S0, seed=5)
        assert bits_equal(var, r["variance"]) and bits_equal(fb, r["fb"])
    hs.close()


# ---------------------------------------------------------------- 6. the denoised adaptive frame is the composition of the calls
@pytest.mark.parametrize("specular_depth", [0, 2])
@pytest.mark.parametrize("size", [8, 64])
def test_adaptive_denoised_is_the_composition_of_the_calls(pkg, hip, size, specular_depth):
    sd = pkg.scenes.cornell_demo(size, size, 16)
    hs = hip.HipScene(sd)
    S0, smax = 4, 16
    _, _, e0, _, _ = hs.render_adaptive(S0, 1e30, spp=S0, seed=6)
    thr = _mid_threshold(e0, 0.5)
    guide = tiled_guide(size, size)
    for g in (guide, None):
        r = hs.render_adaptive_denoised(S0, thr, g, spp=smax, seed=6, aov_spp=2, specular_depth=specular_depth, iterations=4)
        fb, spp, err, var, info, st = hs.render_adaptive_guided(S0, thr, g, spp=smax, seed=6)
        aov = hs.render_aovs(aov_spp=2, seed=6, specular_depth=specular_depth)
        assert bits_equal(r["fb"], fb) and np.array_equal(r["spp"], spp) and bits_equal(r["err"], err)
        assert bits_equal(r["variance"], var)
        assert bits_equal(r["aov"], aov)
        assert bits_equal(r["denoised"], hs.denoise(fb, var, aov, iterations=4))
        assert r["adaptive_info"]["active_pixels"] == info["active_pixels"] and r["stats"].samples == st.samples == int(spp.sum())
    assert len(np.unique(spp)) >= 2
    # the default aov_spp is min(4, min_spp)
    r = hs.render_adaptive_denoised(2, thr, None, spp=8, seed=6)
    assert bits_equal(r["aov"], hs.render_aovs(aov_spp=2, seed=6))
    with pytest.raises(hip.McptError) as e:
        hs.render_adaptive_denoised(2, thr, None, spp=8, seed=6, aov_spp=4)
    assert e.value.code == 1 and "aov_spp" in str(e.value)
    hs.close()


# ---------------------------------------------------------------- 7. the host executable
def test_host_executable_adaptive_denoise(pkg, hip, tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "RayTracing")
    conf = json.loads(json.dumps(pkg.scenes.DEFAULT_CONF))
    conf["camera"]["width"], conf["camera"]["height"], conf["renderer"]["spp"] = 96, 54, 32
    (tmp_path / "conf.json").write_text(json.dumps(conf))
    out, den = str(tmp_path / "adaptive.png"), str(tmp_path / "den.png")
    p = subprocess.run([exe, "--models", MODELS, "--output", out, "--adaptive", "0.1", "--adaptive-min", "4", "--adaptive-denoise", den,
                        "--denoise-aov-spp", "2"], cwd=str(tmp_path), capture_output=True, text=True)
    assert p.returncode == 0 and "Rendering finished in" in p.stdout, p.stderr
    hs = hip.HipScene(pkg.scenes.chess_scene(conf))
    r = hs.render_adaptive_denoised(4, 0.1, None, rel_floor=1e-3, dilate=1, spp=32, seed=1, aov_spp=2)
    assert ("%d samples in total" % r["stats"].samples) in p.stdout, p.stdout
    # (the executable tone-maps on the device, mcpt_tonemap: the CPU's pow rounds a byte the other way now and then)
    assert np.array_equal(pkg.pngio.read_png(out)[:, :, :3], hs.tonemap(r["fb"])[:, :, :3])
    assert np.array_equal(pkg.pngio.read_png(den)[:, :, :3], hs.tonemap(r["denoised"])[:, :, :3])
    for extra, msg in ((["--checkpoint", str(tmp_path / "c.ckpt")], "--checkpoint"), (["--gpus", "2"], "more than one device")):
        p = subprocess.run([exe, "--models", MODELS, "--output", out, "--adaptive", "0.1", "--adaptive-denoise", den] + extra, cwd=str(tmp_path),
                           capture_output=True, text=True)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr)
    p = subprocess.run([exe, "--models", MODELS, "--output", out, "--adaptive-denoise", den], cwd=str(tmp_path), capture_output=True, text=True)
    assert p.returncode != 0 and "--adaptive" in p.stderr
    hs.close()
