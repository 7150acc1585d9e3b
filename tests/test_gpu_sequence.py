"""Frame sequences on the GPU (include/mcpt.h: mcpt_temporal_accumulate, mcpt_sequence_*): k_temporal_accumulate gives the bits of the CPU
build of tp::accumulate_pixel; a sequence is the composition of the calls the library already has (render, render_aovs, render_motion,
temporal_blend / temporal_accumulate, denoise, tonemap), bit for bit, with the host builder and with PLOC; the propagated variance of a
static sequence is (sum of the frames' variances) / N^2; reset, a panned camera, specular AOVs, filter off, the errors; and the quality
figures DESIGN section 8e quotes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import KINDS, SHAPES, bits_equal  # noqa: E402
from test_sequence_cpu import VAR_KINDS, accumulate_case, build_driver, host_accumulate  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHORT = 1  # cornell_demo, Scene::Add order: floor, short box, ...
ALL = ("fb", "accumulated", "denoised", "variance", "len", "aov", "motion", "rgba")


def translate(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], f32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("seq_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


# ---------------------------------------------------------------- 1. the kernel against the CPU build
@pytest.mark.parametrize("shape", SHAPES + [(64, 64)])
@pytest.mark.parametrize("kind", KINDS + VAR_KINDS)
def test_accumulate_device_equals_host_build(hip, tiny, driver, kind, shape):
    H, W = shape
    args, opts = accumulate_case(kind, H, W)
    got, got_var, got_len = tiny.temporal_accumulate(*args, **opts)
    want, want_var, want_len = host_accumulate(driver, hip, *args, **opts)
    assert bits_equal(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(got_len, want_len)
    assert bits_equal(got_var, want_var), int((got_var.view(np.uint32) != want_var.view(np.uint32)).sum())
    # colour and length are the blend kernel's
    color, variance, motion, prev_color, prev_variance, prev_depth, prev_len = args
    blend, blend_len = tiny.temporal_blend(color, motion, prev_color, prev_depth, prev_len, **opts)
    assert bits_equal(got, blend) and bits_equal(got_len, blend_len)


# ---------------------------------------------------------------- 2. the sequence is the composition of the calls we already have
@pytest.mark.parametrize("size", [8, 17, 64])
@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_sequence_is_the_composition_of_the_calls(pkg, hip, builder, size):
    """Six frames, the short box moved by translate(-32 k, 0, 0) before frame k.  With the host builder the separate calls run on a second
    handle.  A tree built on the device is only promised to agree with another device build up to box-grazing rays (include/mcpt.h,
    mcpt_scene_update), so with PLOC the separate calls run on the sequence's own handle, before the sequence's frame: the snapshot they see
    is the one the sequence took at the end of its previous frame, which is what `snapshot; update` gives, and the tree is the very same."""
    H = W = size
    sd = pkg.scenes.cornell_demo(W, H, 4)
    a = hip.HipScene(sd, builder=builder)
    b = a if builder == "ploc" else hip.HipScene(sd, builder=builder)
    seq = a.sequence(filter=True, aov_spp=4)
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    hist_var, prev_depth = np.zeros((H, W), f32), np.zeros((H, W), f32)
    for k in range(6):
        m = translate(-32.0 * k, 0, 0)
        b.snapshot()
        info = b.update([(SHORT, m)])
        assert info["path"] == (1 if builder == "ploc" else 0)
        if a is not b:
            a.update([(SHORT, m)])
        rd = b.render_denoised(spp=4, seed=k + 1, aov_spp=4)
        c, _ = b.render(spp=4, seed=k + 1)
        aov = b.render_aovs(aov_spp=4, seed=k + 1)
        motion = b.render_motion(seed=k + 1, aov_spp=4)
        blend, blend_len = b.temporal_blend(c, motion, hist, prev_depth, length)
        acc, acc_var, acc_len = b.temporal_accumulate(c, rd["variance"], motion, hist, hist_var, prev_depth, length)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=ALL, spp=4, seed=k + 1)
        assert r["info"]["frame_index"] == k
        assert bits_equal(r["fb"], c), k
        assert bits_equal(r["aov"], aov), k
        assert bits_equal(r["motion"], motion), k
        assert bits_equal(r["accumulated"], blend) and bits_equal(r["len"], blend_len), k
        assert bits_equal(acc, blend) and bits_equal(acc_len, blend_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        if k > 0 and size == 64:
            assert (motion[..., 0:2] != 0).any() and (blend_len > 1).any(), k
        hist, length, hist_var, prev_depth = blend, blend_len, acc_var, aov[..., 6].copy()
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 3. static sequence
@pytest.fixture(scope="module")
def static_run(pkg, hip):
    """Eight frames of the static 64 x 64 Cornell scene through a sequence (every output kept), and each frame's own variance."""
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd)
    seq = hs.sequence(filter=True, aov_spp=4, max_history=32)
    frames = []
    for k in range(8):
        r = seq.frame(want=ALL, spp=4, seed=k + 1)
        r["frame_variance"] = hs.render_denoised(spp=4, seed=k + 1, aov_spp=4)["variance"]
        frames.append(r)
    yield hs, seq, frames
    seq.close()
    hs.close()


def test_static_sequence_variance(static_run):
    """On the pixels the rule of include/mcpt.h keeps in all frames so far (the mask of test_gpu_temporal.test_static_accumulation, computed
    the same way) len counts the frames, the variance is the float32 recurrence of the frames' variances bit for bit, and it is
    (sum v_k) / (k + 1)^2 within rtol 1e-4 (tests/test_sequence_cpu.py derives that bound).  At least 1000 such pixels: the back wall alone,
    seen head-on at constant depth, is about a third of the 4096 pixels and cannot fail a 2 % depth test."""
    _, _, frames = static_run
    H = W = 64
    stable = np.ones((H, W), bool)
    ref = ref_v = prev_depth = None
    total = np.zeros((H, W), np.float64)
    for k, r in enumerate(frames):
        c, v, motion = r["fb"], r["frame_variance"], r["motion"]
        assert (motion[..., 0:2] == 0).all()
        total += v
        if k == 0:
            ref, ref_v = c.copy(), v.copy()
            assert (r["len"] == 1).all() and bits_equal(r["accumulated"], c) and bits_equal(r["variance"], v)
        else:
            zp = motion[..., 2]
            stable &= (motion[..., 3] > 0) & np.isfinite(c).all(-1) & np.isfinite(ref).all(-1) & (np.abs(prev_depth - zp) <= f32(0.02) * zp)
            kk = f32(1) / f32(k + 1)
            omk = f32(1) - kk
            ref = ref + (c - ref) * kk
            ref_v = (omk * omk) * ref_v + (kk * kk) * v
        assert ref.dtype == f32 and ref_v.dtype == f32
        assert (r["len"][stable] == k + 1).all(), k
        assert bits_equal(r["accumulated"][stable], ref[stable]), k
        assert bits_equal(r["variance"][stable], ref_v[stable]), k
        want = total[stable] / (k + 1) ** 2
        got = r["variance"][stable].astype(np.float64)
        print("static sequence, frame %d: max relative |variance - sum v / N^2| = %.3g on %d pixels"
              % (k, float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0))), int(stable.sum())))
        assert np.allclose(got, want, rtol=1e-4, atol=0), k
        prev_depth = r["aov"][..., 6].copy()
    assert stable.sum() >= 1000


# ---------------------------------------------------------------- 8. quality (printed and recorded, not asserted beyond finiteness)
def test_quality_figures(static_run):
    hs, _, frames = static_run
    truth, _ = hs.render(spp=2048, seed=1000)
    first, last = frames[0], frames[-1]

    def mse(img):
        return float(((np.asarray(img, np.float64) - truth) ** 2).mean())

    figures = [
        ("one 4-spp frame", mse(first["fb"])),
        ("one frame, filtered", mse(first["denoised"])),
        ("8 frames accumulated", mse(last["accumulated"])),
        ("accumulated, filtered with the propagated variance", mse(last["denoised"])),
        ("accumulated, filtered with the last frame's own variance", mse(hs.denoise(last["accumulated"], last["frame_variance"], last["aov"]))),
    ]
    for name, v in figures:
        print("sequence quality, MSE against 2048 spp: %-58s %.5g" % (name, v))
        assert np.isfinite(v)
    # (frame 0 has no history: its filtered output is the plain filter of that frame)
    assert bits_equal(first["denoised"], hs.denoise(first["fb"], first["frame_variance"], first["aov"]))


# ---------------------------------------------------------------- 4. reset and a panned camera
def test_reset_and_pan(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd)
    seq = hs.sequence(filter=False, aov_spp=4)
    want = ("fb", "accumulated", "variance", "len", "motion")
    seq.frame(want=want, spp=4, seed=1)
    r = seq.frame(want=want, spp=4, seed=2)
    assert r["len"].max() == 2 and r["info"]["frame_index"] == 1
    seq.reset()
    r = seq.frame(want=want, spp=4, seed=3)
    own = hs.render_denoised(spp=4, seed=3, aov_spp=4)
    assert r["info"]["frame_index"] == 0
    assert (r["len"] == 1).all()
    assert bits_equal(r["accumulated"], r["fb"]) and bits_equal(r["fb"], own["fb"])
    assert bits_equal(r["variance"], own["variance"])
    # a 2 degree pan without a reset: the motion is that against the remembered camera of the previous frame
    a = np.radians(2.0)
    eye = np.array([278, 273, -800.0])
    fwd = np.array([np.sin(a), 0, np.cos(a)]) * 800
    pan = pkg.scenes.make_camera(64, 64, 40, eye, eye + fwd, (0, 1, 0), focal_distance=900, aperture_radius=40)
    r = seq.frame(camera=pan, want=want, spp=4, seed=4)
    valid = r["motion"][..., 3] > 0
    assert valid.sum() > 1000 and np.abs(r["motion"][..., 0][valid]).min() > 1
    assert bits_equal(r["motion"], hs.render_motion(prev_camera=sd.camera, camera=pan, seed=4, aov_spp=4))
    assert r["len"].max() == 2
    # ... and a frame after a reset under that camera has zero motion again
    seq.reset()
    r = seq.frame(camera=pan, want=want, spp=4, seed=5)
    assert (r["motion"][..., 0:2] == 0).all() and (r["len"] == 1).all()
    seq.close()
    hs.close()


# ---------------------------------------------------------------- 5. specular AOVs: the history depth stays first-hit
def test_specular_depth_keeps_first_hit_history(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    h0, h2 = hip.HipScene(sd), hip.HipScene(sd)
    s0, s2 = h0.sequence(filter=True, aov_spp=4), h2.sequence(filter=True, aov_spp=4, specular_depth=2)
    differ = False
    for k in range(4):
        r0 = s0.frame(want=("accumulated", "len", "aov"), spp=4, seed=k + 1)
        r2 = s2.frame(want=("accumulated", "len", "aov", "denoised"), spp=4, seed=k + 1)
        assert bits_equal(r0["accumulated"], r2["accumulated"]) and bits_equal(r0["len"], r2["len"]), k
        assert bits_equal(r2["aov"], h2.render_aovs(aov_spp=4, seed=k + 1, specular_depth=2)), k
        assert bits_equal(r0["aov"], h0.render_aovs(aov_spp=4, seed=k + 1)), k
        differ |= not bits_equal(r0["aov"][..., 6], r2["aov"][..., 6])
    assert differ  # (the mirror and glass spheres: the specular AOVs carry another depth there, which must not reach the history)
    assert r0["len"].max() == 4
    for x in (s0, s2, h0, h2):
        x.close()


# ---------------------------------------------------------------- 6. filter off
def test_filter_off(pkg, hip, tiny):
    seq = tiny.sequence(filter=False, aov_spp=4)
    with pytest.raises(hip.McptError) as e:
        seq.frame(want=("denoised",), spp=4, seed=1)
    assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value)
    for k in range(2):
        r = seq.frame(want=("accumulated", "rgba", "len"), spp=4, seed=k + 1)
        assert np.array_equal(r["rgba"], tiny.tonemap(r["accumulated"])), k
    assert r["len"].max() == 2  # the refused frame did not start a history of its own
    seq.close()


# ---------------------------------------------------------------- 7. errors
def test_errors_leave_the_history(pkg, hip, tiny):
    seq = tiny.sequence(filter=True, aov_spp=4)
    r = seq.frame(want=("len",), spp=4, seed=1)
    assert (r["len"] == 1).all()
    other = pkg.scenes.make_camera(9, 8, 40, (278, 273, -800), (278, 273, 0))
    for kw in (dict(camera=other, spp=4), dict(spp=1), dict(spp=4, nranks=2), dict(spp=2), dict(spp=4, spp_total=8), dict(spp=4, sample_offset=4),
               dict(spp=4, accumulate=1)):
        with pytest.raises(hip.McptError) as e:
            seq.frame(want=("len",), seed=2, **kw)
        assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value), kw
    with pytest.raises(ValueError):
        seq.frame(want=("colour",), spp=4, seed=2)
    r = seq.frame(want=("len",), spp=4, seed=2)
    assert r["len"].max() == 2 and r["info"]["frame_index"] == 1  # the history goes on counting
    # no output asked for: the frame still advances the history
    r = seq.frame(want=(), spp=4, seed=3)
    assert set(r) == {"info", "stats"} and r["info"]["frame_index"] == 2
    assert seq.frame(want=("len",), spp=4, seed=4)["len"].max() == 4
    seq.close()
    seq.close()  # idempotent
    with pytest.raises(hip.McptError) as e:
        tiny.sequence(width=8, height=8, max_history=5000)
    assert e.value.code == 1 and "mcpt_sequence_create" in str(e.value)
