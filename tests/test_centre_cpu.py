"""Pixel-centre feature rays without a GPU (include/mcpt.h: mcpt_feature_opts, mcpt_centre_rays, mcpt_render_aovs_features,
mcpt_render_motion_features, mcpt_sequence_create_features): the float32 restatement of the centre ray (tests/centre_cases.py) agrees with
float64; the host build of the motion pass's projection (csrc/mcpt_temporal.h through tests/native/temporal_driver.cpp) sends a point of a
centre ray back to the centre of its pixel, so that a centre feature's motion is measured from where the pixel is; the struct has the
header's size; the calls refuse invalid options before they touch a device.  tests/test_gpu_centre.py checks the kernel against the
restatement bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from centre_cases import cameras, centre_rays_f32, centre_rays_f64  # noqa: E402
from test_temporal_cpu import build_driver  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAMERAS = ["cornell", "cornell_dof", "chess_dof"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("centre_cpu"))


@pytest.mark.parametrize("name", CAMERAS)
def test_restatement_agrees_with_float64(pkg, name):
    """Direction within 1e-5 relative (unit vectors: absolute) of the float64 pinhole ray -- a dozen float32 operations of 6e-8 each --
    and the origin is the eye exactly: with depth of field the lens offset is orient * (aperture * 0, aperture * 0 * +0, 0) = 0."""
    _, cam = cameras(pkg)[name]
    o, d = centre_rays_f32(cam)
    o64, d64 = centre_rays_f64(cam)
    assert o.shape == d.shape == (int(cam["width"]) * int(cam["height"]), 3)
    err = np.abs(d.astype(np.float64) - d64).max()
    print("%s: max |f32 - f64| direction component = %.3g" % (name, err))
    assert err <= 1e-5
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert np.array_equal(o, np.broadcast_to(np.asarray(cam["position"], f32).reshape(3), o.shape))
    # a subset of pixels in any order gives those pixels' rays
    pick = np.array([len(o) - 1, 0, 7, len(o) // 2], np.uint32)
    o2, d2 = centre_rays_f32(cam, pick)
    assert np.array_equal(o2, o[pick]) and np.array_equal(d2.view(np.uint32), d[pick].view(np.uint32))


@pytest.mark.parametrize("name", CAMERAS)
def test_projection_sends_the_centre_ray_back_to_the_pixel_centre(pkg, driver, name):
    """proj(camera, o + d * t) = (i + 0.5, j + 0.5) within 1e-2 px, the bound test_temporal_cpu.py uses for the projection, for every pixel
    and for t over three decades."""
    _, cam = cameras(pkg)[name]
    W, H = int(cam["width"]), int(cam["height"])
    o, d = centre_rays_f32(cam)
    j, i = np.mgrid[0:H, 0:W]
    want = np.stack([i + 0.5, j + 0.5], -1).reshape(-1, 2)
    cam_c = np.ascontiguousarray(cam)
    n = W * H
    for t in (10.0, 100.0, 1000.0, 10000.0):
        p = (o + d * f32(t)).astype(f32)  # (as the motion pass forms a sphere's hit point)
        xy, ok = np.zeros((n, 2), f32), np.zeros(n, np.int32)
        driver.tp_project(n, cam_c.ctypes.data, p.ctypes.data, xy.ctypes.data, ok.ctypes.data)
        assert ok.all()
        err = np.abs(xy - want).max()
        print("%s, t = %g: max |proj - pixel centre| = %.3g px" % (name, t, err))
        assert err < 1e-2, (t, err)


def test_struct_size_and_header(hip):
    assert C.sizeof(hip.FeatureOpts) == 32 and hip.FeatureOpts.reserved.offset == 4
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "typedef struct {\n    int32_t centre;" in h and "} mcpt_feature_opts;     /* 32 bytes */" in h
    for name in ("mcpt_centre_rays", "mcpt_render_aovs_features", "mcpt_render_motion_features", "mcpt_sequence_create_features"):
        assert ("int %s(" % name) in h and name in hip.EXPORTS


def test_argument_checks_come_before_any_device_call(pkg, hip):
    """Every refusal below happens before the library touches a device (there is none on the machines that run this test) and before it
    reads the scene: the handle is not a scene and not mapped memory."""
    L = hip.lib()
    fake = C.c_void_p(0x1000)
    W, H = 4, 3
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    cam = np.ascontiguousarray(pkg.scenes.make_camera(W, H, 40, (0, 0, -5), (0, 0, 0)))
    aov, mo = np.zeros((H, W, 8), f32), np.zeros((H, W, 4), f32)

    def feat(centre=1, word=None):
        o = hip.FeatureOpts(centre=centre)
        if word is not None:
            o.reserved[word] = 1
        return o

    def aovs(o, aov_spp=1, depth=0):
        return L.mcpt_render_aovs_features(fake, p(cam), 1, aov_spp, depth, None if o is None else C.byref(o), p(aov))

    def motion(o, aov_spp=1, depth=0):
        return L.mcpt_render_motion_features(fake, p(cam), p(cam), 1, aov_spp, depth, None if o is None else C.byref(o), p(mo))

    for call, name in ((aovs, b"mcpt_render_aovs_features"), (motion, b"mcpt_render_motion_features")):
        for o in (feat(2), feat(-1)):
            assert call(o) == 1 and name in L.mcpt_last_error() and b"centre" in L.mcpt_last_error()
        for k in range(7):
            assert call(feat(1, k)) == 1 and call(feat(0, k)) == 1, k
            assert b"reserved" in L.mcpt_last_error()
        for spp in (2, 4, 65536):
            assert call(feat(1), aov_spp=spp) == 1 and name in L.mcpt_last_error(), spp
        # what the _ex calls refuse is refused with every setting of the switch
        for o in (None, feat(0), feat(1)):
            assert call(o, aov_spp=-1) == 1 and call(o, aov_spp=65537) == 1
            assert call(o, depth=9) == 1 and call(o, depth=-1) == 1
    assert L.mcpt_render_aovs_features(None, p(cam), 1, 1, 0, None, p(aov)) == 1
    assert L.mcpt_render_aovs_features(fake, None, 1, 1, 0, None, p(aov)) == 1
    assert L.mcpt_render_aovs_features(fake, p(cam), 1, 1, 0, None, None) == 1
    assert L.mcpt_render_motion_features(fake, p(cam), None, 1, 1, 0, None, p(mo)) == 1
    assert L.mcpt_render_motion_features(fake, p(cam), p(cam), 1, 1, 0, None, None) == 1

    # mcpt_centre_rays
    px, o3, d3 = np.zeros(2, np.uint32), np.zeros((2, 3), f32), np.zeros((2, 3), f32)
    assert L.mcpt_centre_rays(None, p(cam), 2, p(px), p(o3), p(d3)) == 1 and b"mcpt_centre_rays" in L.mcpt_last_error()
    assert L.mcpt_centre_rays(fake, None, 2, p(px), p(o3), p(d3)) == 1
    assert L.mcpt_centre_rays(fake, p(cam), -1, p(px), p(o3), p(d3)) == 1
    assert L.mcpt_centre_rays(fake, p(cam), 1 << 31, p(px), p(o3), p(d3)) == 1
    for k in (3, 4, 5):
        args = [fake, p(cam), 2, p(px), p(o3), p(d3)]
        args[k] = None
        assert L.mcpt_centre_rays(*args) == 1, k
    zero_w = cam.copy()
    zero_w["width"] = 0
    assert L.mcpt_centre_rays(fake, p(zero_w), 2, p(px), p(o3), p(d3)) == 1
    assert L.mcpt_centre_rays(fake, p(cam), 0, None, None, None) == 0  # nothing to do

    # mcpt_sequence_create_features
    h = C.c_void_p()

    def create(f, aov_spp=0, adaptive=None, moments=None):
        o = hip.SequenceOpts(filter=1)
        o.denoise.aov_spp = aov_spp
        return L.mcpt_sequence_create_features(fake, W, H, C.byref(o), None, None if adaptive is None else C.byref(adaptive), None, None,
                                               None if moments is None else C.byref(moments), None if f is None else C.byref(f), C.byref(h))

    for o in (feat(2), feat(-1)):
        assert create(o) == 1 and b"mcpt_sequence_create" in L.mcpt_last_error() and b"centre" in L.mcpt_last_error()
    for k in range(7):
        assert create(feat(1, k)) == 1 and create(feat(0, k)) == 1, k
    rule = hip.sequence_adaptive(min_spp=2, threshold=0.05)
    for spp in (2, 4):
        assert create(feat(1), aov_spp=spp) == 1, spp
        assert create(feat(1), aov_spp=spp, adaptive=rule) == 1, spp
        assert create(feat(1), aov_spp=spp, moments=hip.moments_opts()) == 1, spp
    # what mcpt_sequence_create_moments refuses is refused with every setting of the switch
    for f in (None, feat(0), feat(1)):
        assert create(f, aov_spp=-1) == 1 and create(f, aov_spp=65537) == 1
        assert create(f, adaptive=rule, moments=hip.moments_opts()) == 1
        assert L.mcpt_sequence_create_features(None, W, H, C.byref(hip.SequenceOpts()), None, None, None, None, None,
                                               None if f is None else C.byref(f), C.byref(h)) == 1
        assert L.mcpt_sequence_create_features(fake, 0, H, C.byref(hip.SequenceOpts()), None, None, None, None, None,
                                               None if f is None else C.byref(f), C.byref(h)) == 1
    assert h.value is None
