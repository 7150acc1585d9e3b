"""Motion through mirror and glass chains on the GPU (include/mcpt.h: mcpt_render_motion_ex): depth 0 is mcpt_render_motion bit for bit; a
static scene has exactly zero motion, the coverage of the chain AOVs and their depth; a moved box, a moved and a tilted mirror, a panned
camera, two reflections and the depth cap, a moved mirror sphere and a glass sphere against a float64 restatement of every chain
(tests/mirror_scene.py: the chains from the library's own camera rays and hits, the planes from mcpt_transform_triangles, the reflections in
float64); the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirror_scene as ms  # noqa: E402
from test_gpu_temporal import DEPTH_TOL, PX_TOL, assert_motion_close  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
D = 4
BOX_MOVE = ms.translate(3, 0, 0)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def motion_ex(hs, depth, seed=1, aov_spp=4, camera=None, prev_camera=None):
    """mcpt_render_motion_ex called directly (HipScene.render_motion takes the plain entry point for depth 0)."""
    cam = np.ascontiguousarray(camera if camera is not None else hs.sd.camera)
    prev = np.ascontiguousarray(prev_camera if prev_camera is not None else cam)
    Wc, Hc = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
    out = np.zeros((Hc, Wc, 4), f32)
    rc = hs.L.mcpt_render_motion_ex(hs.h, cam.ctypes.data_as(C.c_void_p), prev.ctypes.data_as(C.c_void_p), int(seed), int(aov_spp), int(depth),
                                    out.ctypes.data_as(C.c_void_p))
    assert rc == 0, hs.L.mcpt_last_error()
    return out


# ---------------------------------------------------------------- 1. depth 0
def test_depth_zero_is_the_first_hit_pass(pkg, hip):
    hs = hip.HipScene(ms.mirror_scene(pkg))
    for _ in range(2):  # a fresh scene (buffers of the call's own), then inside the workspace of a render
        for spp in (1, 4):
            assert bits_equal(motion_ex(hs, 0, seed=3, aov_spp=spp), hs.render_motion(seed=3, aov_spp=spp))
        assert bits_equal(hs.render_motion(seed=3, aov_spp=4, specular_depth=0), hs.render_motion(seed=3, aov_spp=4))
        hs.snapshot()
        hs.update([(ms.BOX, BOX_MOVE)])
        hs.render(spp=2, seed=1)
    hs.close()


# ---------------------------------------------------------------- 2. static scene
@pytest.mark.parametrize("name", ["mirrors", "cornell"])
def test_static_scene_has_zero_motion_and_the_chain_coverage(pkg, hip, oracle, name):
    sd = ms.mirror_scene(pkg) if name == "mirrors" else pkg.scenes.cornell_demo(48, 48, 4)
    hs = hip.HipScene(sd)
    runs = []
    for rendered in (False, True):  # the call's own buffers, then the workspace of a 2-spp render
        if rendered:
            hs.render(spp=2, seed=1)
        aov = hs.render_aovs(aov_spp=4, seed=1, specular_depth=D)
        for snap in (False, True):
            if snap:
                hs.snapshot()
            m = hs.render_motion(seed=1, aov_spp=4, specular_depth=D)
            assert (m[..., 0] == 0).all() and (m[..., 1] == 0).all(), (rendered, snap)
            assert bits_equal(m[..., 3], aov[..., 7]), (rendered, snap)
            runs.append(m)
    for m in runs[1:]:
        assert bits_equal(m, runs[0])  # with and without a snapshot, and the two buffer paths
    assert (aov[..., 7] > 0).any() and not bits_equal(aov, hs.render_aovs(aov_spp=4, seed=1))
    if name == "mirrors":
        r = ms.chain_motion_f64(oracle, hs, sd, sd, sd.camera, sd.camera, D)
        ok = (r["n_refr"] == 0).all(-1) & (aov[..., 7] > 0)
        rel = np.abs(m[..., 2][ok].astype(np.float64) - aov[..., 6][ok]) / aov[..., 6][ok]
        print("\n[specular motion] static mirrors: max relative |prev_depth - chain AOV depth| = %.3g on %d pixels without refraction (%d of them "
              "through a mirror)" % (rel.max(), int(ok.sum()), int((ok & (r["n_refl"] > 0).any(-1)).sum())))
        assert rel.max() < DEPTH_TOL
        assert (ok & (r["n_refl"] > 0).all(-1)).sum() > 300
    hs.close()


@pytest.mark.parametrize("size", [(1, 1), (33, 17)], ids=["1x1", "33x17"])
def test_static_scene_odd_sizes(pkg, hip, size):
    sd = ms.mirror_scene(pkg, *size)
    hs = hip.HipScene(sd)
    for rendered in (False, True):
        if rendered:
            hs.render(spp=2, seed=1)
        aov = hs.render_aovs(aov_spp=4, seed=1, specular_depth=D)
        m = hs.render_motion(seed=1, aov_spp=4, specular_depth=D)
        assert m.shape == (size[1], size[0], 4)
        assert (m[..., 0] == 0).all() and (m[..., 1] == 0).all()
        assert bits_equal(m[..., 3], aov[..., 7]) and (m[..., 3] > 0).any()
    hs.close()


# ---------------------------------------------------------------- 3.-8. against the float64 restatement
_cases = {}


def moved_case(pkg, hip, oracle, xf, builder="sah", depth=D, camera=None, prev_camera=None):
    """snapshot, then update(xf); (device chain motion, first-hit motion, the restatement's dict, the scene); computed once per case."""
    key = (tuple(sorted((o, m.tobytes()) for o, m in xf.items())), builder, depth, None if camera is None else camera.tobytes(),
           None if prev_camera is None else prev_camera.tobytes())
    if key not in _cases:
        sd = ms.mirror_scene(pkg)
        hs = hip.HipScene(sd, builder=builder)
        hs.snapshot()
        if xf:
            info = hs.update(list(xf.items()))
            assert info["path"] == (1 if builder == "ploc" else 0)
        cam = sd.camera if camera is None else camera
        prev = cam if prev_camera is None else prev_camera
        got = hs.render_motion(seed=1, aov_spp=4, specular_depth=depth, camera=cam, prev_camera=prev)
        plain = hs.render_motion(seed=1, aov_spp=4, camera=cam, prev_camera=prev)
        want = ms.chain_motion_f64(oracle, hs, ms.moved_scene(pkg, hip, sd, xf), sd, cam, prev, depth)
        hs.close()
        _cases[key] = (got, plain, want, sd)
    return _cases[key]


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_box_moved(pkg, hip, oracle, builder):
    """The gap this pass closes: on M, the pixels whose four first hits are the (static) floor mirror and whose four chains end on the moved
    box, the first-hit pass reports exactly 0 and the chain pass the motion of the reflection.  Checked on the CPU with the oracle library
    when the scene was made: M holds 571 pixels of the 48 x 48 frame, more than 4 x the 30 asserted."""
    got, plain, want, sd = moved_case(pkg, hip, oracle, {ms.BOX: BOX_MOVE}, builder)
    assert_motion_close(got, want["motion"], "box moved, %s" % builder)
    M = np.isin(want["first"], ms.prims_of(sd, [ms.FLOOR])).all(-1) & np.isin(want["last"], ms.prims_of(sd, [ms.BOX])).all(-1)
    print("[specular motion] box moved: %d pixels see the box in the floor with all four samples" % int(M.sum()))
    assert M.sum() >= 30
    assert (plain[..., 0:2][M] == 0).all()
    assert (np.hypot(got[..., 0][M], got[..., 1][M]) > 1).all()
    other = moved_case(pkg, hip, oracle, {ms.BOX: BOX_MOVE}, "sah" if builder == "ploc" else "ploc")[0]
    assert np.array_equal(got[..., 3], other[..., 3])
    assert np.abs(got[..., 0:2] - other[..., 0:2]).max() < PX_TOL


@pytest.mark.parametrize("kind", ["along_normal", "tilted"])
def test_mirror_moved(pkg, hip, oracle, kind):
    """The box is static; the floor mirror is moved along its normal, or tilted 2 degrees about an in-plane axis (the snapshot's normal then
    differs from the live one)."""
    xf = {ms.FLOOR: ms.translate(0, -1.5, 0) if kind == "along_normal" else ms.rotate_z(2.0)}
    got, plain, want, sd = moved_case(pkg, hip, oracle, xf)
    assert_motion_close(got, want["motion"], "floor %s" % kind)
    M = np.isin(want["first"], ms.prims_of(sd, [ms.FLOOR])).all(-1) & np.isin(want["last"], ms.prims_of(sd, [ms.BOX])).all(-1)
    assert M.sum() >= 30
    # the reflection of the static box moves (least near the tilt's axis), and not as the floor's own surface does
    assert np.median(np.hypot(got[..., 0][M], got[..., 1][M])) > 0.5
    assert np.abs(got[..., 0:2][M] - plain[..., 0:2][M]).max() > 0.5


def test_camera_pan(pkg, hip, oracle):
    prev = ms.camera(pkg, pan_deg=2.0)
    got, plain, want, sd = moved_case(pkg, hip, oracle, {}, prev_camera=prev)
    assert_motion_close(got, want["motion"], "2 degree pan")
    M = np.isin(want["first"], ms.prims_of(sd, [ms.FLOOR])).all(-1) & np.isin(want["last"], ms.prims_of(sd, [ms.BOX])).all(-1)
    assert M.sum() >= 30
    # the reflection is reprojected with its own parallax, not the floor's: a pan moves both by about the same amount, but not the same
    assert np.abs(got[..., 0][M]).min() > 1
    assert not bits_equal(got[..., 0:2][M], plain[..., 0:2][M])
    assert np.median(got[..., 2][M] - plain[..., 2][M]) > 1  # the depth is the chain's (the two meet where the box stands on the floor)


@pytest.mark.parametrize("depth", [1, 2])
def test_two_reflections_and_the_cap(pkg, hip, oracle, depth):
    """A view past the box into the corner of the floor and the back mirror, the box moved: at depth 1 a sample stops on the second mirror,
    at depth 2 it goes on to the box with two reflections in its maps."""
    cam = ms.corner_camera(pkg)
    got, plain, want, sd = moved_case(pkg, hip, oracle, {ms.BOX: BOX_MOVE}, depth=depth, camera=cam)
    assert_motion_close(got, want["motion"], "corner, depth %d" % depth)
    back = np.isin(want["last"], ms.prims_of(sd, [ms.BACK]))
    two = (want["n_refl"] == 2) & want["valid"]
    print("[specular motion] corner, depth %d: %d samples end on the back mirror, %d carry two reflections" % (depth, int(back.sum()), int(two.sum())))
    if depth == 1:
        assert (want["n_refl"] <= 1).all() and (back & (want["n_refl"] == 1)).sum() >= 30
    else:
        assert two.sum() >= 30 and not back.any()
        px = two.all(-1) & np.isin(want["last"], ms.prims_of(sd, [ms.BOX])).all(-1)
        assert px.sum() >= 5 and (np.hypot(got[..., 0][px], got[..., 1][px]) > 1).all()


def test_mirror_sphere_moved(pkg, hip, oracle):
    got, plain, want, sd = moved_case(pkg, hip, oracle, {ms.MIRROR_SPHERE: ms.translate(1.0, 0.5, 0)})
    assert_motion_close(got, want["motion"], "mirror sphere moved")
    # (most of what the sphere shows is sky: an invalid sample; the rest ends on the box and on the light)
    on = np.isin(want["first"], ms.prims_of(sd, [ms.MIRROR_SPHERE])) & want["valid"] & (want["n_refl"] > 0)
    print("[specular motion] mirror sphere: %d valid samples in %d pixels" % (int(on.sum()), int(on.any(-1).sum())))
    assert on.sum() >= 30 and on.any(-1).sum() >= 30
    assert np.median(np.hypot(got[..., 0], got[..., 1])[on.any(-1)]) > 0.5  # the tangent plane moved with the centre
    assert (plain[..., 0:2][~np.isin(want["first"], ms.prims_of(sd, [ms.MIRROR_SPHERE])).any(-1)] == 0).all()


def test_glass_sphere_box_behind_it_moved(pkg, hip, oracle):
    got, plain, want, sd = moved_case(pkg, hip, oracle, {ms.BOX: BOX_MOVE})
    through = (want["n_refr"] > 0).all(-1) & want["valid"].all(-1)
    box = through & np.isin(want["last"], ms.prims_of(sd, [ms.BOX])).all(-1)
    print("[specular motion] glass: %d pixels through the glass, %d of them end on the moved box" % (int(through.sum()), int(box.sum())))
    assert through.sum() >= 30 and box.sum() >= 5
    ex = np.abs(got[..., 0:2][through] - want["motion"][..., 0:2][through]).max()
    assert ex < PX_TOL  # refraction as identity: the box point itself, through whatever mirrors the chain also met
    assert (np.hypot(got[..., 0][box], got[..., 1][box]) > 1).all()
    assert (plain[..., 0:2][np.isin(want["first"], ms.prims_of(sd, [ms.GLASS_SPHERE])).all(-1)] == 0).all()


# ---------------------------------------------------------------- 9. errors
def test_errors(pkg, hip):
    hs = hip.HipScene(ms.mirror_scene(pkg, 8, 8))
    other = ms.camera(pkg, 9, 8)
    for kw in (dict(specular_depth=-1), dict(specular_depth=9), dict(prev_camera=other, specular_depth=2), dict(aov_spp=-1, specular_depth=2),
               dict(aov_spp=65537, specular_depth=2)):
        with pytest.raises(hip.McptError) as e:
            hs.render_motion(**kw)
        assert e.value.code == 1 and "mcpt_render_motion_ex" in str(e.value), kw
    L = hs.L
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    c = np.ascontiguousarray(hs.sd.camera)
    mo = np.zeros((8, 8, 4), f32)
    assert L.mcpt_render_motion_ex(hs.h, p(c), p(c), 1, 4, 8, p(mo)) == 0
    for args in ((None, p(c), p(c), 1, 4, 2, p(mo)), (hs.h, None, p(c), 1, 4, 2, p(mo)), (hs.h, p(c), None, 1, 4, 2, p(mo)), (hs.h, p(c), p(c), 1, 4, 2, None)):
        assert L.mcpt_render_motion_ex(*args) == 1
    assert bits_equal(hs.render_motion(specular_depth=2), hs.render_motion(specular_depth=2))  # and the scene still works
    hs.close()
