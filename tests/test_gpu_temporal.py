"""Temporal reuse on the GPU (include/mcpt.h: mcpt_scene_snapshot, mcpt_render_motion, mcpt_temporal_blend): the blend kernel gives the
bits of the CPU build of csrc/mcpt_temporal.h; the motion pass follows its definition (a float64 restatement from the library's own camera
rays and hits and mcpt_transform_triangles) for a static scene, a moved mesh, a moved sphere and a panned camera, with the host and the
device builders; the snapshot's semantics; accumulation over a static and over a moving sequence; the argument checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import (KINDS, SHAPES, bits_equal, blend_case, build_driver, host_blend, numpy_blend, project_f64)  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
# cornell_demo, Scene::Add order: floor, short box, tall box, left, right, light, glass sphere, plastic sphere, mirror sphere
SHORT, GLASS_SPHERE = 1, 6
PX_TOL = 1e-2      # pixels: 100 x the float32 round-off of a projection at these widths, 100 x below a one-pixel error
DEPTH_TOL = 1e-4   # relative: the same round-off argument (a few float32 operations on coordinates of a few hundred units)


def translate(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], f32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("tp_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


# ---------------------------------------------------------------- 1. the blend kernel against the CPU build
@pytest.mark.parametrize("shape", SHAPES + [(64, 64)])
@pytest.mark.parametrize("kind", KINDS)
def test_blend_device_equals_host_build(hip, tiny, driver, kind, shape):
    H, W = shape
    args, opts = blend_case(kind, H, W)
    got, got_len = tiny.temporal_blend(*args, **opts)
    want, want_len = host_blend(driver, hip, *args, **opts)
    assert bits_equal(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(got_len, want_len)


# ---------------------------------------------------------------- the float64 restatement of the motion pass
def scene_geometry(pkg, hip, sd, xf):
    """(vertices[n_tri, 3, 3], centres[n_obj, 3]) in float64 of the scene with the transforms xf = {object: 3x4} applied by the library's
    own host rule (mcpt_transform_triangles)."""
    tris, centres = sd.triangles.copy(), sd.objects["center"].copy()
    for o, m in xf.items():
        if sd.objects["kind"][o] == 0:
            a, n = int(sd.objects["first_tri"][o]), int(sd.objects["n_tri"][o])
            tris[a:a + n] = hip.transform_triangles(m, np.ascontiguousarray(tris[a:a + n]))
        else:
            one = np.zeros(1, pkg.scenes.TRI_DTYPE)
            one["v0"][0] = centres[o]
            centres[o] = hip.transform_triangles(m, one)["v0"][0]
    return np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).astype(np.float64), centres.astype(np.float64)


def prims_of(sd, objects):
    out = []
    for o in objects:
        if sd.objects["kind"][o] == 0:
            out.extend(range(int(sd.objects["first_tri"][o]), int(sd.objects["first_tri"][o] + sd.objects["n_tri"][o])))
        else:
            out.append(len(sd.triangles) + o)
    return np.array(out, np.int64)


def motion_f64(pkg, hip, hs, sd, cam, prev_cam, cur_xf, prev_xf, seed=1, spp=4):
    """The motion records of include/mcpt.h in float64 from mcpt_camera_rays + mcpt_intersect on the live scene (whose transforms are
    cur_xf; the snapshot was taken under prev_xf).  Returns (motion[H, W, 4], prim[H, W, spp])."""
    W, H = int(cam["width"]), int(cam["height"])
    n_px = W * H
    pix, smp = np.repeat(np.arange(n_px), spp), np.tile(np.arange(spp), n_px)
    o, d = hs.camera_rays(pix, smp, seed=seed, camera=cam)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    n_tri = len(sd.triangles)
    p_cur = o.astype(np.float64) + d.astype(np.float64) * np.where(hit, t, 0.0)[:, None]
    p_prev = p_cur.copy()
    Vc, Cc = scene_geometry(pkg, hip, sd, cur_xf)
    Vp, Cp = scene_geometry(pkg, hip, sd, prev_xf)
    tr = hit & (prim < n_tri)
    k = prim[tr]
    v0, e1, e2 = Vc[k, 0], Vc[k, 1] - Vc[k, 0], Vc[k, 2] - Vc[k, 0]
    r = p_cur[tr] - v0
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    d1, d2 = (r * e1).sum(1), (r * e2).sum(1)
    det = a * c - b * b
    u, v = (c * d1 - b * d2) / det, (a * d2 - b * d1) / det
    p_prev[tr] = Vp[k, 0] + (Vp[k, 1] - Vp[k, 0]) * u[:, None] + (Vp[k, 2] - Vp[k, 0]) * v[:, None]
    sp = hit & (prim >= n_tri)
    p_prev[sp] = p_cur[sp] + (Cp[prim[sp] - n_tri] - Cc[prim[sp] - n_tri])
    xy_c, z_c = project_f64(cam, p_cur)
    xy_p, z_p = project_f64(prev_cam, p_prev)
    valid = hit & (z_c > 0) & (z_p > 0)
    rec = np.zeros((n_px * spp, 4))
    rec[valid, 0:2] = (xy_p - xy_c)[valid]
    rec[valid, 2] = np.linalg.norm(p_prev - np.asarray(prev_cam["position"], np.float64).reshape(3), axis=1)[valid]
    rec[valid, 3] = 1
    rec = rec.reshape(n_px, spp, 4)
    n = rec[..., 3].sum(1)
    out = np.zeros((n_px, 4))
    out[:, 0:3] = rec[..., 0:3].sum(1) / np.maximum(n, 1)[:, None]
    out[:, 3] = n / spp
    return out.reshape(H, W, 4), prim.reshape(H, W, spp)


def assert_motion_close(got, want, what=""):
    ex = np.abs(got[..., 0:2] - want[..., 0:2]).max()
    ez = (np.abs(got[..., 2] - want[..., 2]) / np.maximum(want[..., 2], 1.0)).max()
    print("%s: max |dx, dy error| = %.3g px, max relative prev_depth error = %.3g" % (what, ex, ez))
    assert np.array_equal(got[..., 3], want[..., 3].astype(f32)), what
    assert ex < PX_TOL, (what, ex)
    assert ez < DEPTH_TOL, (what, ez)


# ---------------------------------------------------------------- 2. static scene, same camera
def test_static_scene_has_zero_motion(pkg, hip):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    hs = hip.HipScene(sd)
    aov = hs.render_aovs(aov_spp=4, seed=1)
    assert (aov[..., 7] > 0).any()
    for snap in (False, True):
        if snap:
            hs.snapshot()
        m = hs.render_motion(seed=1, aov_spp=4)
        assert m.shape == (48, 48, 4)
        assert (m[..., 0] == 0).all() and (m[..., 1] == 0).all(), snap
        assert bits_equal(m[..., 3], aov[..., 7]), snap
        cov = aov[..., 7] > 0
        rel = np.abs(m[..., 2][cov].astype(np.float64) - aov[..., 6][cov]) / aov[..., 6][cov]
        print("static, snapshot %s: max relative |prev_depth - AOV depth| = %.3g" % (snap, rel.max()))
        assert rel.max() < DEPTH_TOL
        assert (m[..., 2][~cov] == 0).all()
    # aov_spp 0 means 4
    assert bits_equal(hs.render_motion(seed=1, aov_spp=0), m)
    hs.close()


# ---------------------------------------------------------------- 3. one moved object
MOVE = translate(30, 0, -20)
_moved = {}


def moved_result(pkg, hip, obj, builder):
    """(device motion, float64 motion, per-sample primitive ids) of: snapshot, then `obj` translated by MOVE; computed once per case."""
    key = (obj, builder)
    if key not in _moved:
        sd = pkg.scenes.cornell_demo(48, 48, 4)
        hs = hip.HipScene(sd, builder=builder)
        hs.snapshot()
        info = hs.update([(obj, MOVE)])
        assert info["path"] == (1 if builder == "ploc" else 0)
        got = hs.render_motion(seed=1, aov_spp=4)
        want, prim = motion_f64(pkg, hip, hs, sd, sd.camera, sd.camera, {obj: MOVE}, {})
        hs.close()
        _moved[key] = (got, want, prim, sd)
    return _moved[key]


@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("obj", [SHORT, GLASS_SPHERE], ids=["short_box", "glass_sphere"])
def test_one_moved_object(pkg, hip, obj, builder):
    got, want, prim, sd = moved_result(pkg, hip, obj, builder)
    assert_motion_close(got, want, "object %d, %s" % (obj, builder))
    on_moved = np.isin(prim, prims_of(sd, [obj]))
    touched = on_moved.any(-1)
    assert touched.sum() > 50
    assert (got[..., 0:2][~touched] == 0).all()  # only unmoved primitives (or nothing) seen: exactly zero
    # the object went 30 along +x, the camera's left, i.e. towards smaller i: its pixels came from larger i
    full = on_moved.all(-1)
    assert full.sum() > 20 and (got[..., 0][full] > 1).all()
    # the two builders agree within the same bound
    other = moved_result(pkg, hip, obj, "sah" if builder == "ploc" else "ploc")[0]
    assert np.array_equal(got[..., 3], other[..., 3])
    assert np.abs(got[..., 0:2] - other[..., 0:2]).max() < PX_TOL
    assert (np.abs(got[..., 2] - other[..., 2]) / np.maximum(other[..., 2], 1)).max() < DEPTH_TOL


# ---------------------------------------------------------------- 4. camera pan
def test_camera_pan(pkg, hip):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    hs = hip.HipScene(sd)
    a = np.radians(2.0)
    eye = np.array([278, 273, -800.0])
    fwd = np.array([np.sin(a), 0, np.cos(a)]) * 800
    prev = pkg.scenes.make_camera(48, 48, 40, eye, eye + fwd, (0, 1, 0), focal_distance=900, aperture_radius=40)
    got = hs.render_motion(prev_camera=prev, seed=1, aov_spp=4)
    want, _ = motion_f64(pkg, hip, hs, sd, sd.camera, prev, {}, {})
    assert_motion_close(got, want, "2 degree pan")
    aov = hs.render_aovs(aov_spp=4, seed=1)
    assert bits_equal(got[..., 3], aov[..., 7])  # every hit is valid, also those that leave the previous frustum
    ii = np.arange(48)[None, :] + got[..., 0]
    off = (got[..., 3] > 0) & ((ii < -0.5) | (ii > 47.5))
    assert off.sum() > 10
    assert np.abs(got[..., 0][got[..., 3] > 0]).min() > 1  # 2 degrees of a 40 degree field at 48 px: a few pixels everywhere
    # a previous camera that looks the other way: q.z <= 0 for every point, nothing is valid
    back = pkg.scenes.make_camera(48, 48, 40, eye, eye - fwd, (0, 1, 0))
    none = hs.render_motion(prev_camera=back, seed=1, aov_spp=4)
    assert (none == 0).all()
    hs.close()


# ---------------------------------------------------------------- 5. snapshot semantics
def test_snapshot_semantics(pkg, hip):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    hs = hip.HipScene(sd)
    T1, T2 = translate(30, 0, -20), translate(-25, 10, 15)
    hs.snapshot()
    hs.update([(SHORT, T1)])
    m1 = hs.render_motion()
    assert (m1[..., 0:2] != 0).any()
    # an update between two motion calls, without a new snapshot: the snapshot still holds the creation-time geometry
    hs.update([(SHORT, T2)])
    m2 = hs.render_motion()
    want, _ = motion_f64(pkg, hip, hs, sd, sd.camera, sd.camera, {SHORT: T2}, {})
    assert_motion_close(m2, want, "second update, old snapshot")
    assert not bits_equal(m1, m2)
    hs.update([(SHORT, T1)])
    assert bits_equal(hs.render_motion(), m1)
    # a second snapshot after the update: zero motion again
    hs.snapshot()
    m3 = hs.render_motion()
    assert (m3[..., 0:2] == 0).all() and bits_equal(m3[..., 3], m1[..., 3])
    # ... and from there the motion is relative to T1
    hs.update([(SHORT, T2)])
    m4 = hs.render_motion()
    want, _ = motion_f64(pkg, hip, hs, sd, sd.camera, sd.camera, {SHORT: T2}, {SHORT: T1})
    assert_motion_close(m4, want, "snapshot under T1, scene under T2")
    hs.close()


# ---------------------------------------------------------------- 6. static accumulation
def test_static_accumulation(pkg, hip):
    """Eight frames of a static scene.  Everywhere the result is the numpy restatement of the blend; on every pixel the rule of
    include/mcpt.h keeps in all frames so far it is the plain recurrence h += (c - h) * (1 / N) and len counts the frames.  (A silhouette
    pixel's mean depth changes with the seed's jitter, and at 64 x 64 so does that of a floor or side-wall pixel seen at a grazing angle,
    whose footprint spans several per cent of its depth: such a pixel restarts.  That is the rule, not an error.)  With zero motion a pixel
    reads one tap of weight 1, itself, so the kept set follows from the inputs alone: valid > 0, finite colours, and the depth test in
    float32 exactly as the blend makes it."""
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd)
    H = W = 64
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    prev_depth = np.zeros((H, W), f32)
    stable = np.ones((H, W), bool)
    ref = first = None
    for k in range(8):
        c, _ = hs.render(spp=4, seed=k + 1)
        aov = hs.render_aovs(aov_spp=4, seed=k + 1)
        motion = hs.render_motion(seed=k + 1, aov_spp=4)
        assert (motion[..., 0:2] == 0).all()
        want, want_len = numpy_blend(c, motion, hist, prev_depth, length, max_history=32)
        hist, length = hs.temporal_blend(c, motion, hist, prev_depth, length, max_history=32)
        assert bits_equal(hist, want) and bits_equal(length, want_len), k
        if k == 0:
            ref, first = c.copy(), c.copy()  # (no history yet: every pixel starts with len 1)
        else:
            zp = motion[..., 2]
            assert zp.dtype == f32 and prev_depth.dtype == f32
            stable &= (motion[..., 3] > 0) & np.isfinite(c).all(-1) & np.isfinite(ref).all(-1) & (np.abs(prev_depth - zp) <= f32(0.02) * zp)
            ref = ref + (c - ref) * (f32(1) / f32(k + 1))
        assert ref.dtype == f32 and bits_equal(hist[stable], ref[stable]), k
        assert (length[stable] == k + 1).all(), k
        assert (length[motion[..., 3] == 0] == 1).all()
        prev_depth = aov[..., 6].copy()
    covered = motion[..., 3] > 0
    print("static accumulation: %.1f %% of the pixels (%d of %d covered ones) keep their history through all 8 frames"
          % (100 * stable.mean(), int(stable.sum()), int(covered.sum())))
    assert stable.sum() >= 1000  # (the back wall alone, seen head-on, is about a third of the 4096 pixels)
    truth, _ = hs.render(spp=2048, seed=1000)
    mse_one = float(((first.astype(np.float64) - truth) ** 2).mean())
    mse_acc = float(((hist.astype(np.float64) - truth) ** 2).mean())
    print("static accumulation: MSE of one 4-spp frame %.4g, of 8 blended frames %.4g (ratio %.3f)" % (mse_one, mse_acc, mse_acc / mse_one))
    assert mse_acc < 0.5 * mse_one
    hs.close()


# ---------------------------------------------------------------- 7. moving accumulation
def centre_prims(hs, cam):
    """The primitive id seen through every pixel centre (a pinhole ray, the camera ray without its jitter)."""
    W, H = int(cam["width"]), int(cam["height"])
    M = np.asarray(cam["orientation"], np.float64).reshape(3, 3)
    scale = np.tan(np.radians(float(cam["fov"]) * 0.5))
    j, i = np.mgrid[0:H, 0:W]
    x = (1 - 2 * (i + 0.5) / W) * (W / H) * scale
    y = (1 - 2 * (j + 0.5) / H) * scale
    d = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)) @ M.T
    o = np.broadcast_to(np.asarray(cam["position"], np.float64), d.shape)
    return hs.intersect(o, d)[1].reshape(H, W)


def erode(mask, r):
    out = mask.copy()
    H, W = mask.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sh = np.zeros_like(mask)
            sh[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] = mask[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
            out &= sh
    return out


def front_face(sd):
    """The two triangles of the short box whose common normal faces the camera most directly (the camera looks along +z)."""
    a, n = int(sd.objects["first_tri"][SHORT]), int(sd.objects["n_tri"][SHORT])
    t = sd.triangles[a:a + n]
    nrm = np.cross(t["v1"] - t["v0"], t["v2"] - t["v0"]).astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    front = np.argsort(nrm[:, 2])[:2]  # (the camera looks along +z: the most negative n.z)
    assert np.allclose(nrm[front[0]], nrm[front[1]], atol=1e-4) and nrm[front[0], 2] < -0.9
    return a + front


def test_moving_accumulation(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd)
    H = W = 64
    cam = sd.camera
    face = front_face(sd)
    box = prims_of(sd, [SHORT])
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    prev_depth = np.zeros((H, W), f32)
    chain = prev_box = None
    n_uncovered = 0
    for k in range(4):
        hs.snapshot()
        hs.update([(SHORT, translate(-32.0 * k, 0, 0))])  # about 3 px per frame at this depth, away from the glass sphere in front
        c, _ = hs.render(spp=4, seed=k + 1)
        aov = hs.render_aovs(aov_spp=4, seed=k + 1)
        motion = hs.render_motion(seed=k + 1, aov_spp=4)
        hist, length = hs.temporal_blend(c, motion, hist, prev_depth, length)
        assert np.isfinite(hist[np.isfinite(c).all(-1)]).all(), k
        centre = centre_prims(hs, cam)
        on_face = erode(np.isin(centre, face), 2)
        if k == 0:
            chain = on_face
            assert (length[motion[..., 3] > 0] == 1).all()
        else:
            # pixels on the front face whose four taps were, in the previous frame, pixels of the chain
            jj, ii = np.mgrid[0:H, 0:W]
            x0 = np.floor(ii + motion[..., 0]).astype(int)
            y0 = np.floor(jj + motion[..., 1]).astype(int)
            ok = on_face & (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)
            x0, y0 = x0.clip(0, W - 2), y0.clip(0, H - 2)
            chain = ok & chain[y0, x0] & chain[y0, x0 + 1] & chain[y0 + 1, x0] & chain[y0 + 1, x0 + 1]
            assert np.abs(motion[..., 0][on_face]).min() > 2 and np.abs(motion[..., 0][on_face]).max() < 4.5, k
        assert (length[chain] == k + 1).all(), (k, np.unique(length[chain]))
        # pixels the box uncovered: on the box in the previous frame, on what lies behind it now, at another depth
        o, d = hs.camera_rays(np.repeat(np.arange(H * W), 4), np.tile(np.arange(4), H * W), seed=k + 1, camera=cam)
        sample_box = np.isin(hs.intersect(o, d)[1], box).reshape(H, W, 4)
        if k > 0:
            gone = prev_box.all(-1) & ~sample_box.any(-1) & (motion[..., 3] > 0)
            gone &= np.abs(prev_depth - motion[..., 2]) > 0.05 * motion[..., 2]
            n_uncovered += int(gone.sum())
            assert (length[gone] == 1).all() and bits_equal(hist[gone], c[gone]), k
        prev_box = sample_box
        prev_depth = aov[..., 6].copy()
    print("moving accumulation: %d chain pixels in the last frame, %d uncovered pixels over the sequence" % (int(chain.sum()), n_uncovered))
    assert chain.sum() >= 50
    assert n_uncovered >= 10
    hs.close()


# ---------------------------------------------------------------- 8. errors
def test_errors(pkg, hip, tiny):
    cam = tiny.sd.camera
    other = pkg.scenes.make_camera(9, 8, 40, (278, 273, -800), (278, 273, 0))
    for kw in (dict(prev_camera=other), dict(aov_spp=-1), dict(aov_spp=65537)):
        with pytest.raises(hip.McptError) as e:
            tiny.render_motion(**kw)
        assert e.value.code == 1 and "mcpt_render_motion" in str(e.value), kw
    H = W = 8
    a = [np.zeros((H, W, 3), f32), np.zeros((H, W, 4), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)]
    for kw in (dict(depth_tol=-0.02), dict(depth_tol=float("nan")), dict(max_history=-3), dict(max_history=5000)):
        with pytest.raises(hip.McptError) as e:
            tiny.temporal_blend(*a, **kw)
        assert e.value.code == 1 and "mcpt_temporal_blend" in str(e.value), kw
    import ctypes as C
    L = tiny.L
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out, out_len = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    o = hip.temporal_opts()
    o.reserved[3] = 1
    assert L.mcpt_temporal_blend(tiny.h, W, H, *[p(x) for x in a], C.byref(o), p(out), p(out_len)) == 1
    ok = hip.temporal_opts()
    full = [tiny.h, W, H] + [p(x) for x in a] + [C.byref(ok), p(out), p(out_len)]
    assert L.mcpt_temporal_blend(*full) == 0
    for k in (0, 3, 4, 5, 6, 7, 8, 9, 10):
        args = list(full)
        args[k] = None
        assert L.mcpt_temporal_blend(*args) == 1, k
    c = np.ascontiguousarray(cam)
    mo = np.zeros((H, W, 4), f32)
    assert L.mcpt_render_motion(tiny.h, p(c), p(c), 1, 4, p(mo)) == 0
    for args in ((None, p(c), p(c), 1, 4, p(mo)), (tiny.h, None, p(c), 1, 4, p(mo)), (tiny.h, p(c), None, 1, 4, p(mo)), (tiny.h, p(c), p(c), 1, 4, None)):
        assert L.mcpt_render_motion(*args) == 1
    assert L.mcpt_scene_snapshot(None) == 1
    assert L.mcpt_scene_snapshot(tiny.h) == 0
