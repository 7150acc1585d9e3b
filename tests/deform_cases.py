"""Shared by tests/test_scene_deform_cpu.py and tests/test_gpu_scene_deform.py (include/mcpt.h: mcpt_scene_deform): the comparison rules of
tests/test_gpu_scene_update.py (copied, not imported: a test module is nobody's library), the description desc'' a deformed scene must
equal, smooth deformations, the scenes whose meshes sit on the edges of the deformation kernel's waves and blocks, and the float64
restatement of the motion pass for triangles whose vertices moved independently."""
import dataclasses

import numpy as np

f32 = np.float32
INFO_FIELDS = ("n_nodes", "bvh_height", "quantised", "lds_resident", "n_lights", "n_prims")
DEVICE_BUILDERS = ("lbvh", "ploc")
# cornell_demo, Scene::Add order: floor, short box, tall box, left, right, light, glass sphere, plastic sphere, mirror sphere
FLOOR, SHORT, TALL, LIGHT, GLASS_SPHERE, PLASTIC_SPHERE, MIRROR_SPHERE = 0, 1, 2, 5, 6, 7, 8
PX_TOL = 1e-2     # tests/test_gpu_temporal.py: 100 x the float32 round-off of a projection at these widths, 100 x below a one-pixel error
DEPTH_TOL = 1e-4  # relative: a few float32 operations on coordinates of a few hundred units


def translate(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], f32)


def rotate_y(angle, centre, shift=(0, 0, 0)):
    """Rotation about the vertical axis through `centre`, then a translation."""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = np.asarray(centre, float) - R @ np.asarray(centre, float) + np.asarray(shift, float)
    return np.concatenate([R, t[:, None]], axis=1).astype(f32)


# ---------------------------------------------------------------- positions and desc''
def positions_of(tris):
    """(n_tri, 3, 3) float32: v0, v1, v2 of each triangle."""
    return np.ascontiguousarray(np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1), dtype=f32)


def object_positions(sd, o):
    a, n = int(sd.objects["first_tri"][o]), int(sd.objects["n_tri"][o])
    return positions_of(sd.triangles[a:a + n])


def wave(P, amp=14.0, freq=0.021, phase=0.0):
    """A smooth displacement that is a function of the position alone, so corners shared by several triangles stay shared."""
    P = np.asarray(P, np.float64)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    D = np.stack([np.sin(freq * y + phase) + 0.5 * np.sin(freq * z), 0.4 * np.sin(freq * (x + z) + 2 * phase), np.cos(freq * (x - y) + phase)], -1)
    return np.ascontiguousarray(P + amp * D, dtype=f32)


def deformed_scene(pkg, hip, sd, bases, transforms=None):
    """desc'': `bases` maps object -> the latest positions given, `transforms` object -> its current 3x4 matrix; the library's own host
    rules apply both (mcpt_deform_triangles, then mcpt_transform_triangles)."""
    tris, objs = sd.triangles.copy(), sd.objects.copy()
    for o, P in bases.items():
        a, n = int(objs["first_tri"][o]), int(objs["n_tri"][o])
        tris[a:a + n] = hip.deform_triangles(np.ascontiguousarray(P, f32), np.ascontiguousarray(tris[a:a + n]))
    for o, m in (transforms or {}).items():
        if objs["kind"][o] == 0:
            a, n = int(objs["first_tri"][o]), int(objs["n_tri"][o])
            tris[a:a + n] = hip.transform_triangles(m, np.ascontiguousarray(tris[a:a + n]))
        else:  # the centre goes through the same host function as a vertex
            one = np.zeros(1, pkg.scenes.TRI_DTYPE)
            one["v0"][0] = objs["center"][o]
            objs["center"][o] = hip.transform_triangles(m, one)["v0"][0]
    return dataclasses.replace(sd, triangles=tris, objects=objs)


# ---------------------------------------------------------------- device buffers without torch
class DeviceArray:
    """A float32 array in the memory of the current device, allocated through the HIP runtime the library itself is linked to (found among
    this process's loaded libraries, so no second runtime is loaded).  It exposes __cuda_array_interface__, one of the forms
    HipScene.deform takes.  torch is not used here on purpose: it carries a HIP runtime of its own and must be imported before the
    library (bench.py's order), which a test process that has already loaded the library cannot do -- tests/deform_torch_child.py does."""

    _rt = None

    @classmethod
    def runtime(cls):
        if cls._rt is None:
            import ctypes as C
            paths = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
            assert paths, "the HIP runtime is not loaded: load the library first"
            rt = C.CDLL(paths[0])
            rt.hipMalloc.argtypes, rt.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
            rt.hipMemcpy.argtypes, rt.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
            rt.hipFree.argtypes, rt.hipFree.restype = [C.c_void_p], C.c_int
            cls._rt = rt
        return cls._rt

    def __init__(self, host):
        import ctypes as C
        host = np.ascontiguousarray(host, dtype=f32)
        rt, ptr = self.runtime(), C.c_void_p()
        assert rt.hipMalloc(C.byref(ptr), max(host.nbytes, 4)) == 0
        self.ptr, self.shape = ptr.value, host.shape
        assert rt.hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0  # hipMemcpyHostToDevice; blocking
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": "<f4", "data": (self.ptr, False), "strides": None, "version": 3}

    def free(self):
        if self.ptr:
            self.runtime().hipFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------- the comparison rules
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_frame(a, b, device_built, what=""):
    differing = int((~same_bits(a, b)).sum())
    assert differing <= (3 if device_built else 0), (what, differing)


def assert_same_hits(upd, fresh, o, d):
    ta, pa = upd.intersect(o, d)
    tb, pb = fresh.intersect(o, d)
    assert np.array_equal(pa, pb), "primitive ids differ on %d rays" % int((pa != pb).sum())
    assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    return pa


def assert_same_info(upd, fresh):
    a, b = upd.info(), fresh.info()
    assert [a[k] for k in INFO_FIELDS] == [b[k] for k in INFO_FIELDS], (a, b)


def assert_same_tree(upd, fresh):
    (ia, ba, ca, qa), (ib, bb, cb, qb) = upd.dump_bvh(), fresh.dump_bvh()
    for k in ia:
        assert np.array_equal(np.asarray(ia[k]), np.asarray(ib[k])), k
    assert ba.tobytes() == bb.tobytes() and ca.tobytes() == cb.tobytes()
    assert (qa is None) == (qb is None) and (qa is None or qa.tobytes() == qb.tobytes())


def assert_equals_fresh(hs, fresh, o, d, device_built, spp=4, seed=5, what=""):
    """Scene info, hits on the rays (o, d), a frame and, for the host builders, the tree dump.  Returns the primitive ids."""
    assert_same_info(hs, fresh)
    if not device_built:
        assert_same_tree(hs, fresh)
    prim = assert_same_hits(hs, fresh, o, d)
    assert_same_frame(hs.render(spp=spp, seed=seed)[0], fresh.render(spp=spp, seed=seed)[0], device_built, what)
    return prim


def camera_and_random_rays(hs, W, H, spp, lo, hi, n_random=6000, seed=3):
    """The W x H x spp camera rays plus random rays with origins in the box [lo, hi]."""
    pix = np.repeat(np.arange(W * H, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), W * H)
    o, d = hs.camera_rays(pix, smp, seed=7)
    rng = np.random.default_rng(seed)
    o2 = rng.uniform(lo, hi, (n_random, 3)).astype(f32)
    d2 = rng.normal(0, 1, (n_random, 3))
    d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(f32)
    return np.concatenate([o, o2]), np.concatenate([d, d2])


def cornell_rays(hs, W, H, spp, n_random=6000):
    return camera_and_random_rays(hs, W, H, spp, [10, 10, -700], [540, 540, 540], n_random)


# ---------------------------------------------------------------- scenes on the kernel's edges
STRIP_SIZES = (1, 63, 64, 65, 257)  # one lane; a wave less one; a wave; a wave and one; more than a 256-lane block


def strip(pkg, n, y, z, step=3.0, height=8.0):
    """A zigzag strip of n triangles in the plane of constant z: triangle k spans the points k, k + 1, k + 2."""
    k = np.arange(n + 2)
    pts = np.stack([k * step - 0.5 * step * (n + 1), y + height * (k % 2), np.full(n + 2, z)], -1).astype(f32)
    t = np.zeros(n, pkg.scenes.TRI_DTYPE)
    t["v0"], t["v1"], t["v2"] = pts[:-2], pts[1:-1], pts[2:]
    t["t0"], t["t1"], t["t2"] = pts[:-2, :2] * f32(0.01), pts[1:-1, :2] * f32(0.01), pts[2:, :2] * f32(0.01)
    return t


def strips_scene(pkg, W=64, H=64):
    """Objects 0..4: strips of STRIP_SIZES triangles; 5: a floor; 6: a light.  So the five strips deformed in one call are segments of
    1, 63, 64, 65 and 257 lanes: segment borders inside a wave, on a wave's edge, and across the 256-lane block."""
    s = pkg.scenes
    P = s.material_presets()
    b = s._Builder()
    for i, n in enumerate(STRIP_SIZES):
        b.add_mesh(strip(pkg, n, y=-40.0 + 20.0 * i, z=4.0 * i), b.material("rough_plastic", P["rough_plastic"]))
    fl = np.zeros(2, s.TRI_DTYPE)
    fl["v0"], fl["v1"], fl["v2"] = [(-500, -60, -100)] * 2, [(500, -60, 300), (500, -60, -100)], [(-500, -60, 300), (500, -60, 300)]
    b.add_mesh(fl, b.material("rough_white_conductor", P["rough_white_conductor"]))
    lt = np.zeros(2, s.TRI_DTYPE)
    lt["v0"], lt["v1"], lt["v2"] = [(-60, 120, -60)] * 2, [(60, 120, -60), (60, 120, 60)], [(60, 120, 60), (-60, 120, 60)]
    b.add_mesh(lt, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(20, 20, 20))))
    cam = s.make_camera(W, H, 60, (0, 10, -420), (0, 10, 0))
    return b.finish(camera=cam, rr_rate=0.5, spp=4, name="strips")


def scene_65(pkg):
    """One triangle more than the LDS-resident kernels hold (kSmallTris = 64): 63 triangles and a two-triangle light (the boundary scene of
    tests/test_gpu_scene_update.py)."""
    s = pkg.scenes
    P = s.material_presets()
    b = s._Builder()
    rng = np.random.default_rng(1)
    tri = np.zeros(63, s.TRI_DTYPE)
    base = rng.uniform(-20, 20, (63, 3)).astype(f32)
    tri["v0"], tri["v1"], tri["v2"] = base, base + rng.normal(0, 4, (63, 3)).astype(f32), base + rng.normal(0, 4, (63, 3)).astype(f32)
    b.add_mesh(tri, b.material("rough_plastic", P["rough_plastic"]))
    lt = np.zeros(2, s.TRI_DTYPE)
    lt["v0"], lt["v1"], lt["v2"] = [(-10, 40, -10)] * 2, [(10, 40, -10), (10, 40, 10)], [(10, 40, 10), (-10, 40, 10)]
    b.add_mesh(lt, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(20, 20, 20))))
    cam = s.make_camera(48, 32, 60, (0, 0, -70), (0, 0, 0))
    return b.finish(camera=cam, rr_rate=0.5, spp=2, name="65 triangles")


def quad_scene(pkg, W=64, H=64):
    """Object 0: a 4 x 4 grid of quads (32 triangles) facing the camera; 1: a floor; 2: a light; 3: a sphere beside the grid."""
    s = pkg.scenes
    P = s.material_presets()
    b = s._Builder()
    g = np.linspace(-60, 60, 5)
    X, Y = np.meshgrid(g, g, indexing="xy")
    pt = np.stack([X, Y, np.zeros_like(X)], -1).astype(f32)
    tris = []
    for j in range(4):
        for i in range(4):
            a, bb, c, d = pt[j, i], pt[j, i + 1], pt[j + 1, i + 1], pt[j + 1, i]
            tris += [(a, c, bb), (a, d, c)]  # normals towards -z, the camera's side
    q = np.zeros(len(tris), s.TRI_DTYPE)
    q["v0"], q["v1"], q["v2"] = [t[0] for t in tris], [t[1] for t in tris], [t[2] for t in tris]
    b.add_mesh(q, b.material("rough_plastic", P["rough_plastic"]))
    fl = np.zeros(2, s.TRI_DTYPE)
    fl["v0"], fl["v1"], fl["v2"] = [(-300, -80, -200)] * 2, [(300, -80, 200), (300, -80, -200)], [(-300, -80, 200), (300, -80, 200)]
    b.add_mesh(fl, b.material("rough_white_conductor", P["rough_white_conductor"]))
    lt = np.zeros(2, s.TRI_DTYPE)
    lt["v0"], lt["v1"], lt["v2"] = [(-40, 150, -140)] * 2, [(40, 150, -140), (40, 150, -60)], [(40, 150, -60), (-40, 150, -60)]
    b.add_mesh(lt, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(30, 30, 30))))
    b.add_sphere((110, -40, 0), 30, b.material("clear_rough_plastic", P["clear_rough_plastic"]))
    cam = s.make_camera(W, H, 50, (0, 0, -300), (0, 0, 0))
    return b.finish(camera=cam, rr_rate=0.5, spp=4, name="quad")


# ---------------------------------------------------------------- the motion pass in float64 (tests/test_temporal_cpu.py, test_gpu_temporal.py)
def _scalar(v):
    return np.asarray(v).reshape(-1)[0]


def camera_f64(cam):
    """(eye, orientation 3x3, scale, aspect) of a camera record in float64, the scale from the float32 expression of the camera rays."""
    W, H = _scalar(cam["width"]), _scalar(cam["height"])
    rad = f32(np.float64(f32(_scalar(cam["fov"])) * f32(0.5) * f32(3.141592653589793)) / 180.0)
    scale = np.float64(f32(np.tan(np.float64(rad))))
    aspect = np.float64(f32(W) / f32(H))
    return np.asarray(cam["position"], np.float64).reshape(3), np.asarray(cam["orientation"], np.float64).reshape(3, 3), scale, aspect


def project_f64(cam, p):
    """proj(cam, p) of include/mcpt.h in float64: (xy[n, 2], q.z[n])."""
    eye, M, scale, aspect = camera_f64(cam)
    W, H = _scalar(cam["width"]), _scalar(cam["height"])
    q = (np.asarray(p, np.float64) - eye) @ M  # q = M^T (p - eye)
    with np.errstate(all="ignore"):
        sx = (1 - (q[:, 0] / q[:, 2]) / (aspect * scale)) * (0.5 * W)
        sy = (1 - (q[:, 1] / q[:, 2]) / scale) * (0.5 * H)
    return np.stack([sx, sy], -1), q[:, 2]


def motion_f64(hs, sd, V_cur, V_prev, seed=1, spp=4):
    """The motion records of include/mcpt.h in float64 from mcpt_camera_rays + mcpt_intersect on the live scene: a hit's barycentrics on
    the live triangle V_cur[prim] are evaluated on the snapshot's triangle V_prev[prim] ([n_tri, 3, 3] each; spheres do not move here).
    Returns (motion[H, W, 4], prim[H, W, spp])."""
    cam = sd.camera
    W, H = int(_scalar(cam["width"])), int(_scalar(cam["height"]))
    n_px = W * H
    pix, smp = np.repeat(np.arange(n_px), spp), np.tile(np.arange(spp), n_px)
    o, d = hs.camera_rays(pix, smp, seed=seed, camera=cam)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    n_tri = len(sd.triangles)
    p_cur = o.astype(np.float64) + d.astype(np.float64) * np.where(hit, t, 0.0)[:, None]
    p_prev = p_cur.copy()
    Vc, Vp = np.asarray(V_cur, np.float64), np.asarray(V_prev, np.float64)
    tr = hit & (prim < n_tri)
    k = prim[tr]
    v0, e1, e2 = Vc[k, 0], Vc[k, 1] - Vc[k, 0], Vc[k, 2] - Vc[k, 0]
    r = p_cur[tr] - v0
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    d1, d2 = (r * e1).sum(1), (r * e2).sum(1)
    det = a * c - b * b
    u, v = (c * d1 - b * d2) / det, (a * d2 - b * d1) / det
    p_prev[tr] = Vp[k, 0] + (Vp[k, 1] - Vp[k, 0]) * u[:, None] + (Vp[k, 2] - Vp[k, 0]) * v[:, None]
    xy_c, z_c = project_f64(cam, p_cur)
    xy_p, z_p = project_f64(cam, p_prev)
    valid = hit & (z_c > 0) & (z_p > 0)
    rec = np.zeros((n_px * spp, 4))
    rec[valid, 0:2] = (xy_p - xy_c)[valid]
    rec[valid, 2] = np.linalg.norm(p_prev - np.asarray(cam["position"], np.float64).reshape(3), axis=1)[valid]
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
