"""A small hand-built scene of mirrors for the tests of specular motion (include/mcpt.h: mcpt_render_motion_ex,
mcpt_sequence_create_motion), and the float64 restatement of a chain's motion record they compare against.

Objects, in Scene::Add order:
  0 FLOOR   a planar mirror, the plane y = 0 (two triangles, silver_mirror, untextured)
  1 BOX     a ROUGH_CONDUCTOR box of 12 triangles standing on it
  2 LIGHT   an emitting quad above
  3 BACK    a second mirror quad, the plane z = 16, at a right angle to the floor, behind the box
  4 MIRROR_SPHERE  a silver_mirror sphere
  5 GLASS_SPHERE   a smooth_glass sphere in front of the box
A constant background, a pinhole camera (no depth of field) that looks down 30 degrees, 48 x 48, 4 feature samples.  About a third of the
frame shows the box's reflection in the floor."""
import ctypes as C

import numpy as np

f32 = np.float32
FLOOR, BOX, LIGHT, BACK, MIRROR_SPHERE, GLASS_SPHERE = range(6)
W = H = 48
SPP = 4
EYE = (0.0, 14.0, -28.0)


def _quad(S, a, b, c, d):
    t = np.zeros(2, S.TRI_DTYPE)
    t[0]["v0"], t[0]["v1"], t[0]["v2"] = a, b, c
    t[1]["v0"], t[1]["v1"], t[1]["v2"] = a, c, d
    return t


def _box(S, lo, hi):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    P = lambda x, y, z: (x, y, z)  # noqa: E731
    faces = [(P(x0, y0, z0), P(x1, y0, z0), P(x1, y1, z0), P(x0, y1, z0)), (P(x0, y0, z1), P(x0, y1, z1), P(x1, y1, z1), P(x1, y0, z1)),
             (P(x0, y0, z0), P(x0, y1, z0), P(x0, y1, z1), P(x0, y0, z1)), (P(x1, y0, z0), P(x1, y0, z1), P(x1, y1, z1), P(x1, y1, z0)),
             (P(x0, y1, z0), P(x1, y1, z0), P(x1, y1, z1), P(x0, y1, z1)), (P(x0, y0, z0), P(x0, y0, z1), P(x1, y0, z1), P(x1, y0, z0))]
    return np.concatenate([_quad(S, *f) for f in faces])


def camera(pkg, width=W, height=H, pan_deg=0.0):
    """The scene's camera: at EYE, 30 degrees down, fov 50; pan_deg turns it about the vertical axis."""
    a = np.radians(pan_deg)
    d = np.array([np.sin(a) * np.cos(np.pi / 6), -0.5, np.cos(a) * np.cos(np.pi / 6)])
    return pkg.scenes.make_camera(width, height, 50, EYE, np.asarray(EYE) + 10 * d, (0, 1, 0))


def corner_camera(pkg):
    """A view past the box into the corner of the floor and the back mirror: floor, back mirror, then the back face of the box."""
    return pkg.scenes.make_camera(W, H, 40, (18, 8, -6), (10, 0, 15), (0, 1, 0))


def mirror_scene(pkg, width=W, height=H):
    S = pkg.scenes
    P = S.material_presets()
    b = S._Builder()
    b.add_mesh(_quad(S, (-20, 0, -20), (20, 0, -20), (20, 0, 20), (-20, 0, 20)), b.material("floor", P["silver_mirror"]))
    b.add_mesh(_box(S, (-10, 0, 2), (10, 24, 12)), b.material("box", S._mat(S.ROUGH_CONDUCTOR, 0.4, (0.6, 0.25, 0.8))))
    b.add_mesh(_quad(S, (-5, 30, -5), (5, 30, -5), (5, 30, 5), (-5, 30, 5)), b.material("light", S._mat(S.ROUGH_CONDUCTOR, emission=S.light_emission(3.9))))
    b.add_mesh(_quad(S, (-20, 0, 16), (20, 0, 16), (20, 24, 16), (-20, 24, 16)), b.material("back", S._mat(S.SMOOTH_CONDUCTOR, 0.001, (0.9, 0.9, 0.8))))
    b.add_sphere((-9, 3, -2), 3, b.material("mirror_sphere", P["silver_mirror"]))
    b.add_sphere((6, 3, -4), 3, b.material("glass", P["smooth_glass"]))
    return b.finish(camera=camera(pkg, width, height), spp=SPP, name="mirrors", background=np.array([0.25, 0.3, 0.4], f32))


def translate(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], f32)


def rotate_z(deg, about=(0.0, 0.0, 0.0)):
    """A rotation about the z axis through `about` (for the floor: an in-plane axis), as a 3 x 4 transform."""
    a = np.radians(deg)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = np.asarray(about, np.float64)
    return np.concatenate([R, (c - R @ c)[:, None]], 1).astype(f32)


def moved_scene(pkg, hip, sd, xf):
    """A SceneData whose objects carry the transforms xf = {object: 3x4}, by the library's host rule (mcpt_transform_triangles): what the live
    scene is after update(xf)."""
    import dataclasses
    tris, objs = sd.triangles.copy(), sd.objects.copy()
    for o, m in xf.items():
        if objs["kind"][o] == 0:
            a, n = int(objs["first_tri"][o]), int(objs["n_tri"][o])
            tris[a:a + n] = hip.transform_triangles(m, np.ascontiguousarray(tris[a:a + n]))
        else:
            one = np.zeros(1, pkg.scenes.TRI_DTYPE)
            one["v0"][0] = objs["center"][o]
            objs["center"][o] = hip.transform_triangles(m, one)["v0"][0]
    return dataclasses.replace(sd, triangles=tris, objects=objs)


def _dot(a, b):  # the kernels' order, float32
    return f32(a[0] * b[0] + f32(a[1] * b[1] + a[2] * b[2]))


def _tri_normals_f32(t):
    e1, e2 = (t["v1"] - t["v0"]).astype(f32), (t["v2"] - t["v0"]).astype(f32)
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(f32)
    z = (c[:, 0] * c[:, 0] + (c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (c / np.sqrt(z)[:, None]).astype(f32)
    return np.where((z > 0)[:, None], n, c)


def _reflect64(x, a, n):
    return x - 2 * n * np.dot(n, x - a)


def _bary64(V, p):
    e1, e2, r = V[1] - V[0], V[2] - V[0], p - V[0]
    a, b, c = e1 @ e1, e1 @ e2, e2 @ e2
    d1, d2 = r @ e1, r @ e2
    det = a * c - b * b
    return (c * d1 - b * d2) / det, (a * d2 - b * d1) / det


def project_f64(cam, p):
    """((sx, sy), q.z) of the points p[n, 3] in float64 by the projection of include/mcpt.h."""
    Wc, Hc = int(cam["width"]), int(cam["height"])
    M = np.asarray(cam["orientation"], np.float64).reshape(3, 3)
    q = (p - np.asarray(cam["position"], np.float64).reshape(3)) @ M
    scale = np.tan(np.radians(float(cam["fov"]) * 0.5))
    with np.errstate(all="ignore"):
        sx = (1 - (q[:, 0] / q[:, 2]) / ((Wc / Hc) * scale)) * (0.5 * Wc)
        sy = (1 - (q[:, 1] / q[:, 2]) / scale) * (0.5 * Hc)
    return np.stack([sx, sy], 1), q[:, 2]


def chain_motion_f64(oracle, tracer, live, prev, cam, prev_cam, depth, seed=1, spp=SPP):
    """The motion records of include/mcpt.h: mcpt_render_motion_ex in float64.  tracer: a HipScene (or an OracleScene) of the scene `live`
    (a SceneData, moved_scene of the transforms the live scene carries), used for camera_rays and intersect; prev: the SceneData the
    snapshot was taken of.  Every bounce is decided as the kernels decide it (float32, the oracle's material functions: the chain of
    tests/test_gpu_specular_aov.py); the planes, the reflections and the projections are float64.
    Returns dict(motion[H, W, 4], first[H, W, spp], last[H, W, spp] primitive ids (-1: none), n_refl, n_refr [H, W, spp],
    valid[H, W, spp], depth[H, W, spp] the summed distance of the chain)."""
    L = oracle.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Wc, Hc = int(cam["width"]), int(cam["height"])
    n_px = Wc * Hc
    N = n_px * spp
    pix, smp = np.repeat(np.arange(n_px, dtype=np.uint32), spp), np.tile(np.arange(spp, dtype=np.uint32), n_px)
    o, d = tracer.camera_rays(pix, smp, seed=seed, camera=cam)
    o, d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
    n_tri = len(live.triangles)
    mats = np.ascontiguousarray(live.materials)
    tri_mat = np.zeros(n_tri, np.int32)
    for ob in live.objects:
        if ob["kind"] == 0:
            tri_mat[ob["first_tri"]:ob["first_tri"] + ob["n_tri"]] = ob["material"]
    tnrm = _tri_normals_f32(live.triangles)
    Vc = np.stack([live.triangles["v0"], live.triangles["v1"], live.triangles["v2"]], 1).astype(np.float64)
    Vp = np.stack([prev.triangles["v0"], prev.triangles["v1"], prev.triangles["v2"]], 1).astype(np.float64)
    Cc, Cp = live.objects["center"].astype(np.float64), prev.objects["center"].astype(np.float64)
    first = np.full(N, -1, np.int64)
    last = np.full(N, -1, np.int64)
    n_refl, n_refr = np.zeros(N, np.int64), np.zeros(N, np.int64)
    tsum = np.zeros(N)
    hit = np.zeros(N, bool)
    v_cur, v_prev = np.zeros((N, 3)), np.zeros((N, 3))
    planes = [[] for _ in range(N)]  # per sample: (a_cur, n_cur, a_prev, n_prev) of every reflection, oldest first
    idx, co, cd = np.arange(N), o, d
    eps = f32(1e-4)

    def unit(x):
        return x / np.linalg.norm(x)

    for b in range(depth + 1):
        t, prim = tracer.intersect(co, cd)
        nxt, no, nd = [], [], []
        for k, j in enumerate(idx):
            if b == 0:
                first[j] = prim[k]
            if prim[k] < 0:
                last[j] = -1
                continue
            last[j] = prim[k]
            tsum[j] += t[k]
            ro, rd = co[k], cd[k]
            p = (ro + rd * f32(t[k])).astype(f32)
            p64 = ro.astype(np.float64) + rd.astype(np.float64) * t[k]
            if prim[k] < n_tri:
                n, mi = tnrm[prim[k]], tri_mat[prim[k]]
            else:
                ob = live.objects[prim[k] - n_tri]
                mi = ob["material"]
                n = (p - ob["center"].astype(f32)).astype(f32)
                z = _dot(n, n)
                n = (n / np.sqrt(z, dtype=f32)).astype(f32) if z > 0 else n
            M = mats[mi:mi + 1]
            emitter = bool(np.any(M[0]["emission"] > 0))
            # where the hit point is now and was in the snapshot (the first-hit rule)
            if prim[k] < n_tri:
                u, v = _bary64(Vc[prim[k]], p64)
                q_cur = Vc[prim[k], 0] + (Vc[prim[k], 1] - Vc[prim[k], 0]) * u + (Vc[prim[k], 2] - Vc[prim[k], 0]) * v
                q_prev = Vp[prim[k], 0] + (Vp[prim[k], 1] - Vp[prim[k], 0]) * u + (Vp[prim[k], 2] - Vp[prim[k], 0]) * v
            else:
                s = prim[k] - n_tri
                q_cur, q_prev = p64, p64 + (Cp[s] - Cc[s])
            if b < depth and M[0]["type"] in (0, 2) and not emitter:
                wo = (-rd).astype(f32)
                kr = L.orc_material_fresnel(ptr(M), ptr(rd), ptr(n), 1)
                down = _dot(wo, n) < 0
                if kr > 0.5:
                    p2 = (p - n * eps) if down else (p + n * eps)
                    wi = (n * f32(2 * _dot(n, wo)) - wo).astype(f32)
                    if prim[k] < n_tri:
                        nc = unit(np.cross(Vc[prim[k], 1] - Vc[prim[k], 0], Vc[prim[k], 2] - Vc[prim[k], 0]))
                        npv = unit(np.cross(Vp[prim[k], 1] - Vp[prim[k], 0], Vp[prim[k], 2] - Vp[prim[k], 0]))
                    else:
                        nc = npv = unit(p64 - Cc[prim[k] - n_tri])
                    planes[j].append((q_cur, nc, q_prev, npv))
                    n_refl[j] += 1
                else:
                    p2 = (p + n * eps) if down else (p - n * eps)
                    wi = np.zeros(3, f32)
                    L.orc_material_refract(ptr(M), ptr(rd), ptr(n), 1, ptr(wi))
                    n_refr[j] += 1
                nxt.append(j)
                no.append(p2.astype(f32))
                nd.append(wi)
            else:
                vc, vp = q_cur, q_prev
                for (ac, nc, ap, npv) in reversed(planes[j]):  # the newest reflection first
                    vc, vp = _reflect64(vc, ac, nc), _reflect64(vp, ap, npv)
                v_cur[j], v_prev[j] = vc, vp
                hit[j] = True
        if not nxt:
            break
        idx, co, cd = np.array(nxt), np.array(no, f32), np.array(nd, f32)
    xy_c, z_c = project_f64(cam, v_cur)
    xy_p, z_p = project_f64(prev_cam, v_prev)
    valid = hit & (z_c > 0) & (z_p > 0)
    rec = np.zeros((N, 4))
    rec[valid, 0:2] = (xy_p - xy_c)[valid]
    rec[valid, 2] = np.linalg.norm(v_prev - np.asarray(prev_cam["position"], np.float64).reshape(3), axis=1)[valid]
    rec[valid, 3] = 1
    rec = rec.reshape(n_px, spp, 4)
    cnt = rec[..., 3].sum(1)
    out = np.zeros((n_px, 4))
    out[:, 0:3] = rec[..., 0:3].sum(1) / np.maximum(cnt, 1)[:, None]
    out[:, 3] = cnt / spp
    sh = (Hc, Wc, spp)
    return dict(motion=out.reshape(Hc, Wc, 4), first=first.reshape(sh), last=last.reshape(sh), n_refl=n_refl.reshape(sh), n_refr=n_refr.reshape(sh),
                valid=valid.reshape(sh), depth=tsum.reshape(sh))


def prims_of(sd, objects):
    out = []
    for o in objects:
        if sd.objects["kind"][o] == 0:
            out.extend(range(int(sd.objects["first_tri"][o]), int(sd.objects["first_tri"][o] + sd.objects["n_tri"][o])))
        else:
            out.append(len(sd.triangles) + o)
    return np.array(out, np.int64)
