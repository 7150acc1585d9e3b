"""Shared by tests/test_lightmap_cpu.py, tests/test_gpu_lightmap.py and tests/lightmap_torch_child.py (include/mcpt.h: mcpt_lightmap_texels,
mcpt_lightmap_scatter, mcpt_bake_lightmap and their host forms): the numpy restatement of the lightmap rule -- coverage in float64, the
sensor in float32, the dilation in float32 -- written from the text of include/mcpt.h, and the UV layouts the tests ask about."""
import dataclasses

import numpy as np

f32, f64 = np.float32, np.float64
NO_OWNER = np.int32(2 ** 31 - 1)
NAMES = ("texel", "prim", "bary", "origins", "normals")
# the 8 neighbours in the order the dilation adds them
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the rule, restated
def model_texels(sd, ob, W, H, flip=False):
    """The texel sensors of mesh object `ob` of description `sd` -> dict of texel, prim, bary, origins, normals."""
    a, n = int(sd.objects["first_tri"][ob]), int(sd.objects["n_tri"][ob])
    T = sd.triangles[a:a + n]
    px = np.broadcast_to(((np.arange(W, dtype=f64) + 0.5) / f64(W))[None, :], (H, W))
    py = np.broadcast_to(((np.arange(H, dtype=f64) + 0.5) / f64(H))[:, None], (H, W))
    owner = np.full((H, W), NO_OWNER, np.int32)
    W1, W2 = np.zeros((H, W), f64), np.zeros((H, W), f64)
    with np.errstate(all="ignore"):
        for k in range(n - 1, -1, -1):  # descending: the lowest id is written last and owns the texel
            (ax, ay), (bx, by), (cx, cy) = T["t0"][k].astype(f64), T["t1"][k].astype(f64), T["t2"][k].astype(f64)
            area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if area2 == 0 or not np.isfinite(area2):
                continue
            w1 = ((px - ax) * (cy - ay) - (py - ay) * (cx - ax)) / area2
            w2 = ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / area2
            w0 = 1.0 - w1 - w2
            cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
            owner[cov] = a + k
            W1[cov], W2[cov] = w1[cov], w2[cov]
    texel = np.flatnonzero(owner.reshape(-1) != NO_OWNER).astype(np.int32)
    prim = owner.reshape(-1)[texel]
    u, v = W1.reshape(-1)[texel].astype(f32), W2.reshape(-1)[texel].astype(f32)
    t = sd.triangles[prim]
    v0, e1, e2 = t["v0"], (t["v1"] - t["v0"]).astype(f32), (t["v2"] - t["v0"]).astype(f32)
    origins = (v0 + (e1 * u[:, None] + e2 * v[:, None]).astype(f32)).astype(f32)
    with np.errstate(all="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(f32)
        z = (c[:, 0] * c[:, 0] + (c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])).astype(f32)
        nrm = np.where((z > 0)[:, None], c / np.sqrt(z)[:, None], c).astype(f32)
    if flip:
        nrm = -nrm
    return {"texel": texel, "prim": prim.astype(np.int32), "bary": np.stack([u, v], 1).reshape(-1, 2), "origins": origins.reshape(-1, 3),
            "normals": nrm.reshape(-1, 3)}


def model_dilate(W, H, texel, values, dilate):
    """Scatter and `dilate` rounds -> (image (H, W, 3) float32, coverage (H, W) uint8)."""
    img, cov = np.zeros((H * W, 3), f32), np.zeros(H * W, np.uint8)
    texel = np.asarray(texel, np.int64).reshape(-1)
    img[texel] = np.asarray(values, f32).reshape(-1, 3)
    cov[texel] = 1
    img, cov = img.reshape(H, W, 3), cov.reshape(H, W)
    for _ in range(dilate):
        pi, pc = np.pad(img, ((1, 1), (1, 1), (0, 0))), np.pad(cov, 1)
        s, cnt = np.zeros((H, W, 3), f32), np.zeros((H, W), np.int32)
        with np.errstate(all="ignore"):
            for dx, dy in NEIGHBOURS:
                nc = pc[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] != 0
                ni = pi[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                s = np.where(nc[..., None], (s + ni).astype(f32), s)
                cnt = cnt + nc
            take = (cov == 0) & (cnt > 0)
            mean = (s / np.maximum(cnt, 1).astype(f32)[..., None]).astype(f32)
        img = np.where(take[..., None], mean, img).astype(f32)
        cov = np.where(take, np.uint8(2), cov).astype(np.uint8)
    return img, cov


# ---------------------------------------------------------------- UV layouts
def quad(u0=0.0, v0=0.0, u1=1.0, v1=1.0, reverse=False):
    """Two triangles sharing the diagonal (u0, v0) - (u1, v1)."""
    q = [[(u0, v0), (u1, v0), (u1, v1)], [(u0, v0), (u1, v1), (u0, v1)]]
    if reverse:
        q = [[t[0], t[2], t[1]] for t in q]
    return q


def grid(m, u0=0.0, v0=0.0, u1=1.0, v1=1.0):
    """m x m quads: 2 m^2 triangles."""
    out = []
    for j in range(m):
        for i in range(m):
            out += quad(u0 + (u1 - u0) * i / m, v0 + (v1 - v0) * j / m, u0 + (u1 - u0) * (i + 1) / m, v0 + (v1 - v0) * (j + 1) / m)
    return out


def _random_triangles(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.1, 1.1, size=(n, 1, 2))
    return (c + rng.normal(0, 0.15, size=(n, 3, 2))).tolist()


NAN, INF = float("nan"), float("inf")
GOOD_A, GOOD_B = [(0.05, 0.1), (0.6, 0.15), (0.2, 0.7)], [(0.5, 0.5), (0.95, 0.55), (0.7, 0.98)]
TINY = [[(0.01 + 0.125 * i, 0.01 + 0.125 * j), (0.02 + 0.125 * i, 0.01 + 0.125 * j), (0.01 + 0.125 * i, 0.02 + 0.125 * j)] for i in range(8) for j in range(8)]
# name -> (uv triangles, width, height)
CASES = {
    "quad 8x8": (quad(), 8, 8),
    "quad 13x7": (quad(), 13, 7),
    "quad 1x1": (quad(), 1, 1),
    "quad reversed winding": (quad(reverse=True), 8, 8),
    "two overlapping charts": (quad(0.1, 0.1, 0.7, 0.7) + quad(0.4, 0.35, 0.9, 0.95, reverse=True), 24, 20),
    "chart partly outside": (quad(-0.3, 0.5, 0.6, 1.4), 16, 12),
    "degenerate among good": ([GOOD_A, [(0.1, 0.1), (0.5, 0.5), (0.9, 0.9)], [(0.3, 0.3)] * 3, [(NAN, 0.2), (0.8, 0.1), (0.5, 0.9)],
                               [(0.1, 0.2), (INF, 0.1), (0.5, 0.9)], [(0.1, 0.2), (0.4, -INF), (0.5, NAN)], GOOD_B], 16, 16),
    "sub-texel triangles": (TINY, 8, 8),
    "sub-texel among good": (TINY[:20] + [GOOD_A] + TINY[20:], 8, 8),
    "grid of 512 at 64x64": (grid(16), 64, 64),
    "one triangle over 64x64": ([[(0.02, 0.03), (0.97, 0.1), (0.4, 0.95)]], 64, 64),
    "one triangle beyond 64x64": ([[(-0.5, -0.5), (2.5, -0.5), (-0.5, 2.5)]], 64, 64),
    "grid at 33x17": (grid(4, 0.03, 0.02, 0.99, 0.97), 33, 17),
    "random triangles 29x23": (_random_triangles(40, 5), 29, 23),
    "huge coordinates": ([[(0.5, -3e6), (4e6, 2e6), (0.5, 5e6)], [(2e7, 2e7), (3e7, 2e7), (2e7, 3e7)], GOOD_A], 12, 10),
}
PLANAR = ("grid of 512 at 64x64", "grid at 33x17", "quad 13x7")  # layouts whose lifted mesh is a height field: no triangle hides another


def lift(uv, seed=1):
    """Positions (n, 3, 3) float32 for uv triangles (n, 3, 2): a smooth height field over the chart, every vertex nudged on its own so that
    no triangle is degenerate in space; coordinates that are not finite are lifted from a stand-in."""
    uv = np.nan_to_num(np.asarray(uv, f64), nan=0.3, posinf=2.0, neginf=-2.0)
    uv = np.clip(uv, -4.0, 4.0)
    u, v = uv[..., 0], uv[..., 1]
    p = np.stack([4.0 * u - 1.0 + 0.25 * v, 3.0 * v + 0.5, 0.5 * u - 0.25 * v + 0.3 * np.sin(3.0 * u) * np.cos(2.0 * v)], -1)
    return (p + np.random.default_rng(seed).normal(0, 2e-3, size=p.shape)).astype(f32)


LIGHT, MESH = 0, 1  # the objects of case_scene


def case_scene(pkg, name):
    """(SceneData, object, W, H): a light quad above (object 0, so the mesh's global primitive ids differ from its local ones) and the
    case's mesh (object 1), on a constant sky."""
    S = pkg.scenes
    uv, W, H = CASES[name]
    uv = np.asarray(uv, f32).reshape(-1, 3, 2)
    P = lift(uv)
    mesh = np.zeros(len(uv), S.TRI_DTYPE)
    mesh["v0"], mesh["v1"], mesh["v2"] = P[:, 0], P[:, 1], P[:, 2]
    mesh["t0"], mesh["t1"], mesh["t2"] = uv[:, 0], uv[:, 1], uv[:, 2]
    lamp = np.zeros(2, S.TRI_DTYPE)
    corners = np.array([[0, 1.5, 6], [3, 1.5, 6], [3, 3.5, 6], [0, 3.5, 6]], f32)
    lamp["v0"], lamp["v1"], lamp["v2"] = corners[[0, 0]], corners[[2, 3]], corners[[1, 2]]  # facing -z, towards the mesh
    b = S._Builder()
    b.add_mesh(lamp, b.material("light", S._mat(S.ROUGH_CONDUCTOR, emission=S.light_emission(1.0))))
    b.add_mesh(mesh, b.material("white", S.material_presets()["rough_white_conductor"]))
    cam = S.make_camera(32, 32, 40, (1, 2, 9), (1, 2, 0))
    sd = b.finish(camera=cam, rr_rate=0.7, spp=4, name="lightmap case: " + name, background=np.array([0.2, 0.3, 0.4], f32))
    return sd, MESH, W, H


def cornell_charted(pkg, floor_only=False):
    """cornell_demo with a planar chart over x and z for object 0 (floor.obj: floor, ceiling and back wall).  The ceiling's chart lies
    over the floor's, whose lower ids win wherever both cover; the back wall projects to a line and covers nothing."""
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    return pkg.scenes.with_planar_uvs(sd, 0, axes=(0, 2), margin=0.1, triangles=(0, 1) if floor_only else None)


def with_uvs(sd, ob, uv):
    """sd with the texture coordinates of object ob replaced by uv (n_tri, 3, 2)."""
    a, n = int(sd.objects["first_tri"][ob]), int(sd.objects["n_tri"][ob])
    tris = sd.triangles.copy()
    uv = np.asarray(uv, f32).reshape(n, 3, 2)
    for j, k in enumerate(("t0", "t1", "t2")):
        t = tris[k]
        t[a:a + n] = uv[:, j]
        tris[k] = t
    return dataclasses.replace(sd, triangles=tris)
