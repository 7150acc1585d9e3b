"""Shared by tests/test_cull_cpu.py, tests/test_gpu_cull_classify.py and tests/test_gpu_cull.py: the scenes and cameras the sky cull
(csrc/mcpt_cull.hip) is tested on, a numpy float32 restatement of its classifier k_classify, the worst-case camera rays of a pixel
(jitter-square corners x lens rim) built as camera_ray of mcpt_kernels.hip builds them, and the conservativeness checker."""
import math

import numpy as np

from chain_scene import chain_scene

f32 = np.float32
ONE_BELOW = f32(1.0 - 2.0 ** -24)  # the largest uniform rng_block can return: (2^24 - 1) / 2^24


# ------------------------------------------------------------------------------------------------ scenes
def thin_scene(pkg, dof):
    """Needles and slivers far thinner than a pixel, a small sphere, a floor: silhouettes everywhere."""
    s = pkg.scenes
    rng = np.random.default_rng(12)
    P = s.material_presets()
    b = s._Builder()
    n = 300
    tri = np.zeros(n, s.TRI_DTYPE)
    base = rng.uniform([-40, 0, -40], [40, 60, 40], (n, 3)).astype(np.float32)
    d1 = rng.normal(0, 1, (n, 3)).astype(np.float32)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    tri["v0"] = base
    tri["v1"] = base + d1 * rng.uniform(2, 30, (n, 1)).astype(np.float32)
    tri["v2"] = base + rng.normal(0, 0.02, (n, 3)).astype(np.float32)  # slivers 0.02 units wide
    b.add_mesh(tri, b.material("rough_white_conductor", P["rough_white_conductor"]))
    fl = np.zeros(2, s.TRI_DTYPE)
    fl["v0"], fl["v1"], fl["v2"] = [(-60, 0, -60)] * 2, [(-60, 0, 60), (60, 0, 60)], [(60, 0, 60), (60, 0, -60)]
    b.add_mesh(fl, b.material("gold_conductor", P["gold_conductor"]))
    light = s._mat(s.ROUGH_CONDUCTOR, emission=(30, 30, 30))
    lt = np.zeros(2, s.TRI_DTYPE)
    lt["v0"], lt["v1"], lt["v2"] = [(-10, 90, -10)] * 2, [(10, 90, -10), (10, 90, 10)], [(10, 90, 10), (-10, 90, 10)]
    b.add_mesh(lt, b.material("light", light))
    b.add_sphere((25, 40, 0), 1.5, b.material("smooth_glass", P["smooth_glass"]))
    cam = s.make_camera(160, 100, 65, (0, 30, -150), (0, 30, 0), (0, 1, 0), dof, 150.0, 4.0)
    return b.finish(camera=cam, rr_rate=0.5, spp=4, background=np.float32([0.3, 0.5, 0.8]), name="thin")


def _one_sphere(pkg):
    s = pkg.scenes
    obj = np.zeros(1, s.OBJ_DTYPE)
    obj["kind"], obj["material"], obj["center"], obj["radius"] = s.OBJ_SPHERE, 0, (0, 0, 0), 10
    mats = np.stack([s._mat(s.ROUGH_CONDUCTOR, emission=(0.5, 0.25, 0.75))]).astype(s.MAT_DTYPE)
    return s.SceneData(triangles=np.zeros(0, s.TRI_DTYPE), materials=mats, objects=obj, background=np.float32([0.1, 0.2, 0.3]), rr_rate=0.5,
                       spp=4, name="one_sphere")


def _one_triangle(pkg):
    s = pkg.scenes
    b = s._Builder()
    tri = np.zeros(1, s.TRI_DTYPE)
    tri["v0"], tri["v1"], tri["v2"] = (-10, -8, 0), (12, -6, 1), (-2, 11, -1)
    b.add_mesh(tri, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(0.5, 0.25, 0.75))))
    return b.finish(camera=None, rr_rate=0.5, spp=4, background=np.float32([0.1, 0.2, 0.3]), name="one_triangle")


_scene_cache = {}


def scene(pkg, key):
    """The scene of a case (built once; the camera of a case is given to every call, the scene's own is not used)."""
    if key not in _scene_cache:
        if key == "cornell":
            sd = pkg.scenes.cornell_demo(40, 40, 4)
        elif key == "chess":
            sd = pkg.scenes.chess_scene(width=64, height=40, spp=4)
        elif key == "thin":
            sd = thin_scene(pkg, True)
        elif key == "sphere":
            sd = _one_sphere(pkg)
        elif key == "triangle":
            sd = _one_triangle(pkg)
        elif key == "chain":
            sd = chain_scene(pkg, 36)
            sd.background = np.float32([0.1, 0.2, 0.3])
        else:
            raise KeyError(key)
        _scene_cache[key] = sd
    return _scene_cache[key]


# ------------------------------------------------------------------------------------------------ cameras
def _cutoff_aperture(pkg, W, H, fov, focal, factor):
    """The aperture radius at `factor` times the largest one the bound accepts: fmin = F - h - R > 0.05 F  <=>  R < 0.95 F - h."""
    scale = math.tan(math.radians(fov / 2))
    h = focal * math.hypot(W / H * scale / W, scale / H)
    return (0.95 * focal - h) * factor


def camera(pkg, key, root_min=None, root_max=None):
    """The camera of a case; root_min / root_max (the dumped root box) are needed by "thin_face" only."""
    mk = pkg.scenes.make_camera
    thin_eye, thin_at = (0, 30, -150), (0, 30, 0)
    if key == "cornell":
        return mk(40, 40, 40, (278, 273, -800), (278, 273, 0), (0, 1, 0), False, 900, 40)
    if key == "cornell_inside":  # the eye inside the closed box
        return mk(40, 40, 70, (278, 273, 100), (278, 200, 559), (0, 1, 0), False, 900, 40)
    if key == "chess":  # the scene's own camera: depth of field, focused on the king
        return mk(64, 40, 70, (278, 150, -2550), (278, 0, 0), (0, 1, 0), True, 3036.98, 10)
    if key == "chess_up":  # the same eye, looking over the pieces: more sky
        return mk(64, 40, 70, (278, 150, -2550), (278, 900, 0), (0, 1, 0), False, 3036.98, 10)
    if key == "chess_nodof":
        return mk(64, 40, 70, (278, 150, -2550), (278, 0, 0), (0, 1, 0), False, 3036.98, 10)
    if key == "thin_dof":
        return mk(64, 40, 65, thin_eye, thin_at, (0, 1, 0), True, 150.0, 4.0)
    if key == "thin":
        return mk(64, 40, 65, thin_eye, thin_at, (0, 1, 0), False, 150.0, 4.0)
    if key == "thin_inside":  # from inside the cloud of needles, looking out
        return mk(64, 40, 65, (3, 30, 2), (60, 120, 40), (0, 1, 0), True, 60.0, 0.05)
    if key == "thin_focus_short":  # focal distance 0.02 x the distance to the geometry: s_far >> 1
        return mk(64, 40, 65, thin_eye, thin_at, (0, 1, 0), True, 3.0, 0.05)
    if key == "thin_focus_long":  # 50 x: everything is closer than the focal plane, the |1 - s| R term
        return mk(64, 40, 65, thin_eye, thin_at, (0, 1, 0), True, 7500.0, 4.0)
    if key == "thin_aperture_under":  # just inside the fmin > 0.05 focal cut-off
        return mk(64, 40, 65, thin_eye, thin_at, (0, 1, 0), True, 10.0, _cutoff_aperture(pkg, 64, 40, 65, 10.0, 0.999))
    if key == "thin_aperture_over":  # just outside: the bound refuses the camera
        return mk(64, 40, 65, thin_eye, thin_at, (0, 1, 0), True, 10.0, _cutoff_aperture(pkg, 64, 40, 65, 10.0, 1.001))
    if key == "thin_fov1":
        return mk(64, 40, 1, thin_eye, (10, 35, 0), (0, 1, 0), True, 150.0, 0.05)
    if key == "thin_fov150":
        return mk(64, 40, 150, thin_eye, thin_at, (0, 1, 0), True, 150.0, 4.0)
    if key == "thin_1x1":
        return mk(1, 1, 65, thin_eye, thin_at, (0, 1, 0), True, 150.0, 4.0)
    if key == "thin_1x40":
        return mk(1, 40, 65, thin_eye, thin_at, (0, 1, 0), True, 150.0, 4.0)
    if key == "thin_64x1":
        return mk(64, 1, 65, thin_eye, thin_at, (0, 1, 0), True, 150.0, 4.0)
    if key == "thin_37x19":  # odd sizes, the view along +z: x0 == 0 in the centre column and y0 == 0 in the centre row, exactly
        return mk(37, 19, 65, thin_eye, thin_at, (0, 1, 0), False, 150.0, 4.0)
    if key == "thin_face":  # the eye exactly on the -z face of the root box
        return mk(37, 19, 65, (0, 30, float(root_min[2])), (80, 110, float(root_min[2]) + 30), (0, 1, 0), True, 60.0, 0.05)
    if key == "thin_away":  # the scene off to the side
        return mk(37, 19, 65, thin_eye, (400, 30, -150), (0, 1, 0), True, 150.0, 4.0)
    if key == "thin_behind":  # all geometry behind the eye
        return mk(37, 19, 65, thin_eye, (0, 30, -400), (0, 1, 0), True, 150.0, 4.0)
    if key == "sphere":
        return mk(37, 19, 50, (3, 4, -60), (0, 0, 0), (0, 1, 0), True, 60.0, 1.0)
    if key == "triangle":
        return mk(37, 19, 50, (3, 4, -60), (0, 0, 0), (0, 1, 0), True, 60.0, 1.0)
    if key == "chain":  # along +z through the square every box of the chain shares
        return mk(37, 19, 60, (-0.5, -0.25, -40), (-0.5, -0.25, 0), (0, 1, 0), False, 40.0, 1.0)
    raise KeyError(key)


# ------------------------------------------------------------------------------------------------ the table
class Case:
    def __init__(self, scene, cam, tree=("sah", None), instancing=False, need=(), share=False):
        self.scene, self.cam, self.tree, self.instancing, self.need, self.share = scene, cam, tree, instancing, tuple(need), share
        self.id = "%s-%s%s%s" % (cam, tree[0], "" if tree[1] is None else "-q" + tree[1], "-inst" if instancing else "")

    @property
    def host_tree(self):
        return self.tree[0] in ("sah", "reference")


# (MCPT_BVH, MCPT_QUANT_NODES): sah, sah with float nodes, the reference's topology, and the two device builders
TREES5 = [("sah", None), ("sah", "0"), ("reference", "0"), ("lbvh", None), ("ploc", None)]
# need: the pixel classes that must occur ("sky": no ray can hit; "short": a candidate list; "walk": the rays walk the tree);
# share: sky + short pixels must be at least 10 % of the frame
CASES = (
    [Case("cornell", "cornell", need=("short", "walk")),
     Case("cornell", "cornell_inside", need=("short",))]
    + [Case("chess", "chess", tree=t, need=("sky", "short", "walk"), share=True) for t in TREES5]
    + [Case("chess", "chess_nodof", need=("sky", "short", "walk"), share=True),
       Case("chess", "chess_up", instancing=True, need=("sky", "short", "walk"), share=True)]
    + [Case("thin", "thin_dof", tree=t, need=("sky", "short", "walk"), share=True) for t in TREES5]
    + [Case("thin", "thin", need=("sky", "short", "walk"), share=True),
       Case("thin", "thin_inside", need=("short", "walk")),
       Case("thin", "thin_focus_short", need=("walk",)),
       Case("thin", "thin_focus_long", need=("sky", "short", "walk"), share=True),
       Case("thin", "thin_aperture_under", need=("walk",)),
       Case("thin", "thin_aperture_over", need=("walk",)),
       Case("thin", "thin_fov1", need=("short",)),
       Case("thin", "thin_fov150", need=("sky", "walk"), share=True),
       Case("thin", "thin_1x1", need=("walk",)),
       Case("thin", "thin_1x40", need=("sky", "walk"), share=True),
       Case("thin", "thin_64x1", need=("walk",)),
       Case("thin", "thin_37x19", need=("sky", "short", "walk"), share=True),
       Case("thin", "thin_face", need=("sky", "short", "walk"), share=True),
       Case("thin", "thin_away", need=("sky",), share=True),
       Case("thin", "thin_behind", need=("sky",), share=True),
       Case("sphere", "sphere", need=("sky", "short")),
       Case("triangle", "triangle", need=("sky", "short")),
       Case("chain", "chain", tree=("lbvh", None), need=("walk",))]
)


def set_tree(monkeypatch, case):
    """The environment that selects the case's tree for scenes created (or dumped) afterwards."""
    monkeypatch.setenv("MCPT_BVH", case.tree[0])
    if case.tree[1] is None:
        monkeypatch.delenv("MCPT_QUANT_NODES", raising=False)
    else:
        monkeypatch.setenv("MCPT_QUANT_NODES", case.tree[1])
    monkeypatch.setenv("MCPT_INSTANCING", "1" if case.instancing else "0")


# ------------------------------------------------------------------------------------------------ k_classify, restated
def _beam_box(o, d, mn, mx, rho):
    """beam_box of mcpt_cull.hip for rows: o [3], d [n, 3], mn / mx [n, 3], all float32; axis by axis, the same operations."""
    n = len(d)
    smin, smax = np.zeros(n, f32), np.full(n, np.inf, f32)
    ok = np.ones(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            lo, hi = mn[:, a] - rho, mx[:, a] + rho
            da = d[:, a]
            moving = np.abs(da) > f32(1e-30)
            s1, s2 = (lo - o[a]) / da, (hi - o[a]) / da
            smin = np.where(moving, np.fmax(smin, np.fmin(s1, s2)), smin)
            smax = np.where(moving, np.fmin(smax, np.fmax(s1, s2)), smax)
            ok &= moving | ~((o[a] < lo) | (o[a] > hi))
        return ok & (smax * f32(1.0001) + f32(1e-6) >= smin)


def central_rays(cam, info):
    """The central ray of every pixel as k_classify forms it: (eye [3], d [W*H, 3]) in float32."""
    W, H = int(cam["width"]), int(cam["height"])
    m = np.arange(W * H)
    i, j = (m % W).astype(np.int32), (m // W).astype(np.int32)
    scale, aspect, focal = f32(info["scale"]), f32(info["aspect"]), f32(info["focal"])
    x0 = (f32(1) - f32(2) * (i.astype(f32) + f32(0.5)) / f32(W)) * aspect * scale
    y0 = (f32(1) - f32(2) * (j.astype(f32) + f32(0.5)) / f32(H)) * scale
    fp = [x0 * focal, y0 * focal, np.full(W * H, focal, f32)]
    O = np.asarray(cam["orientation"], f32).reshape(9)
    d = np.stack([(O[3 * a] * fp[0] + O[3 * a + 1] * fp[1]) + O[3 * a + 2] * fp[2] for a in range(3)], axis=1).astype(f32)
    return np.asarray(cam["position"], f32).reshape(3), d


def classify(bvh, cam, info):
    """k_classify for every pixel of `cam` over the tree `bvh` = (info dict, boxes, children, ...) of mcpt_bvh_dump / mcpt_scene_dump_bvh,
    with the bound `info` (mcpt_cull_info as a dict) -> (may_hit uint8 [W*H], cand int32 [W*H, 4]) in the encoding of mcpt_debug_classify.
    The same float32 operations in the same order: left child first, the right one on the stack when both are entered."""
    binfo, boxes, children = bvh[0], bvh[1], bvh[2]
    W, H = int(cam["width"]), int(cam["height"])
    n = W * H
    may_hit, cand = np.ones(n, np.uint8), np.full((n, 4), -1, np.int32)
    if not info["classified"]:
        cand[:, 0] = -2
        return may_hit, cand
    rho = f32(info["rho"])
    o, d = central_rays(cam, info)
    root_min, root_max = np.asarray(binfo["root_min"], f32), np.asarray(binfo["root_max"], f32)
    no_inst = binfo["n_instances"] == 0
    n_leaf_prims = binfo["n_leaf_prims"]
    enter = _beam_box(o, d, np.broadcast_to(root_min, (n, 3)), np.broadcast_to(root_max, (n, 3)), rho)
    hit = np.zeros(n, bool)
    n_cand = np.zeros(n, np.int32)
    cur = np.full(n, binfo["root"], np.int64)
    sp = np.zeros(n, np.int32)
    stk = np.zeros((n, 64), np.int64)
    live = np.flatnonzero(enter)
    while len(live):
        c = cur[live]
        leaf = c < 0
        # ---- leaves
        L = live[leaf]
        if len(L):
            cl = cur[L]
            hit[L] = True
            prim_leaf = ((~cl) < n_leaf_prims) | no_inst
            over = ~prim_leaf | (n_cand[L] == 4)
            n_cand[L[over]] = 5
            K = L[~over]
            cand[K, n_cand[K]] = (~cur[K]).astype(np.int32)
            n_cand[K] += 1
            done = over.copy()
            empty = sp[K] == 0
            done[~over] = empty
            P = K[~empty]
            sp[P] -= 1
            cur[P] = stk[P, sp[P]]
            cur[L[done]] = -1
            finished = np.zeros(len(live), bool)
            finished[np.flatnonzero(leaf)[done]] = True
        else:
            finished = np.zeros(len(live), bool)
        # ---- inner nodes
        N = live[~leaf]
        if len(N):
            cn = cur[N]
            b = boxes[cn]
            hl = _beam_box(o, d[N], b[:, 0:3], b[:, 3:6], rho)
            hr = _beam_box(o, d[N], b[:, 6:9], b[:, 9:12], rho)
            left, right = children[cn, 0].astype(np.int64), children[cn, 1].astype(np.int64)
            both = hl & hr
            B = N[both]
            stk[B, sp[B]] = right[both]
            sp[B] += 1
            nxt = np.where(hl, left, right)
            none = ~hl & ~hr
            Z = N[none]
            empty = sp[Z] == 0
            P = Z[~empty]
            sp[P] -= 1
            nxt_none = np.full(len(Z), -1, np.int64)
            nxt_none[~empty] = stk[P, sp[P]]
            nxt[none] = nxt_none
            cur[N] = nxt
            fin_n = np.zeros(len(N), bool)
            fin_n[np.flatnonzero(none)[empty]] = True
            finished[np.flatnonzero(~leaf)[fin_n]] = True
        live = live[~finished]
    may_hit[:] = hit
    walk = n_cand > 4
    cand[walk] = (-2, -1, -1, -1)
    return may_hit, cand


def classes(may_hit, cand):
    """Pixel counts (sky, short list, walk the tree)."""
    walk = cand[:, 0] == -2
    sky = may_hit == 0
    return int(sky.sum()), int((~sky & ~walk).sum()), int(walk.sum())


def check_non_vacuous(case, may_hit, cand):
    sky, short, walk = classes(may_hit, cand)
    n = len(may_hit)
    print("\n[cull classes] %-28s sky %5.1f %%  short list %5.1f %%  walk %5.1f %%  (%d pixels)" % (case.id, 100 * sky / n, 100 * short / n, 100 * walk / n, n))
    have = {"sky": sky, "short": short, "walk": walk}
    for k in case.need:
        assert have[k] > 0, (case.id, k, have)
    if case.share:
        assert 10 * (sky + short) >= n, (case.id, have)


# ------------------------------------------------------------------------------------------------ camera rays
RIM = [(f32(math.cos(k * math.pi / 4)), f32(math.sin(k * math.pi / 4))) for k in range(8)]


def _mat3_mul(O, v):
    return [O[3 * r] * v[0] + (O[3 * r + 1] * v[1] + O[3 * r + 2] * v[2]) for r in range(3)]


def camera_rays_f32(cam, pix, u0, u1, r, ct, st):
    """camera_ray of mcpt_kernels.hip in float32 numpy, operation for operation, from the uniforms u0, u1 (pixel jitter) and the lens
    sample given as r = aperture_radius * sqrtf(u2) and (ct, st) = (cos, sin)(2 pi u3).  All arguments are rows; -> (origins, dirs)."""
    W, H = int(cam["width"]), int(cam["height"])
    half = f32(cam["fov"]) * f32(0.5)
    scale = f32(math.tan(float(f32(float(half * f32(3.141592653589793)) / 180.0))))  # make_camera, csrc/mcpt_wavefront.hip
    aspect = f32(W) / f32(H)
    i, j = (pix % W).astype(f32), (pix // W).astype(f32)
    x = (f32(1) - f32(2) * (i + u0) / f32(W)) * aspect * scale
    y = (f32(1) - f32(2) * (j + u1) / f32(H)) * scale
    O = np.asarray(cam["orientation"], f32).reshape(9)
    eye = np.asarray(cam["position"], f32).reshape(3)
    one, zero = np.ones_like(x), np.zeros_like(x)
    if int(cam["use_dof"]):
        F = f32(cam["focal_distance"])
        dx, dy = r * ct, r * st
        lens = _mat3_mul(O, [dx, dy, zero])
        pos = np.stack([eye[a] + lens[a] for a in range(3)], axis=1)
        v = [x * F - dx, y * F - dy, one * F - zero]
    else:
        pos = np.broadcast_to(eye, (len(x), 3)).copy()
        v = [x, y, one]
    z = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])
    s = np.sqrt(z)
    v = [c / s for c in v]
    return pos.astype(f32), np.stack(_mat3_mul(O, v), axis=1).astype(f32)


def extremal_rays(cam):
    """Per pixel the rays the random sampler never draws: the four corners of the jitter square, each through the lens centre and (with
    depth of field) through eight points of the lens rim at the largest radius -> (pixel [n], origins [n, 3], dirs [n, 3])."""
    n_pix = int(cam["width"]) * int(cam["height"])
    R = f32(cam["aperture_radius"]) * np.sqrt(ONE_BELOW)
    lens = [(f32(0), f32(1), f32(0))] + ([(R, c, s) for c, s in RIM] if int(cam["use_dof"]) else [])
    rows = [(u0, u1, r, c, s) for u0 in (f32(0), ONE_BELOW) for u1 in (f32(0), ONE_BELOW) for (r, c, s) in lens]
    pix = np.repeat(np.arange(n_pix), len(rows))
    col = [np.tile(np.asarray([row[k] for row in rows], f32), n_pix) for k in range(5)]
    o, d = camera_rays_f32(cam, pix, *col)
    return pix, o, d


N_REAL = 16
_rays = {}


def oracle_rays(pkg, oracle, case, cam):
    """Per (scene, camera), once: the extremal rays and N_REAL real sample rays of every pixel with the oracle's closest hits ->
    (pixel [n], prim [n])."""
    key = (case.scene, case.cam)
    if key not in _rays:
        os_ = oracle.OracleScene(scene(pkg, case.scene))
        pix, o, d = extremal_rays(cam)
        n_pix = int(cam["width"]) * int(cam["height"])
        rp = np.repeat(np.arange(n_pix), N_REAL)
        ro, rd = os_.camera_rays(rp, np.tile(np.arange(N_REAL), n_pix), seed=7, camera=cam)
        _, prim = os_.intersect(np.concatenate([o, ro]), np.concatenate([d, rd]))
        _rays[key] = (np.concatenate([pix, rp]), prim)
    return _rays[key]


def violations(may_hit, cand, pix, prim):
    """The rays that contradict a classification: a hit in a pixel classified as sky, or a hit primitive missing from the pixel's short
    list.  pix, prim: per ray its pixel and the primitive it hits (-1: none) -> a bool row per ray."""
    hit = prim >= 0
    short = cand[pix, 0] != -2
    listed = (cand[pix] == prim[:, None]).any(axis=1)
    return hit & ((may_hit[pix] == 0) | (short & ~listed))
