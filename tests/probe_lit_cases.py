"""Shared by tests/test_gpu_probe_lit.py and tests/probe_lit_torch_child.py (include/mcpt.h: mcpt_render_probe_lit): the numpy float32
restatement of a probe-lit frame, built only from pieces that exist without the feature -- centre_rays / camera_rays, intersect,
p = o + d * (float)t in numpy float32, the AOV record or the material table with query_closest's normal, the host forms of the two grid
lookups, cast_rays for the samples that end on the sky or on an emitter -- and the float64 walk of the specular chains.  Every float32
operation is rounded in the written order (no FMA), dot(a, b) = a.x b.x + (a.y b.y + a.z b.z).  No tests in here."""
import ctypes as C

import numpy as np

import probe_depth_cases as pdc
from material_edit_cases import emits
from mirror_scene import _tri_normals_f32
from ray_query_cases import Rays, closest
from sensor_query_cases import cast_values

f32, f64 = np.float32, np.float64
MISS, EMITTER, SURFACE = 0, 1, 2
ZERO = f32(0)


def dot3(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


class Volume:
    """A baked probe volume: the grid, the device buffers the calls take and their host copies."""

    def __init__(self, hs, grid, spp=64, depth_spp=64, max_distance=None, seed=2, depth_seed=3, normal_bias=0.0, backface_max=0.25):
        self.grid, self.nb, self.bm = grid, normal_bias, backface_max
        m = grid[2][0] * grid[2][1] * grid[2][2]
        self.dev = {"sh": pdc.Guarded((m, 27)), **pdc.depth_outputs(m)}
        hs.bake_probe_volume(*grid, depth_spp, max_distance, depth_seed=depth_seed, out=self.dev, spp=spp, seed=seed)
        self.sh, self.mom, self.cnt = self.dev["sh"].get(), self.dev["moments"].get(), self.dev["counts"].get()

    def kw(self, visible):
        """The volume arguments of HipScene.render_probe_lit after (origin, spacing, dims)."""
        if visible:
            return dict(sh=self.dev["sh"], moments=self.dev["moments"], counts=self.dev["counts"], normal_bias=self.nb, backface_max=self.bm)
        return dict(sh=self.dev["sh"])

    def lookup(self, hip, p, n, visible):
        """The host form of the lookup the frame makes: E / pi (n, 3) float32."""
        if len(p) == 0:
            return np.zeros((0, 3), f32)
        if visible:
            return hip.probe_shade_visible(*self.grid, self.sh, self.mom, self.cnt, p, n, normal_bias=self.nb, backface_max=self.bm)
        return hip.probe_shade(*self.grid, self.sh, p, n)


def scene_grid(sd, dims=(3, 2, 3)):
    """(origin, spacing, dims) of a grid over the inner 80 % of the bounding box of the scene's triangles."""
    v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]]).astype(f64)
    lo, hi = v.min(0), v.max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.8
    o = mid - half
    s = [2 * half[a] / max(dims[a] - 1, 1) for a in range(3)]
    return tuple(float(f32(x)) for x in o), tuple(float(f32(x)) for x in s), tuple(dims)


def prim_materials(sd):
    """The material index of every primitive id: triangles, then n_tri + object index for the spheres."""
    n_tri = len(sd.triangles)
    mat = np.zeros(n_tri + len(sd.objects), np.int64)
    for k, ob in enumerate(sd.objects):
        if ob["kind"] == 0:
            mat[ob["first_tri"]:ob["first_tri"] + ob["n_tri"]] = ob["material"]
        mat[n_tri + k] = ob["material"]
    return mat


def frame_rays(hs, cam, centre, spp, seed):
    """(o, d) of shape (n_px * spp, 3), pixel-major in sample order."""
    n_px = int(cam["width"]) * int(cam["height"])
    if centre:
        return hs.centre_rays(np.arange(n_px, dtype=np.uint32), camera=cam)
    pix, smp = np.repeat(np.arange(n_px, dtype=np.uint32), spp), np.tile(np.arange(spp, dtype=np.uint32), n_px)
    return hs.camera_rays(pix, smp, seed=seed, camera=cam)


def fold(v, p, kind, n_px, spp):
    """(lit (n_px, 3), position (n_px, 3)): acc = 0; acc += v_k / (float)spp in sample order; the sum of p over the samples that ended on
    a hit divided by their number, 0 without one."""
    v, p, hit = v.reshape(n_px, spp, 3), p.reshape(n_px, spp, 3), (kind != MISS).reshape(n_px, spp)
    lit, ps, cnt = np.zeros((n_px, 3), f32), np.zeros((n_px, 3), f32), np.zeros(n_px, np.int64)
    fn = f32(spp)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):
            lit = lit + v[:, k] / fn
            ps = np.where(hit[:, k, None], ps + p[:, k], ps).astype(f32)
            cnt += hit[:, k]
        pos = np.where(cnt[:, None] > 0, ps / np.maximum(cnt, 1).astype(f32)[:, None], ZERO).astype(f32)
    return lit.astype(f32), pos


def restate_depth0(hs, hip, sd, vol, visible, cam, centre=True, spp=1, seed=1, aov=None):
    """The frame at specular_depth 0 -> dict(lit (H, W, 3), position (H, W, 3), lookups, kind (H, W, spp)).
    centre with aov (render_aovs(centre=True) of the same camera): the albedo and the flipped normal are the AOV record's.  Otherwise the
    albedo is the material table's (untextured scenes) and the normal query_closest's, flipped with dot(n, d) > 0."""
    Wc, Hc = int(cam["width"]), int(cam["height"])
    n_px = Wc * Hc
    o, d = frame_rays(hs, cam, centre, spp, seed)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(hit[:, None], o + d * t.astype(f32)[:, None], ZERO).astype(f32)
    pm = prim_materials(sd)
    mi = pm[np.where(hit, prim, 0)]
    emitter = hit & emits(sd.materials)[mi]
    kind = np.where(hit, np.where(emitter, EMITTER, SURFACE), MISS)
    if aov is not None:
        a = aov.reshape(n_px, 8)
        alb, nf = a[:, 0:3].astype(f32), a[:, 3:6].astype(f32)
        assert np.array_equal(a[:, 7] > 0, hit), "the AOV record and intersect disagree on the pixels that are hit"
    else:
        M = sd.materials[mi]
        assert not M["textured"][kind == SURFACE].any(), "the material-table albedo holds for untextured materials only"
        conductor = (M["type"] == 0) | (M["type"] == 1)
        alb = np.where(conductor[:, None], M["base_reflectance"], f32(1)).astype(f32)
        ng = closest(hs, Rays(o, d), want=("normal",))[0]["normal"]
        nf = np.where((dot3(ng, d) > 0)[:, None], -ng, ng).astype(f32)
    v = np.zeros((len(o), 3), f32)
    s = kind == SURFACE
    E = vol.lookup(hip, p[s], nf[s], visible)
    v[s] = alb[s] * np.fmax(E, ZERO)
    other = np.flatnonzero(~s)
    if len(other):  # the sky and the emitters: deterministic in cast_rays, whatever the sample
        v[other] = cast_values(hs, o[other], d[other], 1, seed=1)[:, 0, :]
    lit, pos = fold(v, p, kind, n_px, spp)
    return dict(lit=lit.reshape(Hc, Wc, 3), position=pos.reshape(Hc, Wc, 3), lookups=int(s.sum()), kind=kind.reshape(Hc, Wc, spp))


def chain_walk(oracle, hs, sd, cam, depth):
    """The chains of the centre rays of `cam`, every bounce decided as the kernels decide it (float32, the oracle's material functions:
    the walk of tests/mirror_scene.py), the terminal points in float64 -> dict per pixel: kind, prim, p64 (terminal point o + d t in
    float64 of the last segment's float32 ray), d (the last segment's direction), n (the stored normal at an emitter terminal)."""
    L = oracle.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n_px = int(cam["width"]) * int(cam["height"])
    o, d = hs.centre_rays(np.arange(n_px, dtype=np.uint32), camera=cam)
    n_tri = len(sd.triangles)
    mats = np.ascontiguousarray(sd.materials)
    pm = prim_materials(sd)
    em = emits(mats)
    tnrm = _tri_normals_f32(sd.triangles)
    kind, last = np.zeros(n_px, np.int64), np.full(n_px, -1, np.int64)
    p64, dl, nl = np.zeros((n_px, 3)), np.zeros((n_px, 3)), np.zeros((n_px, 3))
    bounces = np.zeros(n_px, np.int64)
    idx, co, cd = np.arange(n_px), np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
    eps = f32(1e-4)

    def dot(a, b):
        return f32(a[0] * b[0] + f32(a[1] * b[1] + a[2] * b[2]))

    for b in range(depth + 1):
        t, prim = hs.intersect(co, cd)
        nxt, no, nd = [], [], []
        for k, j in enumerate(idx):
            dl[j] = cd[k]
            if prim[k] < 0:
                kind[j] = MISS
                continue
            last[j] = prim[k]
            ro, rd = co[k], cd[k]
            p = (ro + rd * f32(t[k])).astype(f32)
            p64[j] = ro.astype(f64) + rd.astype(f64) * t[k]
            if prim[k] < n_tri:
                n = tnrm[prim[k]]
            else:
                n = (p - sd.objects[prim[k] - n_tri]["center"].astype(f32)).astype(f32)
                n = (n / np.sqrt(dot(n, n), dtype=f32)).astype(f32)
            mi = pm[prim[k]]
            M = mats[mi:mi + 1]
            nl[j] = n
            if b < depth and M[0]["type"] in (0, 2) and not em[mi]:
                wo = (-rd).astype(f32)
                kr = L.orc_material_fresnel(ptr(M), ptr(rd), ptr(n), 1)
                down = dot(wo, n) < 0
                if kr > 0.5:
                    p2 = (p - n * eps) if down else (p + n * eps)
                    wi = (n * f32(2 * dot(n, wo)) - wo).astype(f32)
                else:
                    p2 = (p + n * eps) if down else (p - n * eps)
                    wi = np.zeros(3, f32)
                    L.orc_material_refract(ptr(M), ptr(rd), ptr(n), 1, ptr(wi))
                bounces[j] += 1
                nxt.append(j)
                no.append(p2.astype(f32))
                nd.append(wi)
            else:
                kind[j] = EMITTER if em[mi] else SURFACE
        if not nxt:
            break
        idx, co, cd = np.array(nxt), np.array(no, f32), np.array(nd, f32)
    return dict(kind=kind, prim=last, p64=p64, d=dl, n=nl, bounces=bounces)


def lit_frame(hs, vol, visible, position=True, **kw):
    """render_probe_lit into guarded buffers of the camera's size -> (lit, position or None, info) as numpy."""
    cam = kw.get("camera")
    cam = hs.sd.camera if cam is None else cam
    Wc, Hc = int(np.asarray(cam["width"]).reshape(-1)[0]), int(np.asarray(cam["height"]).reshape(-1)[0])
    out = {"lit": pdc.Guarded((Hc, Wc, 3))}
    if position:
        out["position"] = pdc.Guarded((Hc, Wc, 3))
    vk = vol.kw(visible)
    _, _, info = hs.render_probe_lit(*vol.grid, vk.pop("sh"), position=position, out=out, **vk, **kw)
    return out["lit"].get(), (out["position"].get() if position else None), info
