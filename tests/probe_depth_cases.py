"""Shared by tests/test_probe_depth_cpu.py, tests/test_probe_depth_abi.py, tests/test_gpu_probe_depth.py and
tests/probe_depth_torch_child.py (include/mcpt.h: mcpt_query_probe_depth, mcpt_probe_shade_visible and their host forms): numpy float32
restatements of the text of include/mcpt.h -- texel directions, the texel of a vector, the cos^32 fold and the occlusion-aware lookup --
every operation rounded to float32 in the written order (no FMA), dot(a, b) = a.x b.x + (a.y b.y + a.z b.z)."""
import numpy as np

import probe_cases as pc
from ray_query_cases import GUARD, DevBuf, Rays, closest
from sensor_query_cases import SENTINEL, same_bits  # noqa: F401  (re-exported to the tests)

f32, f64 = np.float32, np.float64
RES, TEXELS, ROW = 8, 64, 192
ONE, HALF, ZERO = f32(1), f32(0.5), f32(0)
COUNT_SENTINEL = -77


def dot3(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def sgn(v):
    return np.where(v >= 0, ONE, -ONE).astype(f32)


def texel_dirs():
    """c_j (64, 3): j = 8 ty + tx."""
    j = np.arange(TEXELS)
    tx, ty = (j & 7).astype(f32), (j >> 3).astype(f32)
    ox = (tx + HALF) * f32(0.25) - ONE
    oy = (ty + HALF) * f32(0.25) - ONE
    az = (ONE - np.abs(ox)) - np.abs(oy)
    x = np.where(az < 0, (ONE - np.abs(oy)) * sgn(ox), ox).astype(f32)
    y = np.where(az < 0, (ONE - np.abs(ox)) * sgn(oy), oy).astype(f32)
    ln = np.sqrt((x * x + y * y) + az * az)
    return np.stack([x / ln, y / ln, az / ln], axis=1).astype(f32)


def texel_of(v):
    v = np.asarray(v, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (np.abs(v[:, 0]) + np.abs(v[:, 1])) + np.abs(v[:, 2])
        ok = (s > 0) & np.isfinite(s)
        sd = np.where(ok, s, ONE).astype(f32)
        px, py = v[:, 0] / sd, v[:, 1] / sd
        fold = v[:, 2] < 0
        fx, fy = (ONE - np.abs(py)) * sgn(px), (ONE - np.abs(px)) * sgn(py)
        px, py = np.where(fold, fx, px).astype(f32), np.where(fold, fy, py).astype(f32)
        tx = np.clip(np.floor((px + ONE) * f32(4)), 0, 7)
        ty = np.clip(np.floor((py + ONE) * f32(4)), 0, 7)
        tx, ty = np.where(np.isnan(tx), 0, tx).astype(np.int32), np.where(np.isnan(ty), 0, ty).astype(np.int32)
    return np.where(ok, 8 * ty + tx, 0).astype(np.int32)


def fold(d, r, bf, moments=None, counts=None):
    """moments (n, 192), counts (n, 2): acc = given or 0; for k in sample order W += w, S1 += w * r, S2 += w * (r * r) with w = cos^32."""
    d, r = np.asarray(d, f32), np.asarray(r, f32)
    n, spp, _ = d.shape
    c = texel_dirs()
    acc = np.zeros((n, TEXELS, 3), f32) if moments is None else np.array(moments, f32).reshape(n, TEXELS, 3)
    W, S1, S2 = acc[:, :, 0].copy(), acc[:, :, 1].copy(), acc[:, :, 2].copy()
    for k in range(spp):
        w = np.maximum(dot3(c[None, :, :], d[:, k, None, :]), ZERO).astype(f32)
        for _ in range(5):
            w = w * w
        rk = r[:, k, None]
        W = W + w
        S1 = S1 + w * rk
        S2 = S2 + w * (rk * rk)
    cn = np.zeros((n, 2), np.int32) if counts is None else np.array(counts, np.int32).reshape(n, 2)
    cn[:, 0] += spp
    cn[:, 1] += (np.asarray(bf) != 0).sum(axis=1).astype(np.int32)
    return np.stack([W, S1, S2], axis=2).astype(f32).reshape(n, ROW), cn


def shade_visible(origin, spacing, dims, sh, moments, counts, points, normals, normal_bias, backface_max, kill=()):
    """The occlusion-aware lookup of include/mcpt.h -> (out (n, 3), A (n,)).  kill: probes whose weight is forced to 0."""
    sh = np.asarray(sh, f32).reshape(-1, 27)
    mom = np.asarray(moments, f32).reshape(-1, TEXELS, 3)
    counts = np.asarray(counts, np.int32).reshape(-1, 2)
    p, n = np.asarray(points, f32).reshape(-1, 3), np.asarray(normals, f32).reshape(-1, 3)
    nx, ny, nz = (int(v) for v in dims)
    ax = [pc.grid_axis(p[:, a], origin[a], spacing[a], int(dims[a])) for a in range(3)]
    step = [1 if int(dims[a]) > 1 else 0 for a in range(3)]
    o32, s32 = np.asarray(origin, f32), np.asarray(spacing, f32)
    nb, bm = f32(normal_bias), f32(backface_max)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = p + nb * n
        A = np.zeros(len(p), f32)
        b = np.zeros((len(p), 27), f32)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            wx = ax[0][1] if dx else ONE - ax[0][1]
            wy = ax[1][1] if dy else ONE - ax[1][1]
            wz = ax[2][1] if dz else ONE - ax[2][1]
            wt = (wz * wy) * wx
            ci = [ax[0][0] + dx * step[0], ax[1][0] + dy * step[1], ax[2][0] + dz * step[2]]
            probe = (ci[2] * ny + ci[1]) * nx + ci[0]
            P = np.stack([o32[a] + ci[a].astype(f32) * s32[a] for a in range(3)], axis=1).astype(f32)
            cnt, back = counts[probe, 0], counts[probe, 1]
            dead = (cnt > 0) & (back.astype(f32) > bm * cnt.astype(f32))
            for k in kill:
                dead = dead | (probe == k)
            u = P - p
            lu = np.sqrt(dot3(u, u))
            cosn = np.where(lu > 0, dot3(u, n) / np.where(lu > 0, lu, ONE), ONE).astype(f32)
            h = (cosn + ONE) * HALF
            wb = h * h + f32(0.2)
            v = q - P
            dist = np.sqrt(dot3(v, v))
            m3 = mom[probe, texel_of(v)]
            W, S1, S2 = m3[:, 0], m3[:, 1], m3[:, 2]
            Wd = np.where(W > 0, W, ONE).astype(f32)
            m, m2 = S1 / Wd, S2 / Wd
            var = np.abs(m2 - m * m)
            dd = dist - m
            den = var + dd * dd
            chv = np.where(den > 0, var / np.where(den > 0, den, ONE), ZERO).astype(f32)
            chv = (chv * chv) * chv
            ch = np.where((W > 0) & (dist > m), chv, ONE).astype(f32)
            a = np.where(dead, ZERO, (wt * wb) * ch).astype(f32)
            A = A + a
            b = b + a[:, None] * sh[probe]
        e = pc.irradiance(b, n) / A[:, None]
    plain = pc.shade(origin, spacing, dims, sh, p, n)
    return np.where((A > 0)[:, None], e, plain).astype(f32), A


# ---------------------------------------------------------------- GPU helpers
def samples(hs, p, spp, seed, max_distance, sample_offset=0):
    """(d, r, backfacing) of a call from calls that exist without the feature: probe_rays directions, intersect distances and the normals
    query_closest reports; r = hit ? min((float)t, max_distance) : max_distance, back-facing iff hit and dot(ng, d) > 0."""
    n = len(p)
    o, d = pc.probe_pairs(hs, p, spp, seed, sample_offset)
    o2, d2 = o.reshape(-1, 3), d.reshape(-1, 3)
    t, prim = hs.intersect(o2, d2)
    ng = closest(hs, Rays(o2, d2), want=("normal",))[0]["normal"]
    hit = prim >= 0
    md = f32(max_distance)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.where(hit, np.minimum(t.astype(f32), md), md).astype(f32)
    bf = hit & (dot3(ng, d2) > 0)
    return d, r.reshape(n, spp), bf.reshape(n, spp)


class Guarded:
    """A device output with GUARD elements holding `fill` on both sides of it; get() insists that both runs survived and returns the
    array.  Exposes __cuda_array_interface__ (and ptr) of the array proper."""

    def __init__(self, shape, dtype=f32, fill=SENTINEL):
        self.shape, self.fill = tuple(int(v) for v in shape), fill
        self.buf = DevBuf(shape=(GUARD + int(np.prod(self.shape)),), dtype=dtype, fill=fill, guard=GUARD)
        self.ptr = self.buf.ptr + GUARD * self.buf.dtype.itemsize
        self.__cuda_array_interface__ = dict(self.buf.__cuda_array_interface__, shape=self.shape, data=(self.ptr, False))

    def get(self):
        whole = self.buf.get()  # (the run behind the output is checked there)
        assert (whole[:GUARD] == self.buf.dtype.type(self.fill)).all(), "guard elements in front of the output were overwritten"
        return whole[GUARD:].reshape(self.shape)


def depth_outputs(n):
    return {"moments": Guarded((n, ROW)), "counts": Guarded((n, 2), np.int32, COUNT_SENTINEL)}


def depth(hs, p, spp, max_distance, out=None, **kw):
    """query_probe_depth on the null stream for points uploaded here, into guarded buffers -> (moments, counts, info) as numpy."""
    out = out or depth_outputs(len(p))
    _, _, info = hs.query_probe_depth(DevBuf(np.ascontiguousarray(p, f32)), spp, max_distance, out=out, **kw)
    return out["moments"].get(), out["counts"].get(), info
