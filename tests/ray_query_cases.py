"""Shared by tests/test_ray_query_abi.py, tests/test_gpu_ray_query.py and tests/ray_query_torch_child.py (include/mcpt.h:
mcpt_query_closest, mcpt_query_occluded): device buffers with guard elements made without torch, the occlusion rule restated in
float64, the fixed cycle of tmax values around a known hit distance, and the float64 restatement of the hit attributes."""
import ctypes as C

import numpy as np

from deform_cases import DeviceArray

f32, f64 = np.float32, np.float64
EPS = f64(f32(1e-4))          # kEps, the render loop's EPSILON, a float widened to double
DBL_MAX = np.finfo(f64).max
GUARD = 64                    # guard elements behind every output buffer
ALL = ("t", "prim", "object", "uv", "normal", "point")
# name -> (dtype, values per ray, sentinel)
OUTPUTS = {"t": (f64, 1, -7.25), "prim": (np.int32, 1, -77), "object": (np.int32, 1, -78), "uv": (f32, 2, -9.5), "normal": (f32, 3, -10.5),
           "point": (f32, 3, -11.5), "occluded": (np.uint8, 1, 0xAB)}
TYPESTR = {f32: "<f4", f64: "<f8", np.int32: "<i4", np.uint8: "|u1"}


class DevBuf:
    """An array in the memory of the current device, allocated through the HIP runtime the library is linked to (DeviceArray.runtime of
    tests/deform_cases.py).  `guard` elements holding `fill` follow the array proper; get() copies everything back, insists that they
    survived and returns the array.  Exposes __cuda_array_interface__."""

    def __init__(self, host=None, shape=None, dtype=f32, fill=0, guard=0):
        rt = DeviceArray.runtime()
        if host is not None:
            host = np.ascontiguousarray(host, dtype=dtype)
            shape = host.shape
        self.shape, self.dtype, self.fill, self.guard = tuple(int(s) for s in shape), np.dtype(dtype), fill, guard
        self.size = int(np.prod(self.shape))
        whole = np.full(self.size + guard, fill, dtype)
        if host is not None:
            whole[:self.size] = host.reshape(-1)
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), max(whole.nbytes, 4)) == 0
        self.ptr = p.value
        assert rt.hipMemcpy(self.ptr, whole.ctypes.data, whole.nbytes, 1) == 0  # hipMemcpyHostToDevice; blocking
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": TYPESTR[self.dtype.type], "data": (self.ptr, False), "strides": None, "version": 3}

    def get(self):
        whole = np.zeros(self.size + self.guard, self.dtype)
        # hipMemcpyDeviceToHost; blocking, and on the null stream behind whatever was enqueued there
        assert DeviceArray.runtime().hipMemcpy(whole.ctypes.data, self.ptr, whole.nbytes, 2) == 0
        assert (whole[self.size:] == self.dtype.type(self.fill)).all(), "guard elements behind the output were overwritten"
        return whole[:self.size].reshape(self.shape)

    def free(self):
        if self.ptr:
            DeviceArray.runtime().hipFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def out_buffer(name, n):
    dt, width, fill = OUTPUTS[name]
    return DevBuf(shape=(n,) if width == 1 else (n, width), dtype=dt, fill=fill, guard=GUARD)


class Rays:
    """Rays uploaded once."""

    def __init__(self, o, d, tmax=None):
        self.n = len(o)
        self.o, self.d = DevBuf(o), DevBuf(d)
        self.tmax = None if tmax is None else DevBuf(tmax)


def closest(hs, rays, want=("t", "prim"), enqueue_only=False):
    """query_closest on the null stream into fresh guarded buffers -> (dict of numpy arrays, info); enqueue_only: (dict of DevBuf, info)."""
    out = {w: out_buffer(w, rays.n) for w in want}
    res, info = hs.query_closest(rays.o, rays.d, rays.tmax, want=want, out=out)
    assert set(res) == set(want)
    if enqueue_only:
        return out, info
    return {w: out[w].get() for w in want}, info


def occluded(hs, rays, enqueue_only=False):
    out = out_buffer("occluded", rays.n)
    _, info = hs.query_occluded(rays.o, rays.d, rays.tmax, out=out)
    return (out if enqueue_only else out.get()), info


def expected_occluded(t, prim, tmax):
    """The occlusion rule in float64, no tolerance: ray i is occluded iff it hits and t_i - (double)tmax_i <= -eps."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((prim >= 0) & (np.asarray(t, f64) - np.asarray(tmax, f32).astype(f64) <= -EPS)).astype(np.uint8)


def tmax_cycle(t, prim):
    """tmax per ray from a fixed cycle over the hits: 0.5 t, float32(t), its two float32 neighbours on either side, float32(t + 3e-4), 2 t,
    inf, 0, -1, NaN.  Misses get inf and 1e30 in turn."""
    t = np.asarray(t, f64)
    hit = np.asarray(prim) >= 0
    ts = np.where(hit, t, 1.0)
    tf = ts.astype(f32)
    lo1, hi1 = np.nextafter(tf, f32(-np.inf)), np.nextafter(tf, f32(np.inf))
    lo2, hi2 = np.nextafter(lo1, f32(-np.inf)), np.nextafter(hi1, f32(np.inf))
    n = len(t)
    cand = np.stack([(0.5 * ts).astype(f32), tf, lo1, lo2, hi1, hi2, (ts + 3e-4).astype(f32), (2.0 * ts).astype(f32), np.full(n, np.inf, f32),
                     np.zeros(n, f32), np.full(n, -1, f32), np.full(n, np.nan, f32)], axis=1)
    rank = np.cumsum(hit) - 1   # the k-th hit takes entry k % 12
    out = cand[np.arange(n), np.where(hit, rank % cand.shape[1], 0)]
    miss_rank = np.cumsum(~hit) - 1
    return np.where(hit, out, np.where(miss_rank % 2 == 0, f32(np.inf), f32(1e30))).astype(f32)


def object_of(sd, prim):
    """The host lookup of a primitive id in the ranges of sd.objects (-1 for a miss)."""
    prim = np.asarray(prim)
    nt = len(sd.triangles)
    out = np.full(len(prim), -1, np.int32)
    for ob, o in enumerate(sd.objects):
        if o["kind"] == 0:
            a, n = int(o["first_tri"]), int(o["n_tri"])
            out[(prim >= a) & (prim < a + n)] = ob
    sph = prim >= nt
    out[sph] = prim[sph] - nt
    return out


def scene_extent(sd):
    v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]]).astype(f64)
    return float((v.max(0) - v.min(0)).max())


def check_attributes(sd, o, d, res, what=""):
    """The six outputs of query_closest against the description `sd` in float64 (the bounds are the issue's: float32 rounding at the
    Cornell scale of about 600 is about 6e-5 absolute)."""
    t, prim, obj, uv, nrm, pt = (res[k] for k in ALL)
    nt = len(sd.triangles)
    hit, miss = prim >= 0, prim < 0
    tri, sph = hit & (prim < nt), prim >= nt
    ext = scene_extent(sd)
    assert np.array_equal(obj, object_of(sd, prim)), what
    # misses
    assert (t[miss] == DBL_MAX).all() and (obj[miss] == -1).all()
    assert not uv[miss].any() and not nrm[miss].any() and not pt[miss].any()
    o64, d64 = o.astype(f64), d.astype(f64)
    # triangles
    T = sd.triangles[prim[tri]]
    v0, e1, e2 = T["v0"].astype(f64), T["v1"].astype(f64) - T["v0"].astype(f64), T["v2"].astype(f64) - T["v0"].astype(f64)
    u, v = uv[tri, 0].astype(f64), uv[tri, 1].astype(f64)
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1 + 1e-6).all()
    e_bary = np.abs(pt[tri] - (v0 + u[:, None] * e1 + v[:, None] * e2)).max()
    e_ray = np.abs(pt[tri] - (o64[tri] + t[tri, None] * d64[tri])).max()
    n_ref = np.cross(e1, e2)
    n_ref /= np.linalg.norm(n_ref, axis=1, keepdims=True)
    e_n = np.abs(nrm[tri] - n_ref).max()
    e_len = np.abs(np.linalg.norm(nrm[tri].astype(f64), axis=1) - 1).max()
    print("%s: %d triangle hits, |point - bary| %.3g, |point - ray| %.3g (extent %.4g), |normal error| %.3g, ||normal| - 1| %.3g"
          % (what, int(tri.sum()), e_bary, e_ray, ext, e_n, e_len))
    assert e_bary <= 1e-5 * ext and e_ray <= 1e-4 * ext and e_n <= 1e-5 and e_len <= 1e-6, what
    # spheres
    assert not uv[sph].any()
    if sph.any():
        c = sd.objects["center"][prim[sph] - nt].astype(f64)
        p = pt[sph].astype(f64)
        want = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
        e_s = np.abs(nrm[sph] - want).max()
        e_p = np.abs(p - (o64[sph] + t[sph, None].astype(f32).astype(f64) * d64[sph])).max()
        print("%s: %d sphere hits, |normal error| %.3g, |point - (o + d (float)t)| %.3g" % (what, int(sph.sum()), e_s, e_p))
        assert e_s <= 1e-5 and e_p <= 1e-4 * ext, what
    return int(tri.sum()), int(sph.sum())


class FakeDevice:
    """An object that only claims to be a device buffer (__cuda_array_interface__ over a made-up address): for the checks that run
    before the library is called."""

    def __init__(self, shape, typestr="<f4", strides=None, ptr=0x1000):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 3}
