"""Ray queries on device memory against mcpt_intersect, on the chess scene.  The command behind profiles/ray_query.txt.
python tools/ray_query.py [--width 1920] [--height 1080] [--repeat 5]
Three ray sets: 2^20 camera rays of the frame (pixels spread evenly over it, sample 0), 2^20 random rays inside the scene's box, and 2^16
of the camera rays.  Per set:
  (a) mcpt_intersect, wall time of the call (host arrays in, host arrays out)
  (b) query_closest, want = (t, prim)
  (c) query_closest, all six outputs
  (d) query_occluded, tmax = inf ("is anything hit")
  (e) query_occluded, tmax just short of the hit (0.999 t): nothing is occluded, so every walk runs to its end
Each figure is the median of --repeat runs after one warm-up.  (b)-(e) are timed from the enqueue on a stream of the tool's own to the
return of hipStreamSynchronize; their rays and outputs are resident.  `grew` is that of the second call.
Device buffers come from the HIP runtime the library is linked to, through ctypes; torch is not needed."""
import argparse
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402

f32 = np.float32
TYPESTR = {np.dtype(f32): "<f4", np.dtype(np.float64): "<f8", np.dtype(np.int32): "<i4", np.dtype(np.uint8): "|u1"}


def runtime():
    paths = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
    assert paths, "the HIP runtime is not loaded: load the library first"
    rt = C.CDLL(paths[0])
    rt.hipMalloc.argtypes, rt.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    rt.hipMemcpy.argtypes, rt.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    rt.hipFree.argtypes, rt.hipFree.restype = [C.c_void_p], C.c_int
    rt.hipStreamCreate.argtypes, rt.hipStreamCreate.restype = [C.POINTER(C.c_void_p)], C.c_int
    rt.hipStreamSynchronize.argtypes, rt.hipStreamSynchronize.restype = [C.c_void_p], C.c_int
    rt.hipStreamDestroy.argtypes, rt.hipStreamDestroy.restype = [C.c_void_p], C.c_int
    return rt


class Dev:
    """A device array that exposes __cuda_array_interface__."""

    def __init__(self, rt, host=None, shape=None, dtype=f32):
        self.rt = rt
        if host is not None:
            host = np.ascontiguousarray(host)
            shape, dtype = host.shape, host.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), max(nbytes, 4)) == 0
        self.ptr = p.value
        if host is not None:
            assert rt.hipMemcpy(self.ptr, host.ctypes.data, nbytes, 1) == 0
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": TYPESTR[self.dtype], "data": (self.ptr, False), "strides": None, "version": 3}

    def get(self):
        out = np.zeros(self.shape, self.dtype)
        assert self.rt.hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) == 0
        return out

    def free(self):
        if self.ptr:
            self.rt.hipFree(self.ptr)
            self.ptr = None


def median_ms(call, repeat):
    call()  # warm-up
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    hip.lib()
    sd = scenes.chess_scene(width=args.width, height=args.height, spp=1)
    hs = hip.HipScene(sd)
    rt = runtime()
    stream = C.c_void_p()
    assert rt.hipStreamCreate(C.byref(stream)) == 0
    info = hs.info()
    print("chess %d x %d: %d primitives, tree height %d, quantised %d" % (args.width, args.height, info["n_prims"], info["bvh_height"], info["quantised"]))
    n_big, n_small = 1 << 20, 1 << 16
    n_pix = args.width * args.height
    pix = (np.arange(n_big, dtype=np.uint64) * n_pix // n_big).astype(np.uint32)
    co, cd = hs.camera_rays(pix, np.zeros(n_big, np.uint32), seed=7)
    v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]])
    rng = np.random.default_rng(1)
    ro = rng.uniform(v.min(0), v.max(0), (n_big, 3)).astype(f32)
    rd = rng.normal(size=(n_big, 3))
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(f32)
    step = n_big // n_small
    sets = [("2^20 camera rays", co, cd), ("2^20 random rays", ro, rd), ("2^16 camera rays", co[::step].copy(), cd[::step].copy())]
    names = ("t", "prim", "object", "uv", "normal", "point")
    shapes = {"t": ((), np.float64), "prim": ((), np.int32), "object": ((), np.int32), "uv": ((2,), f32), "normal": ((3,), f32), "point": ((3,), f32)}
    print("%-18s %6s %12s %12s %12s %12s %12s %8s %8s %8s %5s" % ("rays", "hit", "(a) intersect", "(b) t, prim", "(c) all six", "(d) occ inf", "(e) occ short",
                                                                   "(a)/(b)", "(d)/(b)", "(e)/(b)", "grew"))
    for label, o, d in sets:
        n = len(o)
        t, prim = hs.intersect(o, d)
        do, dd = Dev(rt, o), Dev(rt, d)
        t_inf = Dev(rt, np.full(n, np.inf, f32))
        t_short = Dev(rt, np.where(prim >= 0, 0.999 * t, 1e30).astype(f32))
        out = {k: Dev(rt, shape=(n,) + shapes[k][0], dtype=shapes[k][1]) for k in names}
        occ = Dev(rt, shape=(n,), dtype=np.uint8)
        sp = stream.value
        grew = []

        def sync():
            assert rt.hipStreamSynchronize(stream) == 0

        def b():
            grew.append(hs.query_closest(do, dd, want=("t", "prim"), out=out, stream=sp)[1]["grew"])
            sync()

        def c():
            hs.query_closest(do, dd, want=names, out=out, stream=sp)
            sync()

        def dq():
            hs.query_occluded(do, dd, t_inf, out=occ, stream=sp)
            sync()

        def e():
            hs.query_occluded(do, dd, t_short, out=occ, stream=sp)
            sync()

        ms_a = median_ms(lambda: hs.intersect(o, d), args.repeat)
        ms_b = median_ms(b, args.repeat)
        assert np.array_equal(out["prim"].get(), prim) and np.array_equal(out["t"].get().view(np.uint64), t.view(np.uint64))
        ms_c = median_ms(c, args.repeat)
        ms_d = median_ms(dq, args.repeat)
        assert np.array_equal(occ.get(), (prim >= 0).astype(np.uint8))
        ms_e = median_ms(e, args.repeat)
        assert not occ.get().any()
        print("%-18s %6.3f %10.3f ms %9.3f ms %9.3f ms %9.3f ms %9.3f ms %8.2f %8.2f %8.2f %5d"
              % (label, (prim >= 0).mean(), ms_a, ms_b, ms_c, ms_d, ms_e, ms_a / ms_b, ms_d / ms_b, ms_e / ms_b, grew[1]))
        for x in [do, dd, t_inf, t_short, occ] + list(out.values()):
            x.free()
    hs.close()
    rt.hipStreamDestroy(stream)


if __name__ == "__main__":
    main()
