"""Radiance at sensors in device memory against the host route through mcpt_cast_rays, on the chess scene (SAH, quantised).  The command
behind profiles/sensor_query.txt.
python tools/sensor_query.py [--width 1920] [--height 1080] [--n 65536] [--spp 16 64] [--repeat 5]
The sensors are the first hits of n camera rays (pixels spread evenly over the frame, sample 0) from query_closest: the point and the
geometric normal, flipped towards the camera.  As rays (kind "ray") they leave the offset point p + n 1e-4 along n; as hemisphere probes
(kind "hemisphere") they are (p, n).  Per spp:
  (a) the host route: mcpt_cast_rays from host arrays with one entry per (sensor, sample, channel) and the keys (pixel = sensor, sample,
      channel), plus the numpy fold in sample order; wall time of both (the arrays are built before the clock starts)
  (b) query_radiance, kind "ray"; its radiance must equal (a)'s bit for bit
  (c) query_radiance, kind "hemisphere"
  (d) (b) with the variance
Each figure is the median of --repeat runs after one warm-up.  (b)-(d) are wall times of the blocking call on a stream of the tool's own;
sensors and outputs are resident.  Device buffers come from the HIP runtime the library is linked to, through ctypes; torch is not needed."""
import argparse
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tools')
import mcpt_loader  # noqa: E402
from ray_query import Dev, median_ms, runtime  # noqa: E402

f32 = np.float32


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--spp", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    hip.lib()
    sd = scenes.chess_scene(width=args.width, height=args.height, spp=1)
    hs = hip.HipScene(sd, builder="sah", quantise=1)
    rt = runtime()
    stream = C.c_void_p()
    assert rt.hipStreamCreate(C.byref(stream)) == 0
    sp = stream.value
    info = hs.info()
    print("chess %d x %d: %d primitives, tree height %d, quantised %d" % (args.width, args.height, info["n_prims"], info["bvh_height"], info["quantised"]))
    # sensors: the first hits of 4 n camera rays (a third of the frame's rays hit something), the first n that hit
    m, n_pix = 4 * args.n, args.width * args.height
    pix = (np.arange(m, dtype=np.uint64) * n_pix // m).astype(np.uint32)
    co, cd = hs.camera_rays(pix, np.zeros(m, np.uint32), seed=7)
    do, dd = Dev(rt, co), Dev(rt, cd)
    hit = {"prim": Dev(rt, shape=(m,), dtype=np.int32), "normal": Dev(rt, shape=(m, 3), dtype=f32), "point": Dev(rt, shape=(m, 3), dtype=f32)}
    hs.query_closest(do, dd, want=("prim", "normal", "point"), out=hit, stream=sp)
    assert rt.hipStreamSynchronize(stream) == 0
    keep = np.flatnonzero(hit["prim"].get() >= 0)[:args.n]
    n = len(keep)
    assert n == args.n, "only %d of %d camera rays hit" % (n, m)
    nrm, p, cd = hit["normal"].get()[keep], hit["point"].get()[keep], cd[keep]
    nrm = np.where(((nrm * cd).sum(1) < 0)[:, None], nrm, -nrm).astype(f32)
    ray_o = (p + (nrm * f32(1e-4)).astype(f32)).astype(f32)
    for x in [do, dd] + list(hit.values()):
        x.free()
    d_ro, d_p, d_n = Dev(rt, ray_o), Dev(rt, p), Dev(rt, nrm)
    out = {"radiance": Dev(rt, shape=(n, 3), dtype=f32), "variance": Dev(rt, shape=(n, 3), dtype=f32)}
    print("%d sensors" % n)
    print("%5s %16s %14s %16s %16s %8s %8s %8s %14s" % ("spp", "(a) cast + fold", "(b) ray", "(c) hemisphere", "(d) ray + var", "(a)/(b)", "(c)/(b)", "(d)/(b)",
                                                      "(b) Msamples/s"))
    for spp in args.spp:
        kw = dict(spp=spp, seed=args.seed)
        oo, dn = np.repeat(ray_o, spp * 3, axis=0), np.repeat(nrm, spp * 3, axis=0)
        kp = np.repeat(np.arange(n, dtype=np.uint32), spp * 3)
        ks = np.tile(np.repeat(np.arange(spp, dtype=np.uint32), 3), n)
        kc = np.tile(np.arange(3, dtype=np.int32), n * spp)
        res = {}

        def a():
            v = hs.cast_rays(oo, dn, kp, ks, kc, seed=args.seed).reshape(n, spp, 3)
            acc, tot = np.zeros((n, 3), f32), f32(spp)
            with np.errstate(invalid="ignore", over="ignore"):
                for k in range(spp):
                    acc += v[:, k, :] / tot
            res["a"] = acc

        def b():
            hs.query_radiance(d_ro, d_n, out=out, stream=sp, **kw)

        def c():
            hs.query_radiance(d_p, d_n, kind="hemisphere", out=out, stream=sp, **kw)

        def dv():
            hs.query_radiance(d_ro, d_n, variance=True, out=out, stream=sp, **kw)

        ms_a = median_ms(a, args.repeat)
        ms_b = median_ms(b, args.repeat)
        differ = int((~same_bits(out["radiance"].get(), res["a"])).sum())
        assert differ == 0, "%d values of (b) differ from (a)" % differ
        ms_c = median_ms(c, args.repeat)
        ms_d = median_ms(dv, args.repeat)
        print("%5d %13.1f ms %11.1f ms %13.1f ms %13.1f ms %8.2f %8.2f %8.2f %14.1f"
              % (spp, ms_a, ms_b, ms_c, ms_d, ms_a / ms_b, ms_c / ms_b, ms_d / ms_b, n * spp / ms_b / 1e3))
        del oo, dn, kp, ks, kc
    for x in [d_ro, d_p, d_n] + list(out.values()):
        x.free()
    hs.close()
    rt.hipStreamDestroy(stream)


if __name__ == "__main__":
    main()
