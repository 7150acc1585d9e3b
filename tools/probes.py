"""A small probe grid in the Cornell demo scene against hemisphere sensors: what the SH-9 truncation plus the grid's trilinear interpolation
cost.  The command behind the "Light probes" figures of DESIGN.md section 6c.
python tools/probes.py [--dims 5 4 5] [--spp 16384] [--sensor-spp 262144] [--seed 3] [--visibility [--depth-spp 4096]]
python tools/probes.py --lit [--lit-out FILE.png] [--width 1920 --height 1080] [--ref-spp 256] [--direct N [N ...] [--indirect-only]]
The grid spans the box's interior.  At a handful of (point, normal) pairs in free space the tool prints the lookup (probe_shade on the
baked coefficients) next to query_radiance(kind="hemisphere") at the same point and normal, with the sensor's reported standard error:
both are E / pi.  Also printed: the lookup AT a probe against a sensor there (truncation alone, no interpolation), and the wall times of
the bake and of the lookup.  --visibility: the probes' depth maps are made as well (query_probe_depth at the grid's points) and the
occlusion-aware lookup (probe_shade_visible) is printed and summarised next to the plain one; without the flag the output is unchanged.
--lit: the volume of the same defaults (coefficients and depth maps) is baked, render_probe_lit draws the Cornell demo scene from it with
centre rays -- depth 0 and depth 2, occlusion-aware and plain, the host wall clock of each call next to one 1-spp render of the same camera
-- the occlusion-aware depth-2 frame is tone-mapped (HipScene.tonemap) and written as a PNG, and the tone-mapped RMSE of every lit frame
against a path-traced frame of --ref-spp samples is printed per region of the picture.  --direct N: after those, the occlusion-aware
frames at depth 0 and 2 with N light samples of the sampled direct term per surface sample (render_probe_lit(direct_samples=N)), timed
and compared in the same way, and the depth-2 frame of the last N written beside the other PNG; --indirect-only: they shade from a
second volume baked with indirect_only, the volume the term is meant for (without the flag: from the full volume, which counts the
direct light twice).  Without --direct the output is unchanged.
python tools/probes.py --relight ITER [--hysteresis 0.7] [--relight-spp 256] [--direct N] [--indirect-only] [--scene cornell|chess] [--repeat 10]
--relight ITER: starting from a zero volume, relight_probe_volume is iterated ITER times with a new seed per update, for hysteresis 0 and
--hysteresis; after every update the RMS difference of E / pi between the relit volume and the path-traced bake_probe_volume of the same
grid (--spp; full, or indirect-only with --indirect-only, which goes with --direct N) is printed, taken at the surface points of a 160 x 90
centre-ray frame with the occlusion-aware lookup.  Then the wall time of one update against one bake at the same samples per probe (warm-up
runs, the median and the spread of --repeat runs, each timed to the end of the device work), and on the Cornell scene the short box is
moved and ITER more updates from the now stale volume are compared with a fresh bake of the moved scene.
Device buffers come from the HIP runtime the library is linked to, through ctypes; torch is not needed."""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tools')
import mcpt_loader  # noqa: E402
from ray_query import Dev, runtime  # noqa: E402

f32 = np.float32


def lit(args):
    """--lit: bake, render the lit frames, time them, write the PNG, compare with a path-traced frame."""
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    W, H = args.width, args.height
    sd = pkg.scenes.cornell_demo(W, H, 4)
    hs = hip.HipScene(sd, builder="sah")
    rt = runtime()
    dims = tuple(args.dims)
    lo, hi = np.array([40.0, 40.0, 40.0]), np.array([516.0, 500.0, 516.0])
    origin, spacing = tuple(lo), tuple((hi - lo) / np.maximum(np.array(dims) - 1, 1))
    m = dims[0] * dims[1] * dims[2]
    max_distance = 1.5 * float(np.linalg.norm(spacing))
    vol = {"sh": Dev(rt, shape=(m, 27)), "moments": Dev(rt, shape=(m, hip.PROBE_DEPTH_ROW)), "counts": Dev(rt, shape=(m, 2), dtype=np.int32)}
    t0 = time.perf_counter()
    hs.bake_probe_volume(origin, spacing, dims, args.depth_spp, max_distance, depth_seed=args.seed + 2, out=vol, spp=args.spp, seed=args.seed)
    print("volume %dx%dx%d = %d probes at %d spp, depth maps at %d spp, max_distance %.1f: bake %.1f ms"
          % (dims + (m, args.spp, args.depth_spp, max_distance, (time.perf_counter() - t0) * 1e3)))
    # the reference first: it leaves the wavefront workspace the lit calls then work in, as in an interactive session
    t0 = time.perf_counter()
    ref, _ = hs.render(spp=args.ref_spp, seed=args.seed + 7)
    t_ref = (time.perf_counter() - t0) * 1e3
    hs.render(spp=1, seed=1)
    t0 = time.perf_counter()
    _, st = hs.render(spp=1, seed=2)
    t_one = (time.perf_counter() - t0) * 1e3
    print("%d x %d: path-traced reference at %d spp %.1f ms; one 1-spp render %.2f ms wall clock with its read-back (%.2f ms in the library)"
          % (W, H, args.ref_spp, t_ref, t_one, st.ms_total))
    out = {"lit": Dev(rt, shape=(H, W, 3))}
    ref8 = hs.tonemap(ref)[..., :3].astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    u, v = (x + 0.5) / W, (y + 0.5) / H
    mid = (np.abs(u - 0.5) < 0.5 * H / W * 0.98)  # the box's opening: the frame is wider than the box is
    regions = [("whole frame", np.ones((H, W), bool)), ("ceiling and light (top fifth of the box)", mid & (v < 0.2)),
               ("left wall (rough red conductor)", mid & (u < 0.5 - 0.3 * H / W)), ("right wall (gold conductor)", mid & (u > 0.5 + 0.3 * H / W)),
               ("floor (bottom fifth)", mid & (v > 0.8)), ("centre (boxes, spheres, back wall)", (np.abs(u - 0.5) < 0.25 * H / W) & (np.abs(v - 0.5) < 0.25))]
    frames = {}
    for depth in (0, 2):
        for visible in (True, False):
            kw = dict(moments=vol["moments"], counts=vol["counts"], normal_bias=args.normal_bias) if visible else {}
            hs.render_probe_lit(origin, spacing, dims, vol["sh"], centre=True, specular_depth=depth, out=out, **kw)  # (warm: code objects, the counter)
            t0 = time.perf_counter()
            _, _, info = hs.render_probe_lit(origin, spacing, dims, vol["sh"], centre=True, specular_depth=depth, out=out, **kw)
            t_call = (time.perf_counter() - t0) * 1e3
            fb = out["lit"].get()
            frames[(depth, visible)] = fb
            d8 = hs.tonemap(fb)[..., :3].astype(np.float64) - ref8
            print("lit frame, specular_depth %d, %s lookup: %.3f ms wall clock (%.3f ms in the library), %d chunk(s), in_workspace %d, %d lookups of %d samples"
                  % (depth, "occlusion-aware" if visible else "plain", t_call, info["ms_total"], info["chunks"], info["in_workspace"], info["lookups"],
                     info["samples"]))
            print("    tone-mapped RMSE against the reference (0..255): " + "; ".join("%s %.2f" % (nm, np.sqrt((d8[mk] ** 2).mean())) for nm, mk in regions if mk.any()))
    pkg.pngio.write_png(args.lit_out, hs.tonemap(frames[(2, True)])[..., :3])
    print("wrote %s (specular_depth 2, occlusion-aware)" % args.lit_out)
    if args.direct:
        dvol = vol
        if args.indirect_only:
            dvol = {"sh": Dev(rt, shape=(m, 27)), "moments": vol["moments"], "counts": vol["counts"]}
            t0 = time.perf_counter()
            hs.bake_probe_grid(origin, spacing, dims, out=dvol["sh"], spp=args.spp, seed=args.seed, indirect_only=True)
            print("indirect-only volume (the same seeds; the depth maps are the full volume's): bake %.1f ms" % ((time.perf_counter() - t0) * 1e3))
        kw = dict(moments=dvol["moments"], counts=dvol["counts"], normal_bias=args.normal_bias)
        for N in args.direct:
            for depth in (0, 2):
                call = lambda: hs.render_probe_lit(origin, spacing, dims, dvol["sh"], centre=True, specular_depth=depth, out=out, direct_samples=N,  # noqa: E731
                                                   direct_seed=args.seed + 11, **kw)
                call()
                t0 = time.perf_counter()
                _, _, info = call()
                t_call = (time.perf_counter() - t0) * 1e3
                fb = out["lit"].get()
                d8 = hs.tonemap(fb)[..., :3].astype(np.float64) - ref8
                print("lit frame with direct light, %s volume, N %d, specular_depth %d: %.3f ms wall clock (%.3f ms in the library), %d chunk(s), %d piece(s), "
                      "%d light samples, %d shadow rays (%.1f %% of the lanes dead)"
                      % ("indirect-only" if args.indirect_only else "full", N, depth, t_call, info["ms_total"], info["chunks"], info["pieces"], info["light_samples"],
                         info["shadow_rays"], 100.0 * (1 - info["shadow_rays"] / max(info["light_samples"], 1))))
                print("    tone-mapped RMSE against the reference (0..255): " + "; ".join("%s %.2f" % (nm, np.sqrt((d8[mk] ** 2).mean())) for nm, mk in regions if mk.any()))
        name = args.lit_out[:-4] + "_direct.png" if args.lit_out.endswith(".png") else args.lit_out + "_direct"
        pkg.pngio.write_png(name, hs.tonemap(fb)[..., :3])
        print("wrote %s (specular_depth 2, N %d)" % (name, args.direct[-1]))
    hs.close()


def timed(call, sync, warm, repeat):
    """(median, min, max) ms of `repeat` runs of call() + sync() after `warm` warm-up runs."""
    for _ in range(warm):
        call()
        sync()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def relight(args):
    """--relight ITER: iterate relight_probe_volume from a zero volume and compare with the path-traced bake; time both; move an object."""
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    W, H = 160, 90
    dims = tuple(args.dims)
    if args.scene == "chess":
        sd = pkg.scenes.chess_scene(width=W, height=H, spp=4)
        hs = hip.HipScene(sd, builder="sah", quantise=1)
        v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]]).astype(np.float64)
        mid, half = (v.min(0) + v.max(0)) / 2, (v.max(0) - v.min(0)) / 2 * 0.8
        lo, hi = mid - half, mid + half
    else:
        sd = pkg.scenes.cornell_demo(W, H, 4)
        hs = hip.HipScene(sd, builder="sah")
        lo, hi = np.array([40.0, 40.0, 40.0]), np.array([516.0, 500.0, 516.0])
    rt = runtime()
    sync = lambda: rt.hipStreamSynchronize(None)  # noqa: E731
    origin, spacing = tuple(lo), tuple((hi - lo) / np.maximum(np.array(dims) - 1, 1))
    m = dims[0] * dims[1] * dims[2]
    max_distance = 1.5 * float(np.linalg.norm(spacing))
    N, io, spp = args.direct[0] if args.direct else 0, args.indirect_only, args.relight_spp
    print("%s, grid %dx%dx%d = %d probes; update: %d probe rays per probe, hysteresis %g, %d light samples per hit, indirect_only %d; "
          "bake: %d spp, depth maps %d spp" % (args.scene, *dims, m, spp, args.hysteresis, N, int(io), args.spp, args.depth_spp))

    def volume():
        return {"sh": Dev(rt, np.zeros((m, 27), f32)), "moments": Dev(rt, np.zeros((m, hip.PROBE_DEPTH_ROW), f32)), "counts": Dev(rt, np.zeros((m, 2), np.int32))}

    def bake(vol, n_spp, seed):
        hs.bake_probe_volume(origin, spacing, dims, args.depth_spp, max_distance, depth_seed=args.seed + 2, out=vol, spp=n_spp, seed=seed, indirect_only=io)

    # the surface points of a centre-ray frame, with the normals that face the camera
    o, d = hs.centre_rays(np.arange(W * H, dtype=np.uint32))
    dpts = Dev(rt, hip.probe_grid_points(origin, spacing, dims))

    def surface():
        do, dd = Dev(rt, o), Dev(rt, d)
        res, _ = hs.query_closest(do, dd, want=("t", "prim", "normal"), out={"t": Dev(rt, shape=(len(o),), dtype=np.float64),
                                                                             "prim": Dev(rt, shape=(len(o),), dtype=np.int32), "normal": Dev(rt, shape=(len(o), 3))})
        t, ng = res["t"].get(), res["normal"].get()
        hit = res["prim"].get() >= 0
        t = np.where(hit, t, 0.0)
        p = (o + d * t.astype(f32)[:, None])[hit].astype(f32)
        nf = np.where(((ng * d).sum(axis=1) > 0)[:, None], -ng, ng)[hit].astype(f32)
        return Dev(rt, p), Dev(rt, nf), int(hit.sum())

    def e_over_pi(vol, pts):
        out = Dev(rt, shape=(pts[2], 3))
        hs.probe_shade_visible(origin, spacing, dims, vol["sh"], vol["moments"], vol["counts"], pts[0], pts[1], normal_bias=args.normal_bias, out=out)
        return out.get().astype(np.float64)

    def update(src, dst, seed, h):
        hs.relight_probe_volume(origin, spacing, dims, src["sh"], src["moments"], src["counts"], normal_bias=args.normal_bias, spp=spp, seed=seed, hysteresis=h,
                                indirect_only=io, direct_samples=N, direct_seed=seed + 1000, out={"sh": dst["sh"]})

    def iterate(ref, pts, iters, h, start=None, what=""):
        """iters updates, a new seed each, between two volumes that share the live scene's depth maps -> the last volume."""
        a, b = volume(), volume()
        hs.query_probe_depth(dpts, args.depth_spp, max_distance, seed=args.seed + 2, out={"moments": a["moments"], "counts": a["counts"]})
        b["moments"], b["counts"] = a["moments"], a["counts"]
        if start is not None:
            a["sh"] = start["sh"]
        want = e_over_pi(ref, pts)
        print("%s hysteresis %g: RMS of E/pi (relit - baked) over %d surface points, the baked mean is %.4f" % (what, h, pts[2], want.mean()))
        for it in range(iters):
            update(a, b, args.seed + 100 + it, h)
            a, b = b, a
            got = e_over_pi(a, pts)
            print("    update %2d: rms %.5f  (relative to the baked mean %.4f), relit mean %.4f" % (it + 1, np.sqrt(((got - want) ** 2).mean()),
                                                                                                   np.sqrt(((got - want) ** 2).mean()) / want.mean(), got.mean()))
        return a

    ref = volume()
    bake(ref, args.spp, args.seed)
    sync()
    pts = surface()
    last = None
    for h in sorted({0.0, args.hysteresis}):
        last = iterate(ref, pts, args.relight, h, what="from a zero volume,")
    # time: one update against one bake at the same samples per probe
    scratch, tmp = volume(), volume()
    t_upd = timed(lambda: update(last, scratch, args.seed + 7, args.hysteresis), sync, 3, args.repeat)
    t_bake = timed(lambda: bake(tmp, spp, args.seed + 9), sync, 2, args.repeat)
    print("time, %d probes x %d samples: update %.3f ms (min %.3f, max %.3f); bake_probe_volume_ex %.3f ms (min %.3f, max %.3f), of %d runs each; bake / update = %.1f"
          % (m, spp, *t_upd, *t_bake, args.repeat, t_bake[0] / t_upd[0]))
    if args.scene == "cornell":
        move = np.array([[1, 0, 0, 120.0], [0, 1, 0, 0.0], [0, 0, 1, -60.0]], f32)
        hs.update([(1, move)])  # the short box
        moved = volume()
        bake(moved, args.spp, args.seed)
        sync()
        pts = surface()
        stale = np.sqrt(((e_over_pi(last, pts) - e_over_pi(moved, pts)) ** 2).mean())
        print("the short box moved by (120, 0, -60); the stale volume against a fresh bake of the moved scene: rms %.5f" % stale)
        iterate(moved, pts, args.relight, args.hysteresis, start=last, what="after the move, from the stale volume,")
    hs.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--relight", type=int, default=0, metavar="ITER", help="iterate relight_probe_volume ITER times from a zero volume (see the module text)")
    ap.add_argument("--hysteresis", type=float, default=0.7, help="share of the previous coefficients an update keeps (--relight)")
    ap.add_argument("--relight-spp", type=int, default=256, help="probe rays per probe and update (--relight)")
    ap.add_argument("--scene", choices=("cornell", "chess"), default="cornell", help="the scene of --relight (chess: timing and convergence only, nothing moves)")
    ap.add_argument("--repeat", type=int, default=10, help="timed runs per figure (--relight)")
    ap.add_argument("--dims", type=int, nargs=3, default=[5, 4, 5])
    ap.add_argument("--spp", type=int, default=16384)
    ap.add_argument("--sensor-spp", type=int, default=262144)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--visibility", action="store_true", help="also the occlusion-aware lookup (probe depth maps, probe_shade_visible)")
    ap.add_argument("--depth-spp", type=int, default=4096, help="samples per probe of the depth maps (--visibility)")
    ap.add_argument("--normal-bias", type=float, default=2.0, help="normal_bias of the occlusion-aware lookup, in scene units (--visibility)")
    ap.add_argument("--lit", action="store_true", help="render probe-lit frames from the baked volume and compare them with a path-traced frame")
    ap.add_argument("--lit-out", default="probe_lit.png", help="the PNG of the occlusion-aware depth-2 frame (--lit)")
    ap.add_argument("--width", type=int, default=1920, help="frame width (--lit)")
    ap.add_argument("--height", type=int, default=1080, help="frame height (--lit)")
    ap.add_argument("--ref-spp", type=int, default=256, help="samples per pixel of the path-traced reference frame (--lit)")
    ap.add_argument("--direct", type=int, nargs="+", default=[], metavar="N", help="also frames with N light samples of the sampled direct term (--lit)")
    ap.add_argument("--indirect-only", action="store_true", help="the --direct frames shade from a volume baked with indirect_only (--lit)")
    args = ap.parse_args()
    if args.relight:
        return relight(args)
    if args.lit:
        return lit(args)
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah")
    rt = runtime()
    dims = tuple(args.dims)
    lo, hi = np.array([40.0, 40.0, 40.0]), np.array([516.0, 500.0, 516.0])
    origin = tuple(lo)
    spacing = tuple((hi - lo) / np.maximum(np.array(dims) - 1, 1))
    m = dims[0] * dims[1] * dims[2]
    sh = Dev(rt, shape=(m, 27))
    t0 = time.perf_counter()
    _, st = hs.bake_probe_grid(origin, spacing, dims, out=sh, spp=args.spp, seed=args.seed)
    t_bake = (time.perf_counter() - t0) * 1e3
    print("grid %dx%dx%d = %d probes, spacing %s, %d spp: bake %.1f ms (%d samples, %d wavefront iterations; resolve kernels %.3f ms in %d launches)"
          % (dims + (m, np.round(spacing, 1), args.spp, t_bake, st.samples, st.iterations, st.ms_resolve, st.n_resolve)))
    pts = hip.probe_grid_points(origin, spacing, dims)
    # free-space points: above the boxes and the spheres, and in the open front part of the room; three normals each
    P = np.array([[278, 420, 278], [150, 450, 150], [430, 380, 120], [278, 250, 60], [80, 200, 120], [480, 120, 80]], f32)
    N = np.array([[0, 1, 0], [0, -1, 0], [0.57735027, 0.57735027, -0.57735027]], f32)
    # ... and two probes themselves (interpolation weights 1 and 0): the truncation alone
    at = pts[[m // 2, m - dims[0] * dims[1] // 2 - 1]]
    p = np.repeat(np.concatenate([P, at]), len(N), axis=0)
    n = np.tile(N, (len(P) + len(at), 1))
    dp, dn = Dev(rt, p), Dev(rt, n)
    out = Dev(rt, shape=(len(p), 3))
    t0 = time.perf_counter()
    hs.probe_shade(origin, spacing, dims, sh, dp, dn, out=out)
    look = out.get()
    t_look = (time.perf_counter() - t0) * 1e3
    if args.visibility:
        max_distance = 1.5 * float(np.linalg.norm(spacing))
        dpts = Dev(rt, pts)
        dm = {"moments": Dev(rt, shape=(m, hip.PROBE_DEPTH_ROW)), "counts": Dev(rt, shape=(m, 2), dtype=np.int32)}
        t0 = time.perf_counter()
        _, _, qi = hs.query_probe_depth(dpts, args.depth_spp, max_distance, seed=args.seed + 2, out=dm)
        counts = dm["counts"].get()
        t_depth = (time.perf_counter() - t0) * 1e3
        vout = Dev(rt, shape=(len(p), 3))
        t0 = time.perf_counter()
        hs.probe_shade_visible(origin, spacing, dims, sh, dm["moments"], dm["counts"], dp, dn, normal_bias=args.normal_bias, backface_max=0.25, out=vout)
        vlook = vout.get()
        t_vlook = (time.perf_counter() - t0) * 1e3
        print("visibility: depth maps at %d spp, max_distance %.1f: %.1f ms with the read-back (%d launches); %d of %d probes have more than a quarter "
              "of their samples back-facing; occlusion-aware lookup of %d pairs (normal_bias %.1f): %.2f ms"
              % (args.depth_spp, max_distance, t_depth, qi["launches"], int((counts[:, 1] > 0.25 * counts[:, 0]).sum()), m, len(p), args.normal_bias, t_vlook))
    so = {"radiance": Dev(rt, shape=(len(p), 3)), "variance": Dev(rt, shape=(len(p), 3))}
    hs.query_radiance(dp, dn, kind="hemisphere", variance=True, out=so, spp=args.sensor_spp, seed=args.seed + 1)
    ref, se = so["radiance"].get(), np.sqrt(so["variance"].get())
    print("lookup of %d pairs: %.2f ms (first call, with its read-back); hemisphere sensors at %d spp" % (len(p), t_look, args.sensor_spp))
    print("%-22s %-22s %-28s %-28s %-10s %s" % ("point", "normal", "lookup E/pi (rgb)", "sensor E/pi (rgb)", "rel. diff", "sensor s.e. / value"))
    rel_all = []
    for i in range(len(p)):
        lum_l, lum_r = look[i].mean(), ref[i].mean()
        rel = abs(lum_l - lum_r) / max(lum_r, 1e-12)
        rel_all.append(rel)
        tag = "  (at a probe)" if i >= len(P) * len(N) else ""
        if not (lum_r > 0):  # zero: the point lies inside an object; NaN: one of the sensor's samples was not finite.  Left out of the summary
            rel_all[-1] = np.nan
            tag += "  (sensor zero or not finite: skipped)"
        print("%-22s %-22s %-28s %-28s %-10.4f %.4f%s" % (np.round(p[i], 1), np.round(n[i], 2), np.round(look[i], 4), np.round(ref[i], 4), rel,
                                                          se[i].mean() / max(lum_r, 1e-12), tag))
    rel_all = np.array(rel_all)
    k = len(P) * len(N)
    if args.visibility:
        print("%-22s %-22s %-28s %-28s %-10s %s" % ("point", "normal", "visible lookup E/pi (rgb)", "plain lookup E/pi (rgb)", "rel. diff", "plain rel. diff"))
        rel_vis = []
        for i in range(len(p)):
            lum_v, lum_r = vlook[i].mean(), ref[i].mean()
            rel_vis.append(abs(lum_v - lum_r) / max(lum_r, 1e-12) if lum_r > 0 else np.nan)
            print("%-22s %-22s %-28s %-28s %-10.4f %.4f" % (np.round(p[i], 1), np.round(n[i], 2), np.round(vlook[i], 4), np.round(look[i], 4), rel_vis[-1], rel_all[i]))
        rel_vis = np.array(rel_vis)
        print("occlusion-aware lookup, relative difference of the channel mean: interpolated pairs mean %.4f, max %.4f; at probes mean %.4f, max %.4f; "
              "negative lookups: %d" % (np.nanmean(rel_vis[:k]), np.nanmax(rel_vis[:k]), np.nanmean(rel_vis[k:]), np.nanmax(rel_vis[k:]), int((vlook < 0).sum())))
    print("relative difference of the channel mean: interpolated pairs mean %.4f, max %.4f; at probes mean %.4f, max %.4f; negative lookups: %d"
          % (np.nanmean(rel_all[:k]), np.nanmax(rel_all[:k]), np.nanmean(rel_all[k:]), np.nanmax(rel_all[k:]), int((look < 0).sum())))
    hs.close()


if __name__ == "__main__":
    main()
