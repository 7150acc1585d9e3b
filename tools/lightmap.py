"""Bakes the lightmap of one object of a scene and writes it as a PNG; prints mcpt_lightmap_info.  The command behind profiles/lightmap.txt.
python tools/lightmap.py [--scene cornell|chess] [--object 0] [--triangles 0 1] [--size 256 1024] [--spp 16] [--dilate 2] [--repeat 5]
                         [--out lightmap.png] [--host-model]
The shipped models carry no texture coordinates, so the object gets a planar chart first (scenes.with_planar_uvs: --axes, --triangles; the
default is the Cornell box's floor, triangles 0 and 1 of object 0, projected onto x and z).  Per size: one warm-up bake, then --repeat
bakes; the figures are the medians of mcpt_lightmap_info's three legs (host wall clock inside the blocking call, on a stream of the tool's
own, image and coverage resident) and `grew` of the last bake, which is the steady state.  The texel pass alone is timed as well
(lightmap_texels into resident buffers).
--host-model: also the texel pass done the old way -- the numpy restatement of the rule from tests/lightmap_cases.py on the host's copy
of the mesh, then the upload of the sensors -- and a check that both give the same bits.
Device buffers come from the HIP runtime the library is linked to, through ctypes; torch is not needed."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", choices=("cornell", "chess"), default="cornell")
    ap.add_argument("--object", type=int, default=0)
    ap.add_argument("--triangles", type=int, nargs="*", default=None, help="triangles of the object that get the chart (default: 0 1 for cornell, all otherwise)")
    ap.add_argument("--axes", type=int, nargs=2, default=[0, 2])
    ap.add_argument("--size", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None, help="PNG of the last size's map")
    ap.add_argument("--host-model", action="store_true")
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    hip.lib()
    sd = scenes.cornell_demo(64, 64, 1) if args.scene == "cornell" else scenes.chess_scene(width=64, height=64, spp=1)
    tri = args.triangles if args.triangles else ([0, 1] if args.scene == "cornell" and args.object == 0 else None)
    sd = scenes.with_planar_uvs(sd, args.object, axes=tuple(args.axes), triangles=tri)
    hs = hip.HipScene(sd, builder="sah")
    rt = runtime()
    stream = C.c_void_p()
    assert rt.hipStreamCreate(C.byref(stream)) == 0
    sp = stream.value
    n_tri = int(sd.objects["n_tri"][args.object])
    print("%s, object %d: %d triangles, %d with a chart; spp %d, dilate %d, median of %d" % (args.scene, args.object, n_tri, len(tri) if tri else n_tri,
                                                                                          args.spp, args.dilate, args.repeat))
    print("%6s %9s %8s %11s %12s %11s %11s %5s %13s" % ("size", "texels", "items", "texels ms", "radiance ms", "scatter ms", "bake ms", "grew", "texel pass ms"))
    img = None
    for s in args.size:
        W = H = s
        out = {"image": Dev(rt, shape=(H, W, 3), dtype=f32), "coverage": Dev(rt, shape=(H, W), dtype=np.uint8)}
        tex = {"texel": Dev(rt, shape=(W * H,), dtype=np.int32), "origins": Dev(rt, shape=(W * H, 3), dtype=f32), "normals": Dev(rt, shape=(W * H, 3), dtype=f32)}
        infos, walls = [], []

        def bake():
            t0 = time.perf_counter()
            r = hs.bake_lightmap(args.object, W, H, dilate=args.dilate, out=out, stream=sp, spp=args.spp, seed=args.seed)
            walls.append((time.perf_counter() - t0) * 1e3)
            infos.append(r[3])

        bake()  # warm-up: the buffers grow here
        first = infos[0]
        del infos[:], walls[:]
        for _ in range(args.repeat):
            bake()
        med = {k: float(np.median([i[k] for i in infos])) for k in ("ms_texels", "ms_radiance", "ms_scatter")}

        def texel_pass():
            hs.lightmap_texels(args.object, W, H, want=("texel", "origins", "normals"), out=tex, stream=sp)
            assert rt.hipStreamSynchronize(stream) == 0

        ms_pass = median_ms(texel_pass, args.repeat)
        print("%6d %9d %8d %11.3f %12.3f %11.3f %11.3f %5d %13.3f" % (s, infos[-1]["n_texels"], infos[-1]["items"], med["ms_texels"], med["ms_radiance"],
                                                                    med["ms_scatter"], float(np.median(walls)), infos[-1]["grew"], ms_pass))
        print("       first bake at this size: grew %d, texels %.3f ms" % (first["grew"], first["ms_texels"]))
        if args.host_model:
            sys.path.insert(0, 'tests')
            import lightmap_cases as lc
            res, host = {}, {}

            def old_way():
                m = lc.model_texels(sd, args.object, W, H)
                for x in res.values():
                    x.free()
                res.update(texel=Dev(rt, m["texel"]), origins=Dev(rt, m["origins"]), normals=Dev(rt, m["normals"]))
                host.update(m)

            ms_old = median_ms(old_way, args.repeat)
            n = infos[-1]["n_texels"]
            same = all(lc.same_bits(tex[k].get()[:n], host[k]) for k in ("texel", "origins", "normals"))
            print("       numpy model on the host + upload of the sensors: %.1f ms (%.0f x the texel pass); same bits: %s" % (ms_old, ms_old / ms_pass, same))
            for x in res.values():
                x.free()
        img = out["image"].get()
        for x in list(out.values()) + list(tex.values()):
            x.free()
    if args.out and img is not None:
        pkg.pngio.write_png(args.out, pkg.pngio.tonemap_u8(img)[..., :3])
        print("wrote %s" % args.out)
    hs.close()
    rt.hipStreamDestroy(stream)


if __name__ == "__main__":
    main()
