"""Relighting a live scene: what mcpt_scene_set_materials and mcpt_scene_set_environment cost beside the alternatives.  The command behind
profiles/scene_materials.txt.
python tools/materials.py [--scenes chess,chess_high] [--builders sah,ploc] [--repeats 7] [--out profiles/scene_materials.txt]
Per scene and builder it times, in one warm process on one scene handle (the median of --repeats calls after one that warms up):
  one material      the king's material recoloured                                   (path 2, no primitive record touched)
  all materials     every non-emitting material recoloured in one call               (path 2)
  one piece         the king given another material                                   (path 2, the king's triangle records patched)
  texture toggle    the floor's `textured` flag flipped                               (path 2, the floor's triangle records patched)
  light dimmed      the emitter's emission scaled                                     (path 2)
  light off / on    the emitter switched off, then on again: two calls                (path 0 each: the host flatten and the tree build)
  sky: a map        a 64 x 32 map (every other call 63 x 32: the size changes)
  sky: a colour     back to a constant colour
  identity update   mcpt_scene_update of the king with the transform it already has (the yardstick: what moving the same object costs)
  destroy + create  the parent's only way to change a material
Columns: total_ms / transform_ms / build_ms / upload_ms of mcpt_update_info, and the wall time of the Python call.  The wall column of
the path-0 rows has been seen to sit on multiples of 50 ms while total_ms, taken inside the library around the same work, does not:
quote total_ms for those rows."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402

f32 = np.float32


def with_fields(m, **kw):
    """A copy of the material record m (scenes.MAT_DTYPE) with fields replaced."""
    m2 = np.zeros((), dtype=m.dtype)
    for name in m.dtype.names:
        m2[name] = m[name]
    for k, v in kw.items():
        m2[k] = v
    return m2


def recoloured(m, k):
    return with_fields(m, base_reflectance=np.asarray([0.3 + 0.05 * (k % 7), 0.5, 0.9 - 0.05 * (k % 5)], f32))


def timed(call, repeats):
    infos = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        info = call(k)
        wall = (time.perf_counter() - t0) * 1e3
        if isinstance(info, list):  # several calls: their sums
            info = {key: (sum(i[key] for i in info) if key != "path" else info[0]["path"]) for key in info[0]}
        info = dict(info or {})
        info["wall_ms"] = wall
        infos.append(info)
    infos = infos[1:]
    return {key: float(np.median([i.get(key, 0.0) for i in infos])) for key in ("total_ms", "transform_ms", "build_ms", "upload_ms", "wall_ms")}, infos[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="chess,chess_high")
    ap.add_argument("--builders", default="sah,ploc")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "scene_materials.txt"))
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    pkg.build.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# python tools/materials.py --scenes %s --builders %s --repeats %d   (%s)" % (args.scenes, args.builders, args.repeats, hip.lib().mcpt_version().decode()))
    for scene in args.scenes.split(","):
        sd = scenes.chess_scene(width=96, height=54, spp=1) if scene == "chess" else scenes.chess_high(width=96, height=54, spp=1)
        M, O = sd.materials, sd.objects
        em = np.sqrt((M["emission"].astype(f32) ** 2).sum(-1)) > 1e-4
        light = int(np.flatnonzero(em)[0])
        meshes = [o for o in range(len(O)) if O["kind"][o] == 0 and not em[O["material"][o]]]
        king = max(meshes, key=lambda o: int(O["n_tri"][o]))
        floor = next(o for o in meshes if M["textured"][O["material"][o]])
        king_mat, floor_mat = int(O["material"][king]), int(O["material"][floor])
        other = next(int(m) for m in range(len(M)) if not em[m] and m not in (king_mat, floor_mat))
        sky = np.ascontiguousarray(np.random.default_rng(1).uniform(0, 1, (32, 64, 3)), dtype=f32)
        ident = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
        for builder in args.builders.split(","):
            hs = hip.HipScene(sd, builder=builder)
            hs.render(spp=1, seed=1)  # the workspace exists: a warm handle
            say("")
            say("%s, %s: %d triangles, %d objects, %d materials; the king has %d triangles, the floor %d" % (scene, builder, len(sd.triangles), len(O), len(M), int(O["n_tri"][king]), int(O["n_tri"][floor])))
            say("%-18s %4s %9s %9s %9s %9s %9s %9s" % ("edit", "path", "records", "total", "transform", "build", "upload", "wall"))
            rows = [
                ("one material", lambda k: hs.set_materials([(king_mat, recoloured(M[king_mat], k))])),
                ("all materials", lambda k: hs.set_materials([(m, recoloured(M[m], k + m)) for m in range(len(M)) if not em[m]])),
                ("one piece", lambda k: hs.set_materials([], [(king, other if k % 2 == 0 else king_mat)])),
                ("texture toggle", lambda k: hs.set_materials([(floor_mat, with_fields(M[floor_mat], textured=k % 2))])),
                ("light dimmed", lambda k: hs.set_materials([(light, with_fields(M[light], emission=(M[light]["emission"] * f32(0.25 + 0.1 * (k % 3))).astype(f32)))])),
                ("light off / on", lambda k: [hs.set_materials([(light, with_fields(M[light], emission=(0, 0, 0)))]), hs.set_materials([(light, M[light])])]),
                ("sky: a map", lambda k: hs.set_environment(sd.background, sky[:, :64 - k % 2])),
                ("sky: a colour", lambda k: hs.set_environment(sd.background + f32(0.01 * (k % 2)), None)),
                ("identity update", lambda k: hs.update([(king, ident)])),
            ]
            for name, call in rows:
                med, last = timed(call, args.repeats)
                say("%-18s %4d %9d %9.3f %9.3f %9.3f %9.3f %9.3f" % (name, last["path"], last["n_moved_tris"], med["total_ms"], med["transform_ms"], med["build_ms"], med["upload_ms"], med["wall_ms"]))
            hs.set_environment(sd.background, None)
            hs.close()
            walls = []
            for _ in range(4):
                t0 = time.perf_counter()
                h2 = hip.HipScene(sd, builder=builder)
                h2.close()
                walls.append((time.perf_counter() - t0) * 1e3)
            say("%-18s %4s %9s %9s %9s %9s %9s %9.3f   (no frame rendered: the first frame after it also allocates the workspace)"
                % ("destroy + create", "", "", "", "", "", "", float(np.median(walls[1:]))))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
