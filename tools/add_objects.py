"""Adding objects to a live scene: what mcpt_scene_add_objects costs beside the only route there was before it.  The command behind
profiles/scene_add.txt.
python tools/add_objects.py [--scenes chess,chess_high] [--builders ploc,lbvh,sah] [--repeats 5] [--out profiles/scene_add.txt]
Per scene and builder, in one warm process (the median of --repeats calls after one that warms up; every call gets a handle of its own,
created from the smaller description and warmed by one frame, since an added object cannot be taken out again):
  add one   a scene without the king gets the king: one mesh in one call
  add all   a scene of the board and the light gets every piece in one call
and, for both, the route of a library without the call, in the same process on the same device:
  destroy + create   mcpt_scene_destroy of the live scene, extend_scene on the host, mcpt_scene_create_ex of the extended description,
                     and the time by which the first frame of the new handle exceeds its second (the workspace allocation)
Columns: total_ms / transform_ms / build_ms / upload_ms of mcpt_update_info, and the wall time of the Python call (which includes the
wrapper's own extend_scene of its SceneData)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402

f32 = np.float32
KEYS = ("total_ms", "transform_ms", "build_ms", "upload_ms", "wall_ms")


def addition_of(sd, added):
    """(objects, triangles) that add the objects `added` of sd: their triangles packed in that order, first_tri relative to the packed array."""
    objs, tris, at = sd.objects[list(added)].copy(), [], 0
    for k, ob in enumerate(added):
        if sd.objects["kind"][ob] == 0:
            a, n = int(sd.objects["first_tri"][ob]), int(sd.objects["n_tri"][ob])
            tris.append(sd.triangles[a:a + n])
            objs["first_tri"][k] = at
            at += n
    return objs, (np.concatenate(tris) if tris else np.zeros(0, sd.triangles.dtype))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="chess,chess_high")
    ap.add_argument("--builders", default="ploc,lbvh,sah")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "scene_add.txt"))
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    pkg.build.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# python tools/add_objects.py --scenes %s --builders %s --repeats %d   (%s)" % (args.scenes, args.builders, args.repeats, hip.lib().mcpt_version().decode()))
    for scene in args.scenes.split(","):
        sd = scenes.chess_scene(width=96, height=54, spp=1) if scene == "chess" else scenes.chess_high(width=96, height=54, spp=1)
        M, O = sd.materials, sd.objects
        em = np.sqrt((M["emission"].astype(f32) ** 2).sum(-1)) > 1e-4
        pieces = [o for o in range(len(O)) if O["kind"][o] == 0 and not em[O["material"][o]] and not M["textured"][O["material"][o]]]
        king = max(pieces, key=lambda o: int(O["n_tri"][o]))
        for builder in args.builders.split(","):
            say("")
            say("%s, %s: %d triangles, %d objects; the king has %d triangles, the %d pieces %d" % (scene, builder, len(sd.triangles), len(O), int(O["n_tri"][king]), len(pieces), int(O["n_tri"][pieces].sum())))
            say("%-18s %4s %9s %9s %9s %9s %9s %9s" % ("edit", "path", "triangles", "total", "transform", "build", "upload", "wall"))
            for name, added in (("one", [king]), ("all", pieces)):
                mask = np.ones(len(O), bool)
                mask[added] = False
                base, _ = hip.compact_scene(sd, mask)
                objs, tris = addition_of(sd, added)
                rows = []
                for k in range(args.repeats + 1):
                    hs = hip.HipScene(base, builder=builder)
                    hs.render(spp=1, seed=1)  # the workspace exists: a warm handle
                    t0 = time.perf_counter()
                    _, info = hs.add_objects(objs, tris)
                    info["wall_ms"] = (time.perf_counter() - t0) * 1e3
                    hs.close()
                    if k > 0:
                        rows.append(info)
                med = {key: float(np.median([i[key] for i in rows])) for key in KEYS}
                say("%-18s %4d %9d %9.3f %9.3f %9.3f %9.3f %9.3f" % ("add " + name, rows[-1]["path"], rows[-1]["n_moved_tris"], med["total_ms"], med["transform_ms"], med["build_ms"], med["upload_ms"], med["wall_ms"]))
                # the route without the call: the live handle is destroyed and the extended description created, once per repetition
                parts = []
                for _ in range(args.repeats):
                    hs = hip.HipScene(base, builder=builder)
                    hs.render(spp=1, seed=1)
                    t0 = time.perf_counter()
                    hs.close()
                    t1 = time.perf_counter()
                    ext = hip.extend_scene(base, objs, tris)
                    t2 = time.perf_counter()
                    hs = hip.HipScene(ext, builder=builder)
                    t3 = time.perf_counter()
                    hs.render(spp=1, seed=1)
                    t4 = time.perf_counter()
                    hs.render(spp=1, seed=1)
                    t5 = time.perf_counter()
                    hs.close()
                    parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, max(0.0, ((t4 - t3) - (t5 - t4)) * 1e3)])
                d, c, n, w = np.median(np.array(parts), axis=0)
                say("%-18s destroy %.3f + extend %.3f + create %.3f + first frame's extra %.3f = %.3f ms (extra: min %.3f, max %.3f)"
                    % ("destroy+create " + name, d, c, n, w, d + c + n + w, np.array(parts)[:, 3].min(), np.array(parts)[:, 3].max()))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
