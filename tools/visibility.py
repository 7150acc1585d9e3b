"""Hiding and showing objects in a live scene: what mcpt_scene_set_visibility costs beside the only route there was before it.  The
command behind profiles/scene_visibility.txt.
python tools/visibility.py [--scenes chess,chess_high] [--builders ploc,lbvh,sah] [--repeats 5] [--out profiles/scene_visibility.txt]
Per scene and builder it times, in one warm process on one scene handle (the median of --repeats pairs after one pair that warms up):
  hide one / show one   the king hidden, then shown again: one call each
  hide all / show all   every piece (every mesh but the light and the board) hidden in one call, then shown in one call
  identity update       mcpt_scene_update of the king with the transform it already has (the yardstick: what moving the same object costs)
and, for both masks, the route of a library without the call, in the same process on the same device:
  destroy + create      mcpt_scene_destroy of the live scene, compact_scene on the host, mcpt_scene_create_ex of the compacted description,
                        and the time by which the first frame of the new handle exceeds its second (the workspace allocation)
Columns: total_ms / transform_ms / build_ms / upload_ms of mcpt_update_info, and the wall time of the Python call."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402

f32 = np.float32
KEYS = ("total_ms", "transform_ms", "build_ms", "upload_ms", "wall_ms")


def timed_pairs(first, second, repeats):
    """Medians of `first` and of `second`, called alternately; the first pair warms up."""
    rows = ([], [])
    for k in range(repeats + 1):
        for which, call in enumerate((first, second)):
            t0 = time.perf_counter()
            info = dict(call())
            info["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if k > 0:
                rows[which].append(info)
    return [({key: float(np.median([i[key] for i in r])) for key in KEYS}, r[-1]) for r in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="chess,chess_high")
    ap.add_argument("--builders", default="ploc,lbvh,sah")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "scene_visibility.txt"))
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    pkg.build.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# python tools/visibility.py --scenes %s --builders %s --repeats %d   (%s)" % (args.scenes, args.builders, args.repeats, hip.lib().mcpt_version().decode()))
    for scene in args.scenes.split(","):
        sd = scenes.chess_scene(width=96, height=54, spp=1) if scene == "chess" else scenes.chess_high(width=96, height=54, spp=1)
        M, O = sd.materials, sd.objects
        em = np.sqrt((M["emission"].astype(f32) ** 2).sum(-1)) > 1e-4
        pieces = [o for o in range(len(O)) if O["kind"][o] == 0 and not em[O["material"][o]] and not M["textured"][O["material"][o]]]
        king = max(pieces, key=lambda o: int(O["n_tri"][o]))
        ident = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
        for builder in args.builders.split(","):
            hs = hip.HipScene(sd, builder=builder)
            hs.render(spp=1, seed=1)  # the workspace exists: a warm handle
            say("")
            say("%s, %s: %d triangles, %d objects; the king has %d triangles, the %d pieces %d" % (scene, builder, len(sd.triangles), len(O), int(O["n_tri"][king]), len(pieces), int(O["n_tri"][pieces].sum())))
            say("%-18s %4s %9s %9s %9s %9s %9s %9s" % ("edit", "path", "triangles", "total", "transform", "build", "upload", "wall"))
            for name, objs in (("one", [king]), ("all", pieces)):
                pair = timed_pairs(lambda: hs.set_visibility([(o, False) for o in objs]), lambda: hs.set_visibility([(o, True) for o in objs]), args.repeats)
                for verb, (med, last) in zip(("hide", "show"), pair):
                    say("%-18s %4d %9d %9.3f %9.3f %9.3f %9.3f %9.3f" % (verb + " " + name, last["path"], last["n_moved_tris"], med["total_ms"], med["transform_ms"], med["build_ms"], med["upload_ms"], med["wall_ms"]))
            (med, last), _ = timed_pairs(lambda: hs.update([(king, ident)]), lambda: hs.update([(king, ident)]), args.repeats)
            say("%-18s %4d %9d %9.3f %9.3f %9.3f %9.3f %9.3f" % ("identity update", last["path"], last["n_moved_tris"], med["total_ms"], med["transform_ms"], med["build_ms"], med["upload_ms"], med["wall_ms"]))
            # the route without the call: the live handle is destroyed and the compacted description created, once per repetition
            for name, objs in (("one", [king]), ("all", pieces)):
                mask = np.ones(len(O), bool)
                mask[objs] = False
                parts = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    hs.close()
                    t1 = time.perf_counter()
                    csd, _ = hip.compact_scene(sd, mask)
                    t2 = time.perf_counter()
                    hs = hip.HipScene(csd, builder=builder)
                    t3 = time.perf_counter()
                    hs.render(spp=1, seed=1)
                    t4 = time.perf_counter()
                    hs.render(spp=1, seed=1)
                    t5 = time.perf_counter()
                    parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, max(0.0, ((t4 - t3) - (t5 - t4)) * 1e3)])
                d, c, n, w = np.median(np.array(parts), axis=0)
                say("%-18s destroy %.3f + compact %.3f + create %.3f + first frame's extra %.3f = %.3f ms (extra: min %.3f, max %.3f)"
                    % ("destroy+create " + name, d, c, n, w, d + c + n + w, np.array(parts)[:, 3].min(), np.array(parts)[:, 3].max()))
            hs.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
