"""A sine wave through the vertices of chess pieces: mcpt_scene_deform with positions from numpy (host pointer) and, when torch sees a GPU,
from a torch tensor on the scene's device (device pointer), under PLOC and LBVH.  The command behind profiles/scene_deform.txt.
python tools/deform.py [--scene chess|chess_high] [--objects one|all] [--frames 5] [--width 640] [--height 360] [--spp 2]
Per builder and input kind it runs --frames frames of a sequence, `scene.deform(...); seq.frame(seed=k)`, and prints the median
mcpt_update_info of the calls after the first (which warms up): total, transform, build, upload in ms, and the wall time of the Python
call.  It then prints the same for mcpt_scene_update of the same objects, and the parent's only alternative for new vertices: destroy +
create.  --no-frames skips the sequence (the calls alone).  Under `rocprofv3 --kernel-trace --stats -- python tools/deform.py` the
statistics list k_deform_objects beside k_move_objects of the same run.
torch, when present, is imported before the library: it carries its own HIP runtime and the process must end up with one."""
import argparse
import sys
import time

import numpy as np

try:
    import torch
except Exception:  # noqa: BLE001 -- the tool runs without torch, host pointers only
    torch = None

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402

f32 = np.float32


def positions(sd, o):
    a, n = int(sd.objects["first_tri"][o]), int(sd.objects["n_tri"][o])
    t = sd.triangles[a:a + n]
    return np.ascontiguousarray(np.stack([t["v0"], t["v1"], t["v2"]], axis=1), dtype=f32)


def wave(P, k, amp):
    """Frame k of the wave: every vertex moves sideways by a sine of its height."""
    out = P.copy()
    out[..., 0] += f32(amp) * np.sin(0.05 * P[..., 1] + 0.7 * k).astype(f32)
    return out


def median_info(infos):
    keys = ("total_ms", "transform_ms", "build_ms", "upload_ms", "wall_ms")
    return {k: float(np.median([i[k] for i in infos])) for k in keys}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="chess", choices=["chess", "chess_high"])
    ap.add_argument("--objects", default="one", choices=["one", "all"])
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--no-create", action="store_true", help="skip the destroy + create comparison")
    args = ap.parse_args()
    pkg = mcpt_loader.load()
    hip, scenes = pkg.hip_backend, pkg.scenes
    pkg.build.build()
    sd = scenes.chess_scene(width=args.width, height=args.height, spp=args.spp) if args.scene == "chess" else scenes.chess_high(width=args.width, height=args.height, spp=args.spp)
    emits = np.abs(sd.materials["emission"]).sum(-1) > 0 if "emission" in sd.materials.dtype.names else np.zeros(len(sd.materials), bool)
    meshes = [o for o in range(len(sd.objects)) if sd.objects["kind"][o] == 0 and sd.objects["n_tri"][o] > 0 and not emits[sd.objects["material"][o]]]
    big = max(meshes, key=lambda o: int(sd.objects["n_tri"][o]))
    objs = [big] if args.objects == "one" else meshes
    base = {o: positions(sd, o) for o in objs}
    n_tris = sum(len(p) for p in base.values())
    amp = 0.02 * float(np.ptp(sd.triangles["v0"][:, 0]))
    use_torch = torch is not None and torch.cuda.is_available()
    print("%s: %d triangles in %d objects; deforming %d object(s), %d triangles; torch device tensors: %s"
          % (args.scene, len(sd.triangles), len(sd.objects), len(objs), n_tris, "yes" if use_torch else "no"))
    print("%-6s %-8s %9s %9s %9s %9s %9s" % ("tree", "input", "total", "transform", "build", "upload", "wall"))
    for builder in ("ploc", "lbvh"):
        hs = hip.HipScene(sd, builder=builder)
        seq = None if args.no_frames else hs.sequence(filter=True, aov_spp=1)
        kinds = ["host"] + (["device"] if use_torch else [])
        k = 0
        for kind in kinds + ["update"]:
            infos = []
            for _ in range(args.frames):
                k += 1
                if kind == "update":
                    m = np.array([[1, 0, 0, amp * np.sin(0.7 * k)], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
                    t0 = time.perf_counter()
                    info = hs.update([(o, m) for o in objs])
                else:
                    new = {o: wave(p, k, amp) for o, p in base.items()}
                    if kind == "device":
                        dev = torch.device("cuda", torch.cuda.current_device())
                        new = {o: torch.from_numpy(p).to(dev) for o, p in new.items()}
                        torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    info = hs.deform(list(new.items()))
                info["wall_ms"] = (time.perf_counter() - t0) * 1e3
                assert info["path"] == 1 and info["n_moved_tris"] == n_tris
                infos.append(info)
                if seq is not None:
                    seq.frame(want=("rgba",), spp=args.spp, seed=k)
            m = median_info(infos[1:] if len(infos) > 1 else infos)
            print("%-6s %-8s %9.3f %9.3f %9.3f %9.3f %9.3f" % (builder, kind, m["total_ms"], m["transform_ms"], m["build_ms"], m["upload_ms"], m["wall_ms"]))
        if seq is not None:
            seq.close()
        hs.close()
        if not args.no_create:
            walls = []
            for _ in range(max(2, min(args.frames, 4))):
                t0 = time.perf_counter()
                h2 = hip.HipScene(sd, builder=builder)
                walls.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                h2.close()
                walls[-1] += (time.perf_counter() - t0) * 1e3
            print("%-6s %-8s %9s %9s %9s %9s %9.3f   (destroy + create, no frame rendered: the first frame also allocates the workspace)"
                  % (builder, "create", "", "", "", "", float(np.median(walls[1:]))))


if __name__ == "__main__":
    main()
