"""Run as a child process by tests/test_gpu_scene_deform.py: the same deformation given to two scenes, once as a numpy array and once as a
torch tensor on the scene's device.  torch is imported BEFORE the library, bench.py's order: torch carries its own HIP runtime, and the
process must end up with one.  Prints one JSON line per builder."""
import torch  # noqa: I001  (first, on purpose)

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mcpt_loader  # noqa: E402
from deform_cases import SHORT, TALL, cornell_rays, object_positions, same_bits, wave  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    P, Q = wave(object_positions(sd, SHORT)), wave(object_positions(sd, TALL), phase=1.0)
    for builder in ("ploc", "lbvh"):
        a, b = hip.HipScene(sd, builder=builder, device=dev.index), hip.HipScene(sd, builder=builder, device=dev.index)
        ia = a.deform([(SHORT, P), (TALL, Q)])
        tp = torch.from_numpy(P).to(dev)
        tq = torch.from_numpy(Q.reshape(-1)).to(dev)  # the flat shape
        torch.cuda.synchronize(dev)  # the producer stream is done before the call
        ib = b.deform([(SHORT, tp), (TALL, tq)])
        refused = False
        try:
            b.deform([(SHORT, tp.transpose(1, 2))])  # not contiguous
        except ValueError:
            refused = True
        o, d = cornell_rays(a, 64, 64, 4)
        ta, pa = a.intersect(o, d)
        tb, pb = b.intersect(o, d)
        fa, fb = a.render(spp=4, seed=5)[0], b.render(spp=4, seed=5)[0]
        print(json.dumps({"builder": builder, "path_host": ia["path"], "path_device": ib["path"], "n_moved_tris": [ia["n_moved_tris"], ib["n_moved_tris"]],
                          "prim_differ": int((pa != pb).sum()), "t_differ": int((ta.view(np.uint64) != tb.view(np.uint64)).sum()),
                          "hit_fraction": float((pa >= 0).mean()), "frame_differ": int((~same_bits(fa, fb)).sum()),
                          "non_contiguous_refused": refused}))
        a.close()
        b.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
