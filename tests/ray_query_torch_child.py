"""Run as a child process by tests/test_gpu_ray_query.py: rays produced by a torch kernel on a non-default stream, mcpt_query_closest and
mcpt_query_occluded enqueued on that stream with no host synchronisation between producer and query, outputs allocated by the call as
torch tensors.  torch is imported BEFORE the library, bench.py's order: torch carries its own HIP runtime, and the process must end up
with one.  Prints one JSON line."""
import torch  # noqa: I001  (first, on purpose)

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mcpt_loader  # noqa: E402
from deform_cases import cornell_rays  # noqa: E402
from ray_query_cases import expected_occluded, tmax_cycle  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    o, d = cornell_rays(hs, 64, 64, 4)
    # The producer: the rays are stored scaled and shifted, and un-done on the side stream, so that what the query reads exists only once
    # that stream's kernels have run.  Multiplications by 2 and 0.5 and additions of 0 are exact, so the rays are bit for bit (o, d).
    half_o, half_d = torch.from_numpy(o * np.float32(0.5)).to(dev), torch.from_numpy(d * np.float32(0.5)).to(dev)
    t_ref, p_ref = hs.intersect(o, d)
    tm = tmax_cycle(t_ref, p_ref)
    tm_dev = torch.from_numpy(tm).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    infos = []
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        for _ in range(2):  # the second round must not allocate
            to = half_o * 2.0
            td = half_d * 2.0
            tt = tm_dev + 0.0
            res, info = hs.query_closest(to, td)  # stream: torch's current one, i.e. `side`
            occ, _ = hs.query_occluded(to, td, tt)
            fil, _ = hs.query_closest(to, td, tt, want=("prim",))
            infos.append(info)
    side.synchronize()
    t_got, p_got = res["t"].cpu().numpy(), res["prim"].cpu().numpy()
    want_occ = expected_occluded(t_ref, p_ref, tm)
    refused = False
    try:
        hs.query_closest(to.t().contiguous().t(), td)  # transposed: not contiguous
    except ValueError:
        refused = True
    print(json.dumps({"n": int(len(o)), "hit_fraction": float((p_ref >= 0).mean()), "prim_differ": int((p_got != p_ref).sum()),
                      "t_differ": int((t_got.view(np.uint64) != t_ref.view(np.uint64)).sum()),
                      "occluded_differ": int((occ.cpu().numpy() != want_occ).sum()),
                      "filtered_differ": int(((fil["prim"].cpu().numpy() >= 0) != (want_occ == 1)).sum()),
                      "outputs_are_torch": bool(isinstance(res["t"], torch.Tensor) and res["t"].dtype == torch.float64 and res["prim"].dtype == torch.int32
                                                and occ.dtype == torch.uint8 and res["t"].device == dev),
                      "on_side_stream": bool(on_side), "non_contiguous_refused": refused, "grew": [int(i["grew"]) for i in infos]}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
