"""Run as a child process by tests/test_gpu_probes.py: probe points produced by a torch kernel on a non-default stream, mcpt_query_probes,
mcpt_probe_shade and mcpt_bake_probe_grid issued on that stream with no host synchronisation between producer and call, outputs allocated
by the calls as torch tensors, compared with the numpy path (buffers made without torch, the null stream) in the same process.  torch is
imported BEFORE the library, bench.py's order.  Prints one JSON line."""
import torch  # noqa: I001  (first, on purpose)

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mcpt_loader  # noqa: E402
import probe_cases as pc  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    p = pc.probe_points(sd)
    kw = dict(spp=8, seed=4, spp_per_pass=4)
    want_sh, want_rad, _, _ = pc.probes(hs, p, **kw)
    grid = ((60.0, 60.0, 60.0), (110.0, 140.0, 90.0), (5, 4, 5))
    pts = hip.probe_grid_points(*grid)
    want_bake, _, _, _ = pc.probes(hs, pts, radiance=False, **kw)
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=(805, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    want_shade = hip.probe_shade(*grid, want_bake, p, nrm)
    half = torch.from_numpy(p * np.float32(0.5)).to(dev)  # stored halved and doubled on the side stream (exact)
    tn = torch.from_numpy(nrm).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        tp = half * 2.0
        sh, rad, none, st = hs.query_probes(tp, radiance=True, **kw)  # stream: torch's current one, i.e. `side`
        baked, _ = hs.bake_probe_grid(*grid, **kw)
        shaded = hs.probe_shade(*grid, baked, tp, tn)
    side.synchronize()
    refused = False
    try:
        hs.query_probes(tp.t().contiguous().t(), **kw)  # transposed: not contiguous
    except ValueError:
        refused = True
    print(json.dumps({"n": int(len(p)), "on_side_stream": bool(on_side),
                      "outputs_are_torch": bool(isinstance(sh, torch.Tensor) and sh.dtype == torch.float32 and tuple(sh.shape) == (len(p), 27)
                                                and isinstance(rad, torch.Tensor) and none is None and sh.device == dev and st.samples == len(p) * 8
                                                and isinstance(shaded, torch.Tensor) and tuple(baked.shape) == (100, 27)),
                      "sh_differ": int((~pc.same_bits(sh.cpu().numpy(), want_sh)).sum()),
                      "radiance_differ": int((~pc.same_bits(rad.cpu().numpy(), want_rad)).sum()),
                      "bake_differ": int((~pc.same_bits(baked.cpu().numpy(), want_bake)).sum()),
                      "shade_differ": int((~pc.same_bits(shaded.cpu().numpy(), want_shade)).sum()),
                      "non_contiguous_refused": refused}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
