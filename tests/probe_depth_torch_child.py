"""Run as a child process by tests/test_gpu_probe_depth.py: probe points produced by a torch kernel on a non-default stream,
mcpt_query_probe_depth, mcpt_bake_probe_volume and mcpt_probe_shade_visible issued on that stream with no host synchronisation between
producer and call, outputs allocated by the calls as torch tensors, compared with the numpy path (buffers made without torch, the null
stream) in the same process.  torch is imported BEFORE the library, bench.py's order.  Prints one JSON line."""
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
import probe_depth_cases as pdc  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    p = pc.probe_points(sd, 65)
    spp, md, seed = 70, 170.0, 4
    want_m, want_c, _ = pdc.depth(hs, p, spp, md, seed=seed)
    grid = ((60.0, 60.0, 60.0), (110.0, 140.0, 90.0), (5, 4, 5))
    pts = hip.probe_grid_points(*grid)
    kw = dict(spp=4, seed=4)
    want_sh, _, _, _ = pc.probes(hs, pts, radiance=False, **kw)
    want_vm, want_vc, _ = pdc.depth(hs, pts, spp, md, seed=seed)
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=(65, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    want_shade = hip.probe_shade_visible(*grid, want_sh, want_vm, want_vc, p, nrm, normal_bias=2.0, backface_max=0.25)
    half = torch.from_numpy(p * np.float32(0.5)).to(dev)  # stored halved and doubled on the side stream (exact)
    tn = torch.from_numpy(nrm).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        tp = half * 2.0
        mom, cnt, info = hs.query_probe_depth(tp, spp, md, seed=seed)  # stream: torch's current one, i.e. `side`
        vsh, vmom, vcnt, st = hs.bake_probe_volume(*grid, spp, md, depth_seed=seed, **kw)
        shaded = hs.probe_shade_visible(*grid, vsh, vmom, vcnt, tp, tn, normal_bias=2.0, backface_max=0.25)
    side.synchronize()
    refused = False
    try:
        hs.query_probe_depth(tp.t().contiguous().t(), spp, md)  # transposed: not contiguous
    except ValueError:
        refused = True
    print(json.dumps({"n": int(len(p)), "on_side_stream": bool(on_side),
                      "outputs_are_torch": bool(isinstance(mom, torch.Tensor) and mom.dtype == torch.float32 and tuple(mom.shape) == (65, 192)
                                                and isinstance(cnt, torch.Tensor) and cnt.dtype == torch.int32 and tuple(cnt.shape) == (65, 2)
                                                and mom.device == dev and isinstance(shaded, torch.Tensor) and tuple(vmom.shape) == (100, 192)
                                                and st.samples == 100 * 4 and "grew" in info),
                      "moments_differ": int((~pc.same_bits(mom.cpu().numpy(), want_m)).sum()),
                      "counts_differ": int((cnt.cpu().numpy() != want_c).sum()),
                      "volume_differ": int((~pc.same_bits(vsh.cpu().numpy(), want_sh)).sum() + (~pc.same_bits(vmom.cpu().numpy(), want_vm)).sum()
                                           + (vcnt.cpu().numpy() != want_vc).sum()),
                      "shade_differ": int((~pc.same_bits(shaded.cpu().numpy(), want_shade)).sum()),
                      "non_contiguous_refused": refused}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
