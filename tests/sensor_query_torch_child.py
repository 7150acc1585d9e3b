"""Run as a child process by tests/test_gpu_sensor_query.py: sensors produced by a torch kernel on a non-default stream, mcpt_query_radiance
issued on that stream with no host synchronisation between producer and query, outputs allocated by the call as torch tensors, compared
with the numpy path (buffers made without torch, the null stream) in the same process.  torch is imported BEFORE the library, bench.py's
order: torch carries its own HIP runtime, and the process must end up with one.  Prints one JSON line."""
import torch  # noqa: I001  (first, on purpose)

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mcpt_loader  # noqa: E402
from sensor_query_cases import radiance, rays_805, same_bits, surface_sensors  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    o, d = rays_805(hs, sd)
    p, nrm = surface_sensors(hs, sd)
    kw = dict(spp=8, seed=4, spp_per_pass=4)
    want_ray, want_var, _ = radiance(hs, o, d, variance=True, **kw)
    want_hemi, _, _ = radiance(hs, p, nrm, kind="hemisphere", **kw)
    # The producer: the sensors are stored halved and doubled on the side stream (exact), so what the query reads exists only once that
    # stream's kernels have run.
    half = [torch.from_numpy(a * np.float32(0.5)).to(dev) for a in (o, d, p, nrm)]
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        to, td, tp, tn = (h * 2.0 for h in half)
        rad, var, st = hs.query_radiance(to, td, variance=True, **kw)  # stream: torch's current one, i.e. `side`
        hemi, none, _ = hs.query_radiance(tp, tn, kind="hemisphere", **kw)
    side.synchronize()
    refused = False
    try:
        hs.query_radiance(to.t().contiguous().t(), td, **kw)  # transposed: not contiguous
    except ValueError:
        refused = True
    print(json.dumps({"n": int(len(o)), "on_side_stream": bool(on_side),
                      "outputs_are_torch": bool(isinstance(rad, torch.Tensor) and rad.dtype == torch.float32 and tuple(rad.shape) == (len(o), 3)
                                                and isinstance(var, torch.Tensor) and none is None and rad.device == dev and st.samples == len(o) * 8),
                      "ray_differ": int((~same_bits(rad.cpu().numpy(), want_ray)).sum()),
                      "variance_differ": int((~same_bits(var.cpu().numpy(), want_var)).sum()),
                      "hemisphere_differ": int((~same_bits(hemi.cpu().numpy(), want_hemi)).sum()),
                      "non_contiguous_refused": refused}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
