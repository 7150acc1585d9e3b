"""Run as a child process by tests/test_gpu_direct.py: points produced by a torch kernel on a non-default stream, mcpt_query_direct
issued on that stream with no host synchronisation between producer and call, the output allocated by the call as a torch tensor,
compared with the numpy path (buffers made without torch, the null stream) in the same process.  torch is imported BEFORE the library,
bench.py's order.  Prints one JSON line."""
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
from ray_query_cases import DevBuf  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    p = pc.probe_points(sd, 193)
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=(len(p), 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    N, seed, ks = 5, 4, 7
    want = pdc.Guarded((len(p), 3))
    hs.query_direct(DevBuf(p), DevBuf(nrm), N, seed=seed, key_sample=ks, out=want)
    want = want.get()
    half = torch.from_numpy(p * np.float32(0.5)).to(dev)  # stored halved and doubled on the side stream (exact)
    tn = torch.from_numpy(nrm).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        tp = half * 2.0
        got, info = hs.query_direct(tp, tn, N, seed=seed, key_sample=ks)  # stream: torch's current one, i.e. `side`
        again, info2 = hs.query_direct(tp, tn, N, seed=seed, key_sample=ks)
    side.synchronize()
    refused = False
    try:
        hs.query_direct(tp.t().contiguous().t(), tn, N)  # transposed: not contiguous
    except ValueError:
        refused = True
    print(json.dumps({"n": int(len(p)), "on_side_stream": bool(on_side), "nonzero": int((want > 0).any(axis=1).sum()),
                      "outputs_are_torch": bool(isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (len(p), 3)
                                                and got.device == dev and "grew" in info),
                      "differ": int((~pc.same_bits(got.cpu().numpy(), want)).sum()), "again_differ": int((~pc.same_bits(again.cpu().numpy(), want)).sum()),
                      "grew_again": int(info2["grew"]), "non_contiguous_refused": refused}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
