"""Run as a child process by tests/test_gpu_lightmap.py: the values of a scatter produced by a torch kernel on a non-default stream and
scattered on that stream with no host synchronisation in between; texel sensors and a whole bake whose outputs the calls allocate as torch
tensors on that stream; all compared with the host function, the numpy dilation and the numpy path (buffers made without torch, the null
stream) in the same process.  torch is imported BEFORE the library, bench.py's order: torch carries its own HIP runtime, and the process
must end up with one.  Prints one JSON line."""
import torch  # noqa: I001  (first, on purpose)

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mcpt_loader  # noqa: E402
import lightmap_cases as lc  # noqa: E402
from ray_query_cases import DevBuf  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = lc.cornell_charted(pkg)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    W, H, ob, dilate = 24, 16, 0, 3
    kw = dict(spp=8, seed=6, spp_per_pass=4)
    want = hip.lightmap_texels(sd, ob, W, H)
    n = len(want["texel"])
    v = np.random.default_rng(4).uniform(0, 3, size=(n, 3)).astype(np.float32)
    want_img, want_cov = lc.model_dilate(W, H, want["texel"], v, dilate)
    # the numpy path of the bake: device buffers made without torch, the null stream
    out = {"image": DevBuf(shape=(H, W, 3), dtype=np.float32), "coverage": DevBuf(shape=(H, W), dtype=np.uint8), "variance": DevBuf(shape=(H, W, 3), dtype=np.float32)}
    hs.bake_lightmap(ob, W, H, dilate=dilate, variance=True, out=out, **kw)
    ref = [out[k].get() for k in ("image", "coverage", "variance")]
    # The producer: the values are stored halved and doubled on the side stream (exact), so what the scatter reads exists only once that
    # stream's kernels have run.
    half = torch.from_numpy(v * np.float32(0.5)).to(dev)
    texel = torch.from_numpy(want["texel"]).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        values = half * 2.0
        img, cov = hs.lightmap_scatter(ob, W, H, texel, values, dilate=dilate)  # stream: torch's current one, i.e. `side`
        tex, n_dev = hs.lightmap_texels(ob, W, H)
        bimg, bcov, bvar, info, st = hs.bake_lightmap(ob, W, H, dilate=dilate, variance=True, **kw)
        simg, scov = hs.lightmap_scatter(ob, W, H, want["texel"], v, dilate=dilate)  # numpy inputs: staged
    side.synchronize()
    refused = False
    try:
        hs.lightmap_scatter(ob, W, H, texel, values.t().contiguous().t(), dilate=dilate)  # transposed: not contiguous
    except ValueError:
        refused = True
    tensors = [img, cov, bimg, bcov, bvar, simg, scov] + list(tex.values())
    print(json.dumps({"n": int(n), "on_side_stream": bool(on_side),
                      "outputs_are_torch": bool(all(isinstance(t, torch.Tensor) and t.device == dev for t in tensors) and tuple(img.shape) == (H, W, 3)
                                                and cov.dtype == torch.uint8 and tuple(cov.shape) == (H, W) and n_dev == n and info["n_texels"] == n
                                                and all(len(t) == n for t in tex.values()) and st.samples == n * 8),
                      "texels_differ": int(sum(not lc.same_bits(tex[w].cpu().numpy(), want[w]) for w in lc.NAMES)),
                      "scatter_differ": int(not lc.same_bits(img.cpu().numpy(), want_img)) + int(not lc.same_bits(cov.cpu().numpy(), want_cov)),
                      "staged_scatter_differ": int(not lc.same_bits(simg.cpu().numpy(), want_img)) + int(not lc.same_bits(scov.cpu().numpy(), want_cov)),
                      "bake_differ": int(sum(not lc.same_bits(t.cpu().numpy(), r) for t, r in zip((bimg, bcov, bvar), ref))),
                      "non_contiguous_refused": refused}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
