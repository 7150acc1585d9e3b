"""Run as a child process by tests/test_gpu_probe_lit.py: a probe volume baked into torch tensors on a non-default stream and
mcpt_render_probe_lit issued on that stream right behind the bake, with no host synchronisation between the two, outputs allocated by the
call as torch tensors, compared with the numpy path (buffers made without torch, the null stream) in the same process.  torch is imported
BEFORE the library, bench.py's order.  Prints one JSON line."""
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
import probe_lit_cases as plc  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    W, H = 37, 23
    sd = pkg.scenes.cornell_demo(W, H, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    grid = plc.scene_grid(sd)
    vol = plc.Volume(hs, grid, 64, 64, 170.0, normal_bias=2.0)
    want_lit, want_pos, _ = plc.lit_frame(hs, vol, True, aov_spp=3, seed=5)
    want_plain, _, _ = plc.lit_frame(hs, vol, False, centre=True, position=False)
    want_chain, _, _ = plc.lit_frame(hs, vol, True, centre=True, specular_depth=2, position=False)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        sh, mom, cnt, _ = hs.bake_probe_volume(*grid, 64, 170.0, depth_seed=3, spp=64, seed=2)  # stream: torch's current one, i.e. `side`
        lit, pos, info = hs.render_probe_lit(*grid, sh, mom, cnt, normal_bias=2.0, aov_spp=3, seed=5, position=True)
        plain, none, _ = hs.render_probe_lit(*grid, sh, centre=True)
        chain, _, _ = hs.render_probe_lit(*grid, sh, mom, cnt, normal_bias=2.0, centre=True, specular_depth=2)
    side.synchronize()
    refused = False
    try:
        hs.render_probe_lit(*grid, sh.t().contiguous().t(), centre=True)  # transposed: not contiguous
    except ValueError:
        refused = True
    print(json.dumps({"on_side_stream": bool(on_side),
                      "outputs_are_torch": bool(isinstance(lit, torch.Tensor) and lit.dtype == torch.float32 and tuple(lit.shape) == (H, W, 3)
                                                and isinstance(pos, torch.Tensor) and tuple(pos.shape) == (H, W, 3) and lit.device == dev
                                                and none is None and info["samples"] == W * H * 3),
                      "lit_differ": int((~pc.same_bits(lit.cpu().numpy(), want_lit)).sum()),
                      "position_differ": int((~pc.same_bits(pos.cpu().numpy(), want_pos)).sum()),
                      "plain_differ": int((~pc.same_bits(plain.cpu().numpy(), want_plain)).sum()),
                      "chain_differ": int((~pc.same_bits(chain.cpu().numpy(), want_chain)).sum()),
                      "non_contiguous_refused": refused}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
