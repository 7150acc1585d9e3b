"""Run as a child process by tests/test_gpu_probe_relight.py: a probe volume baked into torch tensors on a non-default stream,
mcpt_probe_volume_relight issued on that stream right behind the bake and once more on its own output, with no host synchronisation in
between, outputs allocated by the call as torch tensors, and an edit of the scene enqueued behind the calls; compared with the numpy path
(buffers made without torch, the null stream) in the same process.  torch is imported BEFORE the library, bench.py's order.  Prints one
JSON line."""
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
import probe_relight_cases as prc  # noqa: E402
from deform_cases import SHORT, translate  # noqa: E402


def main():
    pkg = mcpt_loader.load()
    hip = pkg.hip_backend
    if not torch.cuda.is_available():
        print(json.dumps({"error": "torch sees no GPU"}))
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = pkg.scenes.cornell_demo(32, 24, 4)
    hs = hip.HipScene(sd, builder="sah", device=dev.index)
    grid = plc.scene_grid(sd)
    m = grid[2][0] * grid[2][1] * grid[2][2]
    md, nb = 170.0, 2.0
    kw = dict(spp=70, seed=5, hysteresis=0.75, direct_samples=3, direct_seed=2, indirect_only=True)
    # the numpy path: the null stream, buffers made without torch
    vol = plc.Volume(hs, grid, 64, 64, md, normal_bias=nb)
    want_sh, want_mom, want_cnt, _ = prc.relight(hs, vol, True, depth=True, max_distance=md, **kw)
    first = prc.HostVolume(grid, want_sh, want_mom, want_cnt, nb, vol.bm)
    want_chained = prc.relight(hs, first, True, **kw)[0]
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    move = translate(40, 0, -30)
    with torch.cuda.stream(side):
        cur = torch.cuda.current_stream(dev).cuda_stream
        on_side = cur == side.cuda_stream and cur != torch.cuda.default_stream(dev).cuda_stream
        sh, mom, cnt, _ = hs.bake_probe_volume(*grid, 64, md, depth_seed=3, spp=64, seed=2)  # stream: torch's current one, i.e. `side`
        sh1, mom1, cnt1, info = hs.relight_probe_volume(*grid, sh, mom, cnt, normal_bias=nb, depth=True, max_distance=md, **kw)
        sh2, none_m, none_c, _ = hs.relight_probe_volume(*grid, sh1, mom1, cnt1, normal_bias=nb, **kw)
        hs.update([(SHORT, move)])  # an edit behind the calls: it waits for the scene's query event
        sh3, _, _, _ = hs.relight_probe_volume(*grid, sh, mom, cnt, normal_bias=nb, **kw)
    side.synchronize()
    refused = overlap = False
    try:
        hs.relight_probe_volume(*grid, sh.t().contiguous().t(), **kw)  # transposed: not contiguous
    except ValueError:
        refused = True
    try:
        hs.relight_probe_volume(*grid, sh, out={"sh": sh}, **kw)
    except hip.McptError as e:
        overlap = "overlap" in str(e)
    # the moved scene through the numpy path
    want_moved = prc.relight(hs, vol, True, **kw)[0]
    print(json.dumps({"on_side_stream": bool(on_side),
                      "outputs_are_torch": bool(all(isinstance(t, torch.Tensor) and t.device == dev for t in (sh1, mom1, cnt1, sh2))
                                                and sh1.dtype == torch.float32 and tuple(sh1.shape) == (m, 27) and tuple(mom1.shape) == (m, 192)
                                                and cnt1.dtype == torch.int32 and tuple(cnt1.shape) == (m, 2) and none_m is None and none_c is None
                                                and info["launches"] >= 1),
                      "sh_differ": int((~pc.same_bits(sh1.cpu().numpy(), want_sh)).sum()),
                      "moments_differ": int((~pc.same_bits(mom1.cpu().numpy(), want_mom)).sum()),
                      "counts_differ": int((cnt1.cpu().numpy() != want_cnt).sum()),
                      "chained_differ": int((~pc.same_bits(sh2.cpu().numpy(), want_chained)).sum()),
                      "edit_behind_the_call": bool((sh3.cpu().numpy() != sh1.cpu().numpy()).any()),
                      "after_edit_differ": int((~pc.same_bits(sh3.cpu().numpy(), want_moved)).sum()),
                      "non_contiguous_refused": refused, "overlap_refused": overlap}))
    hs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
