"""The denoiser against plain rendering, on the chess frame (1920x1080, constant sky: sky cull on) and the Cornell box (384x384): wall time
of render against render_denoised at a few sample counts (the variance and the AOVs left on the device, so both calls copy the same
frames back), with the render / AOV / filter times of mcpt_denoise_info, and the tone-mapped RMSE of the noisy and of the denoised frame
against a plain frame of 8192 spp and another seed.  Equal time: a plain render at the sample count whose wall time matches the denoised
call's (scaled from the measured times, then measured itself).  --specular-depths: one denoised row per depth of the feature samples' mirror /
glass chains (mcpt_denoise_opts.specular_depth; 0: first-hit features).
python tools/denoise.py [--out FILE] [--spps 64,256,2048] [--ref-spp 8192] [--scenes chess,cornell] [--specular-depths 0,4]"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402


def tone(fb):
    return np.power(np.clip(np.nan_to_num(fb.astype(np.float64), nan=1.0), 0.0, 1.0), 0.45)


def rmse(a, b):
    return float(np.sqrt(np.mean((tone(a) - tone(b)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--spps", default="64,256,2048")
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--scenes", default="chess,cornell")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--specular-depths", default="0")
    a = ap.parse_args()
    pkg = mcpt_loader.load()
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for scene in a.scenes.split(","):
        sd = pkg.scenes.chess_scene(width=a.width, height=a.height, spp=64) if scene == "chess" else pkg.scenes.cornell_demo(384, 384, 64)
        hs = pkg.HipScene(sd, device=0)
        hs.render(spp=64, seed=5)  # (warm-up: allocations)
        depths = [int(x) for x in a.specular_depths.split(",")]
        for depth in depths:
            hs.render_denoised(spp=64, seed=5, specular_depth=depth)
        t = time.perf_counter()
        ref, _ = hs.render(spp=a.ref_spp, seed=12345)
        say("%s: reference %d spp (seed 12345) %.2f s" % (scene, a.ref_spp, time.perf_counter() - t))
        for spp in [int(x) for x in a.spps.split(",")]:
            for depth in depths:
                tp, td = [], []
                for _ in range(3):  # (median of three: a single call of a few tens of ms is noisy)
                    t = time.perf_counter()
                    fb, st = hs.render(spp=spp, seed=1)
                    tp.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    r = hs.render_denoised(spp=spp, seed=1, features=False, specular_depth=depth)
                    td.append(time.perf_counter() - t)
                tp, td = float(np.median(tp)), float(np.median(td))
                assert np.array_equal(r["fb"], fb, equal_nan=True)
                spp_eq = max(spp, int(round(spp * td / tp)))
                te = []
                for _ in range(3):
                    t = time.perf_counter()
                    fe, _ = hs.render(spp=spp_eq, seed=1)
                    te.append(time.perf_counter() - t)
                te = float(np.median(te))
                inf = r["info"]
                row = dict(scene=scene, spp=spp, specular_depth=depth, s_render=tp, s_render_denoised=td, ms_render=inf["ms_render"],
                           ms_aov=inf["ms_aov"], ms_denoise=inf["ms_denoise"], rmse_noisy=rmse(fb, ref), rmse_denoised=rmse(r["denoised"], ref),
                           spp_equal_time=spp_eq, s_equal_time=te, rmse_equal_time=rmse(fe, ref))
                rows.append(row)
                say("  %5d spp depth %d: render %7.3f s | render_denoised %7.3f s (render %.1f ms, AOVs %.2f ms, filter %.2f ms) | RMSE noisy %.5f"
                    " denoised %.5f | equal time: plain %d spp %7.3f s RMSE %.5f"
                    % (spp, depth, tp, td, inf["ms_render"], inf["ms_aov"], inf["ms_denoise"], row["rmse_noisy"], row["rmse_denoised"], spp_eq, te,
                       row["rmse_equal_time"]))
        hs.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(a.out.rsplit(".", 1)[0] + ".json", "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
