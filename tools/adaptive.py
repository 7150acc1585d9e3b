"""Adaptive sampling against uniform sampling on the chess frame (1920x1080): uniform 2048 spp against mcpt_render_adaptive with S0 = 64,
maximum 2048, at a few thresholds; with the constant sky (sky cull on) and with a synthetic 2048x1024 lat-long map (no cull).  Reports wall
time, total samples and the tone-mapped RMSE against a uniform 8192-spp frame of another seed.
python tools/adaptive.py [--out FILE] [--thresholds 0.02,0.05,0.1] [--width W --height H]"""
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


def env_map(w=2048, h=1024):
    """A smooth synthetic sky: a horizon gradient, a bright sun-like lobe and some coloured bands, values in [0, 1]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    th, ph = np.pi * (y + 0.5) / h, 2 * np.pi * (x + 0.5) / w
    sky = np.stack([0.35 + 0.25 * np.cos(th), 0.45 + 0.25 * np.cos(th), 0.7 + 0.25 * np.cos(th)], -1)
    sun = np.exp(-((th - 0.6) ** 2 + (ph - 2.0) ** 2) / 0.01)[..., None] * np.float32([0.6, 0.5, 0.3])
    bands = 0.08 * np.sin(6 * ph)[..., None] * np.float32([1.0, 0.6, 0.2])
    return np.clip(sky + sun + bands, 0, 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--thresholds", default="0.02,0.05,0.1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=2048)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=8192)
    a = ap.parse_args()
    pkg = mcpt_loader.load()
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    W, H = a.width, a.height
    for sky in ("constant", "envmap"):
        sd = pkg.scenes.chess_scene(width=W, height=H, spp=a.spp)
        if sky == "envmap":
            sd.env_pixels = env_map()
        hs = pkg.HipScene(sd, device=0)
        hs.render(spp=a.min_spp, seed=5)  # (warm-up: allocations)
        t = time.perf_counter()
        ref, _ = hs.render(spp=a.ref_spp, seed=12345)
        say("%s sky: reference %d spp (seed 12345) %.2f s" % (sky, a.ref_spp, time.perf_counter() - t))
        t = time.perf_counter()
        uni, su = hs.render(spp=a.spp, seed=1)
        tu = time.perf_counter() - t
        ru = rmse(uni, ref)
        say("  uniform  %4d spp: %8.3f s  %7.3f Gsamples  RMSE %.5f" % (a.spp, tu, su.samples / 1e9, ru))
        rows.append(dict(sky=sky, mode="uniform", spp=a.spp, s=tu, samples=su.samples, rmse=ru))
        for k in (a.min_spp, 4 * a.min_spp):  # uniform frames at lower counts: the RMSE-against-samples curve adaptive is compared with
            t = time.perf_counter()
            f, s = hs.render(spp=k, seed=1)
            tk = time.perf_counter() - t
            rows.append(dict(sky=sky, mode="uniform", spp=k, s=tk, samples=s.samples, rmse=rmse(f, ref)))
            say("  uniform  %4d spp: %8.3f s  %7.3f Gsamples  RMSE %.5f" % (k, tk, s.samples / 1e9, rows[-1]["rmse"]))
        for thr in [float(x) for x in a.thresholds.split(",")]:
            t = time.perf_counter()
            fb, spp, err, info, st = hs.render_adaptive(a.min_spp, thr, spp=a.spp, seed=1)
            ta = time.perf_counter() - t
            ra = rmse(fb, ref)
            rows.append(dict(sky=sky, mode="adaptive", threshold=thr, s=ta, samples=st.samples, rmse=ra, rounds=info["rounds"],
                             active_pixels=info["active_pixels"], ms_round=[round(x, 2) for x in info["ms_round"]]))
            say("  adaptive thr %.3f: %8.3f s  %7.3f Gsamples (%.0f spp on average)  RMSE %.5f  rounds %d, active %s, ms/round %s"
                % (thr, ta, st.samples / 1e9, st.samples / (W * H), ra, info["rounds"], info["active_pixels"],
                   [round(x, 1) for x in info["ms_round"]]))
        hs.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(a.out.rsplit(".", 1)[0] + ".json", "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
