"""One 1920x1080 chess frame through the pieces of temporal reuse, beside what they are compared with: the AOV pass (the same rays as the
motion pass) and the a-trous filter.  Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/temporal.py`
for the kernel times (each call is repeated --repeat times; the statistics average over the launches); on its own it prints wall times,
which include the host copies of every call.
python tools/temporal.py [--width 1920] [--height 1080] [--scene chess|cornell] [--repeat 5]
python tools/temporal.py --trace KERNEL_TRACE_CSV [--repeat 5]   sums such a run's kernel trace per pass: the AOV pass and the motion pass
launch the same three kernels first, which the statistics cannot tell apart, so the trace is cut at every k_aov_keys and each piece goes
to the pass whose fold ends it.  The launch counts must fit the calls a run with that --repeat makes, or nothing is printed.
python tools/temporal.py --sequence [--frames 8]   the same frames (seed k + 1 for frame k) twice in one process: through the host-array
loop snapshot / render / render_aovs / render_motion / temporal_blend / denoise / tonemap, and through HipSequence.frame(want=("rgba",)).
Prints the wall time per frame of both (the median over the frames after the first, which warms up) and the sequence's per-stage event
times.  render() returns no variance, so the loop's denoise is fed the variance of one earlier frame: it does the filter's work on the
accumulated image without the cost of getting a variance, which flatters the loop.
  --normal-test / --color-clamp [--clamp-k K]   the sequence rejects stale history (mcpt_sequence_create_ex): also prints, per frame, the
share of pixels whose flags byte has bit 0 (the normal test skipped a tap) and bit 1 (the clamp moved the history).  --no-loop skips the
host-array loop (the sequence alone, e.g. to compare ms_accumulate with and without the switches).
python tools/temporal.py --sequence --adaptive T [--adaptive-min N] [--guided] [--spp CAP] [--move] [--ref-spp 2048]   an adaptive sequence
(mcpt_sequence_create_adaptive: levels N, 2N, ..., CAP; --guided: the threshold relaxed by the history length each pixel is about to get).
Prints, per frame, the total samples, the histogram of the counts, the stage times and the MSE of the accumulated frame against a
--ref-spp render of that frame's geometry (seed 1000).  --move: the short box of the Cornell scene moves by translate(-32 k, 0, 0) before
frame k (a reference per frame; a static scene renders one).  --quality instead of --adaptive: the same figures for a uniform sequence at
--spp samples per pixel.
  --weighted   the history is weighted by sample counts (mcpt_sequence_create_weighted); with --adaptive T --guided the rule is guided by the
history weight.  Prints the mean weight per frame.  --spp-list 64,4,4,4 with --quality: a uniform sequence whose frame k has the k-th count
(the last one repeats), e.g. a caller that lowers params.spp while the camera moves.  --len-mask N: the MSE also over the pixels whose history
length is N in that frame.
  --moments   the variance comes from the temporal moments of each pixel's luminance (mcpt_sequence_create_moments), so --spp 1 is allowed:
python tools/temporal.py --sequence --quality --spp 1 --moments [--min-len 4] [--radius 3].  The sequence is created with filter 1 and every frame
also prints the RMSE after the tone curve (clip(c, 0, 1)^0.45) of the accumulated and of the denoised frame against the reference, and the
share of pixels whose variance is temporal (len >= min_len).  --filtered prints the same two figures for a sequence without moments, whose
filter is guided by the render's own variance: the pair to compare at equal samples is --frames 16 --spp 1 --moments against --frames 8
--spp 2 --filtered.
  --specular-depth N   the sequence's denoise.specular_depth (the features behind up to N mirror / glass bounces); with --specular-motion the
motion follows those chains too and the history is validated against the chain depth (mcpt_sequence_create_motion).  --move with --scene
chess moves the nearest rough pawn by 6 units (about 3.5 px at 1080p) along x per frame, and the MSE is also given over the pixels whose
first hit is the floor mirror, where the pawn's reflection moves.
  --centre-features   every feature pass of the sequence runs on the pixels' centre rays, one per pixel (mcpt_sequence_create_features): the
pair to compare is the same command with and without it, e.g. --sequence --quality --spp 1 --moments [--move].  The last line of every
--quality run gives the median stage times over the frames after the first and the share of pixels whose history reached 4 frames.
  --feedback K   the filter's a-trous iteration K becomes the colour history of the next frame (mcpt_sequence_create_feedback; a filtered
uniform sequence: --moments or --filtered): the pair to compare is the same command with and without it.  Every filtered --quality run of at
least four frames also prints the flicker: the RMS of the frame-to-frame differences of the tone-mapped denoised output over its last four
frames (of a moving scene that includes the motion itself)."""
import argparse
import csv
import re
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import mcpt_loader  # noqa: E402


def summarize_trace(path, repeat):
    """Kernel time per call of each pass, from the sums over all the calls this script made."""
    # render_denoised or the call that feeds the blend, the warm-up call, the repeats; the blend has no first call
    calls_of = {"mcpt_render_aovs": repeat + 2, "mcpt_render_motion": repeat + 2, "a-trous filter": repeat + 2, "mcpt_temporal_blend": repeat + 1}
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_\w+)", r["Kernel_Name"])
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), m.group(1) if m else r["Kernel_Name"][:40]))
    rows.sort()
    folds = {"k_aov_fold": "mcpt_render_aovs", "k_motion_fold": "mcpt_render_motion"}
    alone = {"k_dn_prep": "a-trous filter", "k_dn_atrous": "a-trous filter", "k_dn_remod": "a-trous filter",
             "k_temporal_blend": "mcpt_temporal_blend"}
    per = {}  # pass -> kernel -> [launches, ns]
    piece = None
    # the kernels of a pass: the AOV pass inside render_denoised may overlap the frame's last render kernels, the motion pass runs alone
    own, seen = {"k_aov_resolve", "k_aov_fold"}, None
    for _, _, name in rows:
        seen = set() if name == "k_aov_keys" else seen
        if seen is not None:
            seen.add(name)
            if name in folds:
                own |= seen if name == "k_motion_fold" else set()
                seen = None
    for _, dur, name in rows:
        if piece is not None and name not in own and name not in alone:
            continue
        if name == "k_aov_keys":
            piece = []
        if piece is not None:
            piece.append((name, dur))
            if name in folds:
                for n, d in piece:
                    e = per.setdefault(folds[name], {}).setdefault(n, [0, 0])
                    e[0] += 1
                    e[1] += d
                piece = None
        elif name in alone:
            e = per.setdefault(alone[name], {}).setdefault(name, [0, 0])
            e[0] += 1
            e[1] += dur
    # what marks one call (the two passes run one fold per chunk of rays, the same number in every call)
    once = {"mcpt_render_aovs": "k_aov_fold", "mcpt_render_motion": "k_motion_fold", "a-trous filter": "k_dn_prep", "mcpt_temporal_blend": "k_temporal_blend"}
    for what in ("mcpt_render_aovs", "mcpt_render_motion", "a-trous filter", "mcpt_temporal_blend"):
        k, calls = per.get(what, {}), calls_of[what]
        n = k.get(once[what], [0, 0])[0]
        if n == 0 or n % calls or (what in alone.values() and n != calls):
            sys.exit("%s: %d launches of %s do not fit %d calls: is this the trace of a run with --repeat %d?" % (what, n, once[what], calls, repeat))
        print("%-20s %8.3f ms per call (kernel time, %d calls)" % (what, sum(v[1] for v in k.values()) / calls / 1e6, calls))
        for n, (cnt, ns) in sorted(k.items(), key=lambda kv: -kv[1][1]):
            print("    %-18s %4d launches  %8.3f ms per call  %8.1f us per launch" % (n, cnt, ns / calls / 1e6, ns / cnt / 1e3))


def sequence_timing(pkg, sd, W, H, frames, reject=None, loop=True):
    hs = pkg.HipScene(sd)
    var = hs.render_denoised(spp=4, seed=1, aov_spp=4)["variance"]  # (also sizes the workspace)
    hist, length, prev_depth = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    t_loop = []
    rgba_loop = None
    for k in range(frames if loop else 0):
        t0 = time.perf_counter()
        hs.snapshot()
        c, _ = hs.render(spp=4, seed=k + 1)
        aov = hs.render_aovs(aov_spp=4, seed=k + 1)
        motion = hs.render_motion(seed=k + 1, aov_spp=4)
        hist, length = hs.temporal_blend(c, motion, hist, prev_depth, length)
        rgba_loop = hs.tonemap(hs.denoise(hist, var, aov))
        prev_depth = aov[..., 6].copy()
        t_loop.append(time.perf_counter() - t0)
    seq = hs.sequence(filter=True, aov_spp=4, **(reject or {}))
    t_seq, stages, shares = [], [], []
    for k in range(frames):
        t0 = time.perf_counter()
        r = seq.frame(want=("rgba",), spp=4, seed=k + 1)
        t_seq.append(time.perf_counter() - t0)
        stages.append(r["info"])
        if reject:  # (outside the timed part)
            fl = seq.flags()
            shares.append((100 * float((fl & 1).astype(bool).mean()), 100 * float((fl & 2).astype(bool).mean())))
    med = lambda t: 1e3 * float(np.median(t[1:]))  # noqa: E731
    print("%dx%d, %d frames each, the first not counted" % (W, H, frames))
    if reject:
        print("history rejection: " + ", ".join("%s %s" % kv for kv in sorted(reject.items())))
        for k, (a, b) in enumerate(shares):
            print("    frame %d: normal test skipped a tap in %.2f %% of the pixels, the clamp moved the history in %.2f %%" % (k, a, b))
    if loop:
        print("host-array loop   median wall %.2f ms per frame (min %.2f, max %.2f)" % (med(t_loop), 1e3 * min(t_loop[1:]), 1e3 * max(t_loop[1:])))
    print("sequence          median wall %.2f ms per frame (min %.2f, max %.2f)" % (med(t_seq), 1e3 * min(t_seq[1:]), 1e3 * max(t_seq[1:])))
    print("sequence stages, median event time in ms: " + ", ".join(
        "%s %.3f" % (k[3:], float(np.median([s[k] for s in stages[1:]]))) for k in ("ms_render", "ms_aov", "ms_motion", "ms_accumulate", "ms_filter")))
    print("sequence ms_total (wall time inside the call) median %.2f ms" % float(np.median([s["ms_total"] for s in stages[1:]])))
    print("sequence ms_accumulate per frame: " + " ".join("%.4f" % s["ms_accumulate"] for s in stages[1:]))
    if loop:
        same = float((r["rgba"] == rgba_loop).mean())
        print("last frame: %.2f %% of the rgba bytes equal the loop's (the two filters are guided by different variances)" % (100 * same))
    seq.close()
    hs.close()


def sequence_quality(pkg, sd, W, H, frames, spp, adaptive, reject, move, ref_spp, specular_depth=0, specular_motion=False, weighted=False, spp_list=None,
                     len_mask=0, moments=None, filtered=False, centre=False, feedback=0):
    """Per frame of a uniform (adaptive None) or adaptive sequence: samples, count histogram, stage times, MSE of `accumulated`.
    spp_list: the samples per pixel of frame k of a uniform sequence (the last entry repeats)."""
    hs = pkg.HipScene(sd)
    filtered = filtered or moments is not None
    aov_spp = 1 if centre else min(4, adaptive["min_spp"] if adaptive else min(spp_list or [spp]))
    seq = hs.sequence(filter=filtered, moments=moments if moments is not None else False, aov_spp=aov_spp, adaptive=adaptive, centre_features=centre, feedback=feedback,
                      specular_depth=specular_depth, specular_motion=specular_motion, weighted=weighted, **(reject or {}))
    chess = sd.name.startswith("chess")
    step = 6.0 if chess else -32.0  # object 1: the nearest rough pawn of the chess scene, the short box of the Cornell scene
    floor = None
    if chess:  # Scene::Add order: 14 pawns, the light, the floor
        a, n = int(sd.objects["first_tri"][15]), int(sd.objects["n_tri"][15])
        o, d = hs.camera_rays(np.arange(W * H), np.zeros(W * H, np.int64), seed=1)
        prim = hs.intersect(o, d)[1].reshape(H, W)
        floor = (prim >= a) & (prim < a + n)
        print("specular depth %d, specular motion %s; %.1f %% of the pixels see the floor mirror first" % (specular_depth, bool(specular_motion), 100 * floor.mean()))
    what = ("uniform %s spp" % (",".join(str(x) for x in spp_list) if spp_list else spp)) + (", weighted" if weighted else "") if not adaptive else ("weighted " if weighted else "") + "adaptive %s, levels %d..%d, threshold %g" % (
        "guided" if adaptive["guided"] else "unguided", adaptive["min_spp"], spp, adaptive["threshold"])
    if moments is not None:
        what += ", variance from temporal moments (min_len %d, radius %d)" % (moments["min_len"] or 4, moments["radius"] or 3)
    what += ", features from %s" % ("the centre ray of each pixel" if centre else "%d sampled camera ray%s per pixel" % (aov_spp, "s" * (aov_spp > 1)))
    if feedback:
        what += ", iteration %d of the filter fed back into the history" % feedback
    print("%dx%d %s sequence, %s; reference %d spp" % (W, H, "moving" if move else "static", what, ref_spp))

    def tone_rmse(img):
        with np.errstate(invalid="ignore"):
            d = np.clip(img.astype(np.float64), 0, 1) ** 0.45 - np.clip(truth, 0, 1) ** 0.45
        return float(np.sqrt(np.nanmean(d * d)))

    truth, total, stages, toned = None, 0, [], []
    for k in range(frames):
        if move:
            hs.update([(1, np.array([[1, 0, 0, step * k], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32))])
        if truth is None or move:
            truth = hs.render(spp=ref_spp, seed=1000)[0].astype(np.float64)
        spp_k = spp_list[min(k, len(spp_list) - 1)] if spp_list else spp
        r = seq.frame(want=("accumulated", "len") + (("denoised",) if filtered else ()), spp=spp_k, seed=k + 1)
        sq = (r["accumulated"].astype(np.float64) - truth) ** 2
        mse = float(np.nanmean(sq))
        n = int(r["stats"].samples)
        total += n
        hist = ""
        if adaptive:
            cn = seq.counts()
            lv, cnt = np.unique(cn["spp"], return_counts=True)
            hist = "  counts " + " ".join("%d:%d" % (a, b) for a, b in zip(lv, cnt))
            if adaptive["guided"]:
                hist += "  mean guide %.2f" % float(cn["guide"].mean())
        if weighted:
            hist += "  mean weight %.2f" % float(seq.weight().mean())
        if len_mask:
            keep = r["len"] == len_mask
            hist += "  MSE where len == %d (%.1f %% of the pixels) %.6g" % (len_mask, 100 * keep.mean(), float(np.nanmean(sq[keep])) if keep.any() else float("nan"))
        if filtered:
            toned = (toned + [np.clip(r["denoised"].astype(np.float64), 0, 1) ** 0.45])[-4:]
            hist += "  tone-curve RMSE accumulated %.5f denoised %.5f" % (tone_rmse(r["accumulated"]), tone_rmse(r["denoised"]))
        if moments is not None:
            hist += "  temporal variance in %.1f %% of the pixels" % (100 * float((r["len"] >= (moments["min_len"] or 4)).mean()))
        if floor is not None:
            hist += "  MSE on the floor mirror %.6g" % float(np.nanmean(sq[floor]))
        i = r["info"]
        stages.append(i)
        print("frame %d: %d samples (%.2f per pixel)  MSE %.6g%s  ms: render %.3f aov %.3f motion %.3f accumulate %.3f total %.2f"
              % (k, n, n / (W * H), mse, hist, i["ms_render"], i["ms_aov"], i["ms_motion"], i["ms_accumulate"], i["ms_total"]), flush=True)
    print("all frames: %d samples (%.2f per pixel and frame)" % (total, total / (W * H * frames)))
    if frames > 1:
        print("median over frames 1..%d, ms: " % (frames - 1) + ", ".join("%s %.3f" % (key[3:], float(np.median([s[key] for s in stages[1:]])))
                                                                     for key in ("ms_render", "ms_aov", "ms_motion", "ms_accumulate", "ms_filter", "ms_total"))
              + "; len >= 4 in %.1f %% of the pixels of the last frame" % (100 * float((r["len"] >= 4).mean())))
    if len(toned) == 4:
        d = np.stack([toned[i + 1] - toned[i] for i in range(3)])
        print("flicker: frame-to-frame RMS difference of the tone-mapped denoised output over the last four frames %.5f" % float(np.sqrt(np.nanmean(d * d))))
    seq.close()
    hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", help="a rocprofv3 kernel-trace CSV of a run of this script with the same --repeat: print the kernel time per pass")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="chess", choices=["chess", "cornell"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sequence", action="store_true", help="time the host-array frame loop against HipSequence.frame")
    ap.add_argument("--frames", type=int, default=8, help="--sequence: frames per way (at least 6: one warm-up and five counted)")
    ap.add_argument("--normal-test", action="store_true", help="--sequence: reject taps whose normal differs (mcpt_history_opts)")
    ap.add_argument("--color-clamp", action="store_true", help="--sequence: clamp the history to the new frame's 3x3 neighbourhood")
    ap.add_argument("--clamp-k", type=float, default=0.0, help="--color-clamp: the box's half-width in standard deviations (0: the default)")
    ap.add_argument("--no-loop", action="store_true", help="--sequence: skip the host-array loop")
    ap.add_argument("--adaptive", type=float, default=None, help="--sequence: an adaptive sequence with this threshold; prints samples, counts and MSE")
    ap.add_argument("--adaptive-min", type=int, default=4, help="--adaptive: the first level")
    ap.add_argument("--guided", action="store_true", help="--adaptive: relax each pixel's threshold by sqrt(the history length it is about to get)")
    ap.add_argument("--weighted", action="store_true", help="--adaptive / --quality: weigh the history by sample counts (mcpt_sequence_create_weighted)")
    ap.add_argument("--spp-list", default=None, help="--quality: comma-separated samples per pixel of frame 0, 1, ... (the last one repeats)")
    ap.add_argument("--len-mask", type=int, default=0, help="--adaptive / --quality: also the MSE over the pixels whose history length is this")
    ap.add_argument("--quality", action="store_true", help="--sequence: the figures of --adaptive for a uniform sequence at --spp")
    ap.add_argument("--spp", type=int, default=64, help="--adaptive: the cap; --quality: the samples per pixel")
    ap.add_argument("--move", action="store_true", help="--adaptive / --quality with --scene cornell: move the short box before every frame")
    ap.add_argument("--ref-spp", type=int, default=2048, help="--adaptive / --quality: samples per pixel of the reference")
    ap.add_argument("--moments", action="store_true", help="--quality: the variance from temporal luminance moments (mcpt_sequence_create_moments); allows --spp 1")
    ap.add_argument("--min-len", type=int, default=0, help="--moments: the shortest history whose variance is temporal (0: 4)")
    ap.add_argument("--radius", type=int, default=0, help="--moments: the radius of the spatial window (0: 3)")
    ap.add_argument("--filtered", action="store_true", help="--quality: create the sequence with filter 1 and print the tone-curve RMSE of the denoised frame too")
    ap.add_argument("--specular-depth", type=int, default=0, help="--adaptive / --quality: denoise.specular_depth of the sequence, and the depth of --specular-motion")
    ap.add_argument("--specular-motion", action="store_true", help="--adaptive / --quality: reproject what is seen through mirrors and glass (needs --specular-depth > 0)")
    ap.add_argument("--centre-features", action="store_true", help="--adaptive / --quality: the features of each pixel from its centre ray (mcpt_sequence_create_features)")
    ap.add_argument("--feedback", type=int, default=0, help="--quality with --moments or --filtered: feed this a-trous iteration back into the history (mcpt_sequence_create_feedback)")
    a = ap.parse_args()
    if a.trace:
        return summarize_trace(a.trace, a.repeat)
    pkg = mcpt_loader.load()
    W, H = a.width, a.height
    sd = pkg.scenes.chess_scene(width=W, height=H, spp=4) if a.scene == "chess" else pkg.scenes.cornell_demo(W, H, 4)
    spp_list = [int(x) for x in a.spp_list.split(",")] if a.spp_list else None
    if spp_list and a.adaptive is not None:
        sys.exit("--spp-list is for a uniform sequence (--quality)")
    if a.sequence and (a.adaptive is not None or a.quality or a.move or a.specular_depth > 0 or a.weighted or spp_list or a.moments or a.filtered or a.centre_features or a.feedback):  # (all but the first two imply --quality)
        reject = dict(normal_test=a.normal_test, color_clamp=a.color_clamp, clamp_k=a.clamp_k) if a.normal_test or a.color_clamp else None
        rule = None if a.adaptive is None else dict(min_spp=a.adaptive_min, threshold=a.adaptive, dilate=1, guided=int(a.guided))
        if a.specular_motion and a.specular_depth <= 0:
            sys.exit("--specular-motion needs --specular-depth N > 0")
        return sequence_quality(pkg, sd, W, H, a.frames, a.spp, rule, reject, a.move, a.ref_spp, a.specular_depth, a.specular_motion, a.weighted, spp_list,
                                a.len_mask, dict(min_len=a.min_len, radius=a.radius) if a.moments else None, a.filtered, a.centre_features, a.feedback)
    if a.sequence:
        if a.frames < 6:
            sys.exit("--frames must be at least 6")
        reject = None
        if a.normal_test or a.color_clamp:
            reject = dict(normal_test=a.normal_test, color_clamp=a.color_clamp, clamp_k=a.clamp_k)
        return sequence_timing(pkg, sd, W, H, a.frames, reject, not a.no_loop)
    hs = pkg.HipScene(sd)
    r = hs.render_denoised(spp=4, seed=1, aov_spp=4)  # (also sizes the workspace the AOV and motion passes run in)
    color, var, aov = r["fb"], r["variance"], r["aov"]
    hs.snapshot()
    length = np.ones((H, W), np.float32)

    def wall(name, f):
        f()
        t = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
        print("%-16s median wall %.2f ms (host copies included)" % (name, 1e3 * float(np.median(t))), flush=True)

    wall("render_aovs", lambda: hs.render_aovs(aov_spp=4, seed=1))
    wall("render_motion", lambda: hs.render_motion(seed=1, aov_spp=4))
    motion = hs.render_motion(seed=1, aov_spp=4)
    wall("denoise", lambda: hs.denoise(color, var, aov))
    wall("temporal_blend", lambda: hs.temporal_blend(color, motion, color, aov[..., 6], length))
    wall("snapshot", hs.snapshot)
    print("valid pixels %.1f %%" % (100 * float((motion[..., 3] > 0).mean())))


if __name__ == "__main__":
    main()
