"""Weighted sequences on the GPU (include/mcpt.h: mcpt_sequence_create_weighted, mcpt_sequence_weight): a frame of a weighted sequence is
the composition of the separate calls -- render_aovs, render_motion, history_weight, render_adaptive_weighted or render_denoised,
temporal_accumulate_weighted, denoise -- bit for bit, uniform (at a params.spp that changes from frame to frame), adaptive and adaptive
guided, with and without history rejection, with the host builder and with PLOC; a null or zeroed switch is mcpt_sequence_create_motion; a
uniform sequence at a constant spp is the unweighted sequence with weight = len * spp; a reset restarts the weights and a refused frame
leaves them alone; and on a static scene whose first frame has 64 samples and the next three 4 each the weighted history has less than half
the unweighted one's error."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import bits_equal  # noqa: E402
from test_gpu_adaptive import _mid_threshold  # noqa: E402
from test_gpu_sequence import ALL, SHORT, translate  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
S0, CAP = 4, 16
UNIFORM_SPP = (16, 4, 4, 8, 4, 16)  # a uniform sequence whose caller changes params.spp from frame to frame


def _threshold(hs, q=0.5):
    """A threshold between two neighbouring S0 estimates of the scene as it stands (seed 1)."""
    _, _, e0, _, _ = hs.render_adaptive(S0, 1e30, spp=S0, seed=1)
    return _mid_threshold(e0, q)


# ---------------------------------------------------------------- 1. the sequence is the composition of the calls
@pytest.mark.parametrize("reject", [False, True])
@pytest.mark.parametrize("mode", ["uniform", "adaptive", "guided"])
@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("size", [8, 17, 64])
def test_weighted_sequence_is_the_composition_of_the_calls(pkg, hip, size, builder, mode, reject):
    """Six frames, the short box moved by translate(-32 k, 0, 0) before frame k, as test_gpu_sequence_adaptive does: with the host builder
    the separate calls run on a second handle, with PLOC on the sequence's own handle before its frame."""
    H = W = size
    sd = pkg.scenes.cornell_demo(W, H, CAP)
    a = hip.HipScene(sd, builder=builder)
    b = a if builder == "ploc" else hip.HipScene(sd, builder=builder)
    thr = _threshold(b)
    rej = dict(normal_test=True, color_clamp=True) if reject else {}
    adaptive = None if mode == "uniform" else dict(min_spp=S0, threshold=thr, dilate=1, guided=int(mode == "guided"))
    seq = a.sequence(filter=True, aov_spp=2, adaptive=adaptive, weighted=True, **rej)
    assert (seq.weight() == 0).all()  # before the first frame
    hist, length, weight = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
    hist_var, prev_depth, prev_normal = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    mh = f32(32)
    relaxed, unequal = False, False
    for k in range(6):
        m = translate(-32.0 * k, 0, 0)
        b.snapshot()
        b.update([(SHORT, m)])
        if a is not b:
            a.update([(SHORT, m)])
        aov = b.render_aovs(aov_spp=2, seed=k + 1)
        motion = b.render_motion(seed=k + 1, aov_spp=2)
        normal = np.ascontiguousarray(aov[..., 3:6])
        if mode == "uniform":
            spp_k = UNIFORM_SPP[k]
            rd = b.render_denoised(spp=spp_k, seed=k + 1, aov_spp=2)
            fb, var, count = rd["fb"], rd["variance"], float(spp_k)
        else:
            spp_k = CAP
            guide = b.history_weight(motion, hist, prev_depth, length, weight, normal, prev_normal, normal_test=reject) if mode == "guided" else None
            fb, spp, err, var, info, st = b.render_adaptive_weighted(S0, thr, guide, dilate=1, spp=CAP, seed=k + 1)
            count = spp
        acc, acc_var, acc_len, flags, acc_w = b.temporal_accumulate_weighted(fb, var, motion, normal, count, hist, hist_var, prev_depth, length,
                                                                            prev_normal, weight, **rej)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=ALL, spp=spp_k, seed=k + 1)
        assert r["info"]["frame_index"] == k
        assert bits_equal(r["aov"], aov) and bits_equal(r["motion"], motion), k
        assert bits_equal(r["fb"], fb), k
        assert bits_equal(r["accumulated"], acc) and bits_equal(r["len"], acc_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(seq.weight(), acc_w), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        if reject:
            assert np.array_equal(seq.flags(), flags), k
        s = np.full((H, W), f32(spp_k)) if mode == "uniform" else spp.astype(f32)
        if mode != "uniform":
            cn = seq.counts()
            assert np.array_equal(cn["spp"], spp) and bits_equal(cn["err"], err), k
            assert bits_equal(cn["guide"], guide if mode == "guided" else np.zeros((H, W), f32)), k
            assert cn["info"]["active_pixels"] == info["active_pixels"] and r["stats"].samples == int(spp.sum()) == st.samples, k
        if mode == "guided":
            # the guide's contract inside a sequence: the weight the blend then gave, wherever the frame's colour is finite
            fin = np.isfinite(fb).all(-1)
            cap = (mh - f32(1)) * s
            assert bits_equal(acc_w[fin], (np.where(guide < cap, guide, cap) + s)[fin]), k
            relaxed |= bool((guide > 0).any())
        assert (acc_w >= s).all() and (acc_w[acc_len == 1] == s[acc_len == 1]).all()
        unequal |= bool((acc_w != acc_len * s).any())
        hist, length, hist_var, prev_depth, prev_normal, weight = acc, acc_len, acc_var, aov[..., 6].copy(), normal, acc_w
    if size == 64:
        assert unequal  # frames of different counts met in one pixel
        assert relaxed == (mode == "guided")
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 2. a null or zeroed switch
@pytest.mark.parametrize("adaptive", [False, True])
def test_null_or_zeroed_switch_is_sequence_create_motion(pkg, hip, adaptive):
    sd = pkg.scenes.cornell_demo(48, 32, CAP)
    scenes = [hip.HipScene(sd) for _ in range(3)]
    ad = dict(min_spp=S0, threshold=0.1, dilate=1, guided=1) if adaptive else None
    kw = dict(filter=True, aov_spp=2, normal_test=True, color_clamp=True, specular_depth=2, specular_motion=True)
    seqs = [hip.HipSequence(scenes[0], adaptive=ad, **kw), hip.HipSequence(scenes[1], adaptive=ad, weighted="null", **kw),
            hip.HipSequence(scenes[2], adaptive=ad, weighted=hip.SequenceWeighted(), **kw)]
    for k in range(3):
        rs = [s.frame(want=ALL, spp=CAP, seed=k + 1) for s in seqs]
        for r in rs[1:]:
            for key in ALL:
                assert np.array_equal(r[key].view(np.uint8), rs[0][key].view(np.uint8)), (k, key)
            assert r["stats"].samples == rs[0]["stats"].samples
        assert np.array_equal(seqs[1].flags(), seqs[0].flags()) and np.array_equal(seqs[2].flags(), seqs[0].flags())
        if adaptive:
            cs = [s.counts() for s in seqs]
            for c in cs[1:]:
                assert all(np.array_equal(c[key].view(np.uint8), cs[0][key].view(np.uint8)) for key in ("spp", "err", "guide"))
    for s in seqs:  # none keeps weights
        with pytest.raises(hip.McptError) as e:
            s.weight()
        assert e.value.code == 1 and "mcpt_sequence_weight" in str(e.value)
    for x in seqs + scenes:
        x.close()


# ---------------------------------------------------------------- 3. a uniform sequence at a constant spp
@pytest.mark.parametrize("reject", [False, True])
def test_constant_spp_is_the_unweighted_sequence(pkg, hip, reject):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    rej = dict(normal_test=True, color_clamp=True) if reject else {}
    sw, su = a.sequence(filter=True, aov_spp=2, max_history=4, weighted=True, **rej), b.sequence(filter=True, aov_spp=2, max_history=4, **rej)
    for k in range(6):
        m = translate(-32.0 * k, 0, 0)
        a.update([(SHORT, m)])
        b.update([(SHORT, m)])
        rw, ru = sw.frame(want=ALL, spp=4, seed=k + 1), su.frame(want=ALL, spp=4, seed=k + 1)
        for key in ALL:
            assert np.array_equal(rw[key].view(np.uint8), ru[key].view(np.uint8)), (k, key)
        assert bits_equal(sw.weight(), ru["len"] * f32(4)), k
        if reject:
            assert np.array_equal(sw.flags(), su.flags())
    assert ru["len"].max() == 4 and (ru["len"] == 1).any()
    for x in (sw, su, a, b):
        x.close()


# ---------------------------------------------------------------- 4. reset and failed frames
def test_reset_and_refused_frames(pkg, hip):
    sd = pkg.scenes.cornell_demo(8, 8, CAP)
    hs = hip.HipScene(sd)
    seq = hs.sequence(filter=False, aov_spp=2, weighted=True)
    seq.frame(want=("len",), spp=16, seed=1)
    r = seq.frame(want=("len", "accumulated"), spp=4, seed=2)
    w = seq.weight()
    assert r["len"].max() == 2 and w.max() == 20 and r["info"]["frame_index"] == 1
    other = pkg.scenes.make_camera(9, 8, 40, (278, 273, -800), (278, 273, 0))
    for kw in (dict(spp=1), dict(camera=other, spp=4), dict(spp=4, nranks=2), dict(spp=4, spp_total=4), dict(spp=4, accumulate=1)):
        with pytest.raises(hip.McptError) as e:
            seq.frame(want=("len",), seed=3, **kw)
        assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value), kw
        assert bits_equal(seq.weight(), w)
    r3 = seq.frame(want=("len", "accumulated"), spp=8, seed=3)
    assert r3["len"].max() == 3 and r3["info"]["frame_index"] == 2 and seq.weight().max() == 28  # the history went on from where it was
    seq.reset()
    assert seq.weight().max() == 28  # the last frame's weights stay readable
    r = seq.frame(want=("len", "fb", "accumulated"), spp=4, seed=4)
    fin = np.isfinite(r["fb"]).all(-1)
    assert r["info"]["frame_index"] == 0 and (r["len"] == 1).all() and (seq.weight()[fin] == 4).all() and fin.any()
    assert bits_equal(r["accumulated"], r["fb"])
    seq.close()
    # an adaptive sequence: after a reset the weights are the count map
    seq = hs.sequence(filter=False, aov_spp=2, weighted=True, adaptive=dict(min_spp=S0, threshold=_threshold(hs), dilate=1, guided=1))
    seq.frame(want=("len",), spp=CAP, seed=1)
    seq.frame(want=("len",), spp=CAP, seed=2)
    assert (seq.counts()["guide"] > 0).any()
    seq.reset()
    seq.frame(want=("len",), spp=CAP, seed=3)
    cn = seq.counts()
    assert (cn["guide"] == 0).all() and bits_equal(seq.weight(), cn["spp"].astype(f32))
    seq.close()
    # the create-time errors
    for wd in (hip.SequenceWeighted(weighted=2), hip.SequenceWeighted(weighted=-1)):
        with pytest.raises(hip.McptError) as e:
            hip.HipSequence(hs, weighted=wd)
        assert e.value.code == 1 and "weighted" in str(e.value)
    hs.close()


# ---------------------------------------------------------------- 5. quality
def test_weighted_history_keeps_the_good_frame(pkg, hip):
    """Static Cornell demo 64 x 64, uniform frames of (64, 4, 4, 4) samples, seeds 1..4, weighted against unweighted; the MSE of `accumulated`
    in frame 3 against a 4096-spp render of another seed, over the pixels whose len is 4 in both runs (len is the same plane in both: the
    weights do not enter it).  Condition: those pixels are at least half of the covered ones (79.7 % of the pixels of
    this scene keep their history over eight frames).  From the counts alone the weighted pixel has variance sigma^2 / 76 and the unweighted
    one (sigma^2 / 64 + 3 sigma^2 / 4) / 16, a ratio of 0.275; zero motion reads a single tap, so nothing is blurred.  The bound 0.5 leaves
    room for the reference's own noise (sigma^2 / 4096 on both sides) and the heavy-tailed pixels."""
    sd = pkg.scenes.cornell_demo(64, 64, 64)
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    ref, _ = a.render(spp=4096, seed=99)
    sw, su = a.sequence(filter=False, aov_spp=4, weighted=True), b.sequence(filter=False, aov_spp=4)
    for k, spp in enumerate((64, 4, 4, 4)):
        rw = sw.frame(want=("accumulated", "len", "aov"), spp=spp, seed=k + 1)
        ru = su.frame(want=("accumulated", "len"), spp=spp, seed=k + 1)
    assert bits_equal(rw["len"], ru["len"])
    covered = rw["aov"][..., 7] > 0
    keep = (rw["len"] == 4) & np.isfinite(ref).all(-1) & np.isfinite(rw["accumulated"]).all(-1) & np.isfinite(ru["accumulated"]).all(-1)
    assert keep.sum() >= 0.5 * covered.sum(), (int(keep.sum()), int(covered.sum()))
    assert (sw.weight()[keep] == 76).all()
    mse_w = float(((rw["accumulated"][keep].astype(np.float64) - ref[keep]) ** 2).mean())
    mse_u = float(((ru["accumulated"][keep].astype(np.float64) - ref[keep]) ** 2).mean())
    print("weighted history, spp (64, 4, 4, 4): %d of %d covered pixels keep len 4; MSE weighted %.6g, unweighted %.6g, ratio %.3f"
          % (int(keep.sum()), int(covered.sum()), mse_w, mse_u, mse_w / mse_u))
    assert mse_w / mse_u < 0.5
    for x in (sw, su, a, b):
        x.close()
