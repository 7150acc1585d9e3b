"""Adaptive sequences on the GPU (include/mcpt.h: mcpt_sequence_create_adaptive, mcpt_sequence_counts): a frame of an adaptive sequence is
the composition of the separate calls -- render_aovs, render_motion, history_len, render_adaptive_guided, temporal_accumulate_ex, denoise --
bit for bit, with the host builder and with PLOC, guided and unguided, with and without history rejection; the first frame and the first
after a reset of a guided sequence are the unguided sequence's; a guided frame never samples a pixel more than mcpt_render_adaptive does,
and its guide is the previous length + 1 where the history holds; a null rule is mcpt_sequence_create_ex; the errors leave history, counts
and frame index alone."""
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


def _threshold(hs, q=0.5):
    """A threshold between two neighbouring S0 estimates of the scene as it stands (seed 1)."""
    _, _, e0, _, _ = hs.render_adaptive(S0, 1e30, spp=S0, seed=1)
    return _mid_threshold(e0, q)


# ---------------------------------------------------------------- 8. the sequence is the composition of the calls
@pytest.mark.parametrize("reject", [False, True])
@pytest.mark.parametrize("guided", [0, 1])
@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("size", [8, 17, 64])
def test_adaptive_sequence_is_the_composition_of_the_calls(pkg, hip, size, builder, guided, reject):
    """Six frames, the short box moved by translate(-32 k, 0, 0) before frame k, as test_gpu_sequence does: with the host builder the
    separate calls run on a second handle, with PLOC on the sequence's own handle before its frame."""
    H = W = size
    sd = pkg.scenes.cornell_demo(W, H, CAP)
    a = hip.HipScene(sd, builder=builder)
    b = a if builder == "ploc" else hip.HipScene(sd, builder=builder)
    thr = _threshold(b)
    rej = dict(normal_test=True, color_clamp=True) if reject else {}
    seq = a.sequence(filter=True, aov_spp=2, adaptive=dict(min_spp=S0, threshold=thr, dilate=1, guided=guided), **rej)
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    hist_var, prev_depth, prev_normal = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    c0 = seq.counts()
    assert (c0["spp"] == 0).all() and (c0["guide"] == 0).all() and c0["info"]["rounds"] == 0  # before the first frame
    levels, relaxed = set(), False
    for k in range(6):
        m = translate(-32.0 * k, 0, 0)
        b.snapshot()
        b.update([(SHORT, m)])
        if a is not b:
            a.update([(SHORT, m)])
        aov = b.render_aovs(aov_spp=2, seed=k + 1)
        motion = b.render_motion(seed=k + 1, aov_spp=2)
        normal = np.ascontiguousarray(aov[..., 3:6])
        guide = b.history_len(motion, hist, prev_depth, length, normal, prev_normal, normal_test=reject) if guided else None
        fb, spp, err, var, info, st = b.render_adaptive_guided(S0, thr, guide, dilate=1, spp=CAP, seed=k + 1)
        acc, acc_var, acc_len, flags = b.temporal_accumulate_ex(fb, var, motion, normal, hist, hist_var, prev_depth, length, prev_normal, **rej)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=ALL, spp=CAP, seed=k + 1)
        cn = seq.counts()
        assert r["info"]["frame_index"] == k
        assert bits_equal(r["aov"], aov), k
        assert bits_equal(r["motion"], motion), k
        assert np.array_equal(cn["spp"], spp), (k, int((cn["spp"] != spp).sum()))
        assert bits_equal(cn["err"], err), k
        assert bits_equal(cn["guide"], guide if guided else np.zeros((H, W), f32)), k
        assert cn["info"]["rounds"] == info["rounds"] and cn["info"]["active_pixels"] == info["active_pixels"], k
        assert bits_equal(r["fb"], fb), k
        assert bits_equal(r["accumulated"], acc) and bits_equal(r["len"], acc_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        assert r["stats"].samples == int(spp.sum()) == st.samples, k
        if reject:
            assert np.array_equal(seq.flags(), flags), k
        if guided:
            # the guide's contract inside a sequence: the length the blend then gave, wherever the frame's colour is finite
            fin = np.isfinite(fb).all(-1)
            assert bits_equal(guide[fin], acc_len[fin]), k
            relaxed |= bool((guide > 1).any())
        levels |= set(int(x) for x in np.unique(spp))
        hist, length, hist_var, prev_depth, prev_normal = acc, acc_len, acc_var, aov[..., 6].copy(), normal
    if size == 64:
        assert len(levels) >= 2, levels
        assert relaxed == bool(guided)
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 9. first frame and reset
def test_first_frame_and_reset_of_a_guided_sequence_are_unguided(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, CAP)
    hu, hg = hip.HipScene(sd), hip.HipScene(sd)
    thr = _threshold(hu)
    rule = dict(min_spp=S0, threshold=thr, dilate=1)
    su = hu.sequence(filter=True, aov_spp=2, adaptive=dict(guided=0, **rule))
    sg = hg.sequence(filter=True, aov_spp=2, adaptive=dict(guided=1, **rule))
    differ = False
    for k in range(5):
        if k == 3:
            su.reset()
            sg.reset()
        ru, rg = su.frame(want=ALL, spp=CAP, seed=k + 1), sg.frame(want=ALL, spp=CAP, seed=k + 1)
        cu, cg = su.counts(), sg.counts()
        assert (cg["spp"] <= cu["spp"]).all(), k  # (the unguided frame is mcpt_render_adaptive of this seed, whatever the history)
        if k in (0, 3):  # no history: the guide is 1 everywhere
            assert (cg["guide"] == 1).all() and rg["info"]["frame_index"] == 0
            assert np.array_equal(cu["spp"], cg["spp"]) and bits_equal(cu["err"], cg["err"])
            for key in ALL:
                assert np.array_equal(ru[key].view(np.uint8), rg[key].view(np.uint8)), (k, key)
        else:
            assert (cg["guide"] > 1).any()
            differ |= not np.array_equal(cu["spp"], cg["spp"])
    assert differ
    for x in (su, sg, hu, hg):
        x.close()


# ---------------------------------------------------------------- 10. guided never samples more
def test_guided_never_samples_more_on_a_static_scene(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, CAP)
    hs, plain = hip.HipScene(sd), hip.HipScene(sd)
    thr = _threshold(plain)
    seq = hs.sequence(filter=False, aov_spp=2, max_history=4, adaptive=dict(min_spp=S0, threshold=thr, dilate=1, guided=1))
    prev_len, fewer = None, 0
    for k in range(7):
        r = seq.frame(want=("fb", "len", "motion"), spp=CAP, seed=k + 1)
        cn = seq.counts()
        _, want_spp, _, _, _ = plain.render_adaptive(S0, thr, dilate=1, spp=CAP, seed=k + 1)
        if k == 0:
            assert np.array_equal(cn["spp"], want_spp) and (cn["guide"] == 1).all()
        else:
            assert (cn["spp"] <= want_spp).all(), k
            fewer += int((cn["spp"] < want_spp).sum())
            # pixels that keep their history: the frame's length is the previous one + 1, capped -- and that is what the guide said
            assert (r["motion"][..., 0:2] == 0).all()
            keeps = r["len"] > 1  # (max_history is 4: a pixel that took history has a length above 1)
            assert keeps.sum() > 1000
            assert np.array_equal(cn["guide"][keeps], np.minimum(prev_len[keeps] + 1, f32(4))), k
            assert bits_equal(cn["guide"][keeps], r["len"][keeps])
        assert r["stats"].samples == int(cn["spp"].sum())
        prev_len = r["len"]
    assert fewer > 0
    for x in (seq, hs, plain):
        x.close()


# ---------------------------------------------------------------- 11. a null rule
@pytest.mark.parametrize("reject", [False, True])
def test_null_rule_is_sequence_create_ex(pkg, hip, reject):
    sd = pkg.scenes.cornell_demo(48, 32, 4)
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    rej = dict(normal_test=True, color_clamp=True) if reject else {}
    sa = hip.HipSequence(a, filter=True, aov_spp=2, create_adaptive=True, **rej)
    sb = b.sequence(filter=True, aov_spp=2, **rej)
    for k in range(3):
        ra, rb = sa.frame(want=ALL, spp=4, seed=k + 1), sb.frame(want=ALL, spp=4, seed=k + 1)
        for key in ALL:
            assert np.array_equal(ra[key].view(np.uint8), rb[key].view(np.uint8)), (k, key)
        assert ra["stats"].samples == rb["stats"].samples == 48 * 32 * 4
        if reject:
            assert np.array_equal(sa.flags(), sb.flags())
    for s in (sa, sb):  # neither keeps counts
        with pytest.raises(hip.McptError) as e:
            s.counts()
        assert e.value.code == 1 and "mcpt_sequence_counts" in str(e.value)
    for x in (sa, sb, a, b):
        x.close()


# ---------------------------------------------------------------- 12. errors
def test_errors_leave_history_counts_and_frame_index(pkg, hip):
    sd = pkg.scenes.cornell_demo(8, 8, CAP)
    hs = hip.HipScene(sd)
    seq = hs.sequence(filter=True, aov_spp=2, adaptive=dict(min_spp=S0, threshold=0.05, dilate=1, guided=1))
    seq.frame(want=("len",), spp=CAP, seed=1)
    r = seq.frame(want=("len",), spp=CAP, seed=2)
    assert r["len"].max() == 2 and r["info"]["frame_index"] == 1
    before = seq.counts()
    other = pkg.scenes.make_camera(9, 8, 40, (278, 273, -800), (278, 273, 0))
    for kw in (dict(spp=24), dict(spp=12), dict(spp=2), dict(spp=3), dict(camera=other, spp=CAP), dict(spp=CAP, nranks=2), dict(spp=CAP, spp_total=CAP),
               dict(spp=CAP, sample_offset=4), dict(spp=CAP, accumulate=1), dict(spp=S0 << 16)):
        with pytest.raises(hip.McptError) as e:
            seq.frame(want=("len",), seed=3, **kw)
        assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value), kw
    after = seq.counts()
    for key in ("spp", "err", "guide"):
        assert np.array_equal(before[key].view(np.uint8), after[key].view(np.uint8)), key
    assert before["info"] == after["info"]
    r = seq.frame(want=("len",), spp=CAP, seed=3)
    assert r["len"].max() == 3 and r["info"]["frame_index"] == 2  # the history goes on counting
    assert (seq.counts()["guide"].max() == 3)
    # R = 0 is a uniform frame at min_spp
    r = seq.frame(want=("len",), spp=S0, seed=4)
    assert (seq.counts()["spp"] == S0).all() and r["stats"].samples == 64 * S0
    # the create-time errors
    for kw in (dict(adaptive=dict(min_spp=1, threshold=0.1)), dict(adaptive=dict(min_spp=4, threshold=-1.0)),
               dict(adaptive=dict(min_spp=4, threshold=0.1, guided=2)), dict(adaptive=dict(min_spp=2, threshold=0.1), aov_spp=4)):
        with pytest.raises(hip.McptError) as e:
            hs.sequence(**kw)
        assert e.value.code == 1 and "mcpt_sequence_create" in str(e.value), kw
    seq.close()
    # a sequence without a rule keeps no counts
    plain = hs.sequence(filter=False, aov_spp=2)
    with pytest.raises(hip.McptError) as e:
        plain.counts()
    assert e.value.code == 1 and "mcpt_sequence_counts" in str(e.value)
    plain.close()
    hs.close()
