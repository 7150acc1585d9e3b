"""Sequences that reproject their reflections (include/mcpt.h: mcpt_sequence_create_motion) on the GPU: a null or zeroed switch is
mcpt_sequence_create_adaptive's sequence bit for bit; with the switch a frame is the composition of the separate calls -- render_aovs and
render_motion at the specular depth, history_len, the render, temporal_accumulate_ex fed the chain planes, denoise -- with the host builder
and with PLOC, plain and adaptive-guided; the ghost of a moved reflection, kept for the whole history without the switch, goes with it while
the reflection that is still there keeps its history; reset and the errors that leave the history alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirror_scene as ms  # noqa: E402
from test_gpu_sequence import ALL  # noqa: E402
from test_temporal_cpu import bits_equal  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
DEPTH = 2
S0, CAP = 4, 16


def box_at(k):
    """The box's transform before frame k: 2.5 units along x per frame, about 3 px of its reflection in the floor."""
    return ms.translate(-6.0 + 2.5 * k, 0, 0)


def same(r, q, keys=ALL):
    for key in keys:
        assert np.array_equal(r[key].view(np.uint8), q[key].view(np.uint8)), key


# ---------------------------------------------------------------- 1. switch off is identity
@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive_guided"])
def test_switch_off_is_identity(pkg, hip, adaptive):
    sd = ms.mirror_scene(pkg)
    scenes = [hip.HipScene(sd) for _ in range(3)]
    kw = dict(filter=True, aov_spp=4, specular_depth=DEPTH)
    if adaptive:
        kw["adaptive"] = dict(min_spp=S0, threshold=0.05, dilate=1, guided=1)
    seqs = [scenes[0].sequence(**kw), hip.HipSequence(scenes[1], motion="null", **kw), hip.HipSequence(scenes[2], motion=hip.SequenceMotion(), **kw)]
    for k in range(3):
        out = []
        for hs, seq in zip(scenes, seqs):
            hs.update([(ms.BOX, box_at(k))])
            out.append(seq.frame(want=ALL, spp=CAP if adaptive else 4, seed=k + 1))
        for q in out[1:]:
            same(out[0], q)
            assert q["stats"].samples == out[0]["stats"].samples
        if adaptive:
            c = [s.counts() for s in seqs]
            for q in c[1:]:
                assert np.array_equal(c[0]["spp"], q["spp"]) and bits_equal(c[0]["err"], q["err"]) and bits_equal(c[0]["guide"], q["guide"])
    assert out[0]["len"].max() == 3 and (out[0]["motion"][..., 0:2] != 0).any()
    # with a specular depth of 0 the switch itself changes nothing
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    sa, sb = a.sequence(filter=True, aov_spp=4), b.sequence(filter=True, aov_spp=4, specular_motion=True)
    for k in range(2):
        a.update([(ms.BOX, box_at(k))])
        b.update([(ms.BOX, box_at(k))])
        same(sa.frame(want=ALL, spp=4, seed=k + 1), sb.frame(want=ALL, spp=4, seed=k + 1))
    for x in seqs + [sa, sb] + scenes + [a, b]:
        x.close()


# ---------------------------------------------------------------- 2. the sequence equals the separate calls
@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive_guided"])
@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_sequence_is_the_composition_of_the_calls(pkg, hip, builder, adaptive):
    """Six frames, the box moved before each, specular depth 2, specular motion, the normal test and the colour clamp on.  The separate calls
    get the planes of the chain AOVs as prev_depth, normal and prev_normal.  With the host builder they run on a second handle; a tree built
    on the device is only promised to agree with another device build up to box-grazing rays, so with PLOC they run on the sequence's own
    handle before its frame (tests/test_gpu_sequence.py): the snapshot they see is the one the sequence took at the end of its last frame."""
    H, W = ms.H, ms.W
    sd = ms.mirror_scene(pkg)
    a = hip.HipScene(sd, builder=builder)
    b = a if builder == "ploc" else hip.HipScene(sd, builder=builder)
    rej = dict(normal_test=True, color_clamp=True)
    thr = 0.05
    kw = dict(adaptive=dict(min_spp=S0, threshold=thr, dilate=1, guided=1)) if adaptive else {}
    seq = a.sequence(filter=True, aov_spp=4, specular_depth=DEPTH, specular_motion=True, **rej, **kw)
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    hist_var, prev_depth, prev_normal = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    moved = flagged = False
    for k in range(6):
        b.snapshot()
        info = b.update([(ms.BOX, box_at(k))])
        assert info["path"] == (1 if builder == "ploc" else 0)
        if a is not b:
            a.update([(ms.BOX, box_at(k))])
        aov = b.render_aovs(aov_spp=4, seed=k + 1, specular_depth=DEPTH)
        motion = b.render_motion(seed=k + 1, aov_spp=4, specular_depth=DEPTH)
        normal = np.ascontiguousarray(aov[..., 3:6])
        first = b.render_motion(seed=k + 1, aov_spp=4)
        if adaptive:
            guide = b.history_len(motion, hist, prev_depth, length, normal, prev_normal, normal_test=True)
            fb, spp, err, var, ainfo, st = b.render_adaptive_guided(S0, thr, guide, dilate=1, spp=CAP, seed=k + 1)
        else:
            rd = b.render_denoised(spp=4, seed=k + 1, aov_spp=4, specular_depth=DEPTH)
            fb, var = rd["fb"], rd["variance"]
            assert bits_equal(rd["aov"], aov)
        acc, acc_var, acc_len, flags = b.temporal_accumulate_ex(fb, var, motion, normal, hist, hist_var, prev_depth, length, prev_normal, **rej)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=ALL, spp=CAP if adaptive else 4, seed=k + 1)
        assert r["info"]["frame_index"] == k
        assert bits_equal(r["aov"], aov), k
        assert bits_equal(r["motion"], motion), k
        assert bits_equal(r["fb"], fb), k
        assert bits_equal(r["accumulated"], acc) and bits_equal(r["len"], acc_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        assert np.array_equal(seq.flags(), flags), k
        if adaptive:
            cn = seq.counts()
            assert np.array_equal(cn["spp"], spp) and bits_equal(cn["err"], err) and bits_equal(cn["guide"], guide), k
            assert cn["info"]["rounds"] == ainfo["rounds"] and cn["info"]["active_pixels"] == ainfo["active_pixels"], k
            assert r["stats"].samples == int(spp.sum()) == st.samples, k
        if k > 0:
            moved |= bool((np.hypot(motion[..., 0], motion[..., 1])[(first[..., 0:2] == 0).all(-1)] > 1).sum() > 100)
            flagged |= bool(flags.any())
        hist, length, hist_var, prev_depth, prev_normal = acc, acc_len, acc_var, aov[..., 6].copy(), normal
    assert moved and flagged and length.max() == 6
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 3. the ghost goes
def test_the_ghost_goes(pkg, hip, oracle):
    """Six frames, the box moving 2.5 units per frame, plain clamp-less sequences at specular depth 2 with and without the switch.
    G: the pixels whose four first hits are the floor in every frame, whose four chains ended on the box in frame 4 and end elsewhere in
       frame 5 (behind the box the back mirror, 14 units and more further along the chain of about 40: over 10 %).  Without the switch
       they keep the stale reflection (len 6 where the first-hit depth passes the 2 % rule and the colours are finite in all frames); with it
       they restart (len 1): the stored chain depth is the box's and the tap fails the depth test.
    T: the pixels whose chains end on the box in all six frames, and whose four reprojected taps, frame after frame, were such pixels too
       and pass the depth test against the stored chain depth: with the switch the reflection that is still there keeps its history, len 6.
    Checked on the CPU when the scene was made, with the oracle's hits and the numpy restatement of the blend's taps: 65 pixels in G, all of
    them passing the first-hit rule, and 188 in T: 4 x the 16 asserted of each."""
    H, W = ms.H, ms.W
    sd = ms.mirror_scene(pkg)
    off, on = hip.HipScene(sd), hip.HipScene(sd)
    s_off = off.sequence(filter=False, aov_spp=4, specular_depth=DEPTH)
    s_on = on.sequence(filter=False, aov_spp=4, specular_depth=DEPTH, specular_motion=True)
    floor, box = ms.prims_of(sd, [ms.FLOOR]), ms.prims_of(sd, [ms.BOX])
    want = ("fb", "len", "aov", "motion")
    floor_all, passes, finite = np.ones((H, W), bool), np.ones((H, W), bool), np.ones((H, W), bool)
    on_box, T = [], None
    prev_sd, prev_first_depth, prev_chain_depth = sd, None, None
    jj, ii = np.mgrid[0:H, 0:W]
    for k in range(6):
        off.update([(ms.BOX, box_at(k))])
        on.update([(ms.BOX, box_at(k))])
        live = ms.moved_scene(pkg, hip, sd, {ms.BOX: box_at(k)})
        chains = ms.chain_motion_f64(oracle, on, live, prev_sd, sd.camera, sd.camera, DEPTH, seed=k + 1)
        first_aov = off.render_aovs(aov_spp=4, seed=k + 1)  # (the sequence's snapshot is untouched by these calls)
        first_motion = off.render_motion(seed=k + 1, aov_spp=4)
        r_off, r_on = s_off.frame(want=want, spp=4, seed=k + 1), s_on.frame(want=want, spp=4, seed=k + 1)
        assert bits_equal(r_off["motion"], first_motion)
        floor_all &= np.isin(chains["first"], floor).all(-1)
        on_box.append(np.isin(chains["last"], box))
        finite &= np.isfinite(r_off["fb"]).all(-1) & np.isfinite(r_on["fb"]).all(-1)
        if k > 0:
            zp = first_motion[..., 2]
            passes &= (first_motion[..., 3] > 0) & (np.abs(prev_first_depth - zp) <= f32(0.02) * zp)
        # T: the taps of the chain motion, as the blend takes them
        mo = r_on["motion"]
        here = on_box[k].all(-1) & finite
        if k == 0:
            T = here
        else:
            fx, fy = ii.astype(f32) + mo[..., 0], jj.astype(f32) + mo[..., 1]
            x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
            ok = here & (mo[..., 3] > 0) & (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)
            x0, y0 = x0.clip(0, W - 2), y0.clip(0, H - 2)
            ztol = f32(0.02) * mo[..., 2]
            for dy in (0, 1):
                for dx in (0, 1):
                    ok &= T[y0 + dy, x0 + dx] & (np.abs(prev_chain_depth[y0 + dy, x0 + dx] - mo[..., 2]) <= ztol)
            T = ok
        prev_sd, prev_first_depth, prev_chain_depth = live, first_aov[..., 6].copy(), r_on["aov"][..., 6].copy()
    G = floor_all & on_box[4].all(-1) & (~on_box[5]).all(-1)
    kept = G & passes & finite
    print("\n[sequence specular] G %d pixels (%d pass the first-hit rule), T %d; without the switch len on G: %s, with it: %s"
          % (int(G.sum()), int(kept.sum()), int(T.sum()), np.unique(r_off["len"][kept]), np.unique(r_on["len"][G])))
    assert G.sum() >= 16 and kept.sum() >= 16 and T.sum() >= 16
    assert (r_off["len"][kept] == 6).all()  # the stale reflection is kept
    assert (r_on["len"][G] == 1).all()      # ... and goes
    assert (r_on["len"][T] == 6).all()      # the reflection that stayed keeps its history
    for x in (s_off, s_on, off, on):
        x.close()


# ---------------------------------------------------------------- 4. reset and errors
def test_reset_and_errors_leave_the_history(pkg, hip):
    sd = ms.mirror_scene(pkg)
    hs = hip.HipScene(sd)
    seq = hs.sequence(filter=True, aov_spp=4, specular_depth=DEPTH, specular_motion=True)
    want = ("fb", "accumulated", "variance", "len", "motion")
    seq.frame(want=want, spp=4, seed=1)
    r = seq.frame(want=want, spp=4, seed=2)
    assert r["len"].max() == 2 and r["info"]["frame_index"] == 1
    other = ms.camera(pkg, 49, 48)
    for kw in (dict(camera=other, spp=4), dict(spp=1), dict(spp=4, nranks=2), dict(spp=2), dict(spp=4, spp_total=8), dict(spp=4, sample_offset=4),
               dict(spp=4, accumulate=1)):
        with pytest.raises(hip.McptError) as e:
            seq.frame(want=("len",), seed=3, **kw)
        assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value), kw
    r = seq.frame(want=want, spp=4, seed=3)
    assert r["len"].max() == 3 and r["info"]["frame_index"] == 2  # the history goes on counting
    seq.reset()
    r = seq.frame(want=want, spp=4, seed=4)
    own = hs.render_denoised(spp=4, seed=4, aov_spp=4, specular_depth=DEPTH)
    assert r["info"]["frame_index"] == 0 and (r["len"] == 1).all() and (r["motion"][..., 0:2] == 0).all()
    assert bits_equal(r["accumulated"], r["fb"]) and bits_equal(r["fb"], own["fb"]) and bits_equal(r["variance"], own["variance"])
    # a 2 degree pan without a reset: the chain motion against the remembered camera of the previous frame
    pan = ms.camera(pkg, pan_deg=2.0)
    r = seq.frame(camera=pan, want=want, spp=4, seed=5)
    assert bits_equal(r["motion"], hs.render_motion(prev_camera=sd.camera, camera=pan, seed=5, aov_spp=4, specular_depth=DEPTH))
    assert r["len"].max() == 2
    seq.close()
    seq.close()  # idempotent
    for kw in (dict(motion=hip.SequenceMotion(specular_motion=2)), dict(specular_motion=True, max_history=5000)):
        with pytest.raises(hip.McptError) as e:
            hip.HipSequence(hs, filter=True, specular_depth=DEPTH, **kw)
        assert e.value.code == 1 and "mcpt_sequence_create" in str(e.value), kw
    bad = hip.SequenceMotion(specular_motion=1)
    bad.reserved[6] = 1
    with pytest.raises(hip.McptError):
        hip.HipSequence(hs, filter=True, specular_depth=DEPTH, motion=bad)
    seq = hs.sequence(filter=False, specular_depth=DEPTH, specular_motion=True)  # the refused creations left the scene usable
    assert seq.frame(want=("len",), spp=4, seed=1)["len"].max() == 1
    seq.close()
    hs.close()
