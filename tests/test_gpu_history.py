"""History rejection on the GPU (include/mcpt.h: mcpt_temporal_accumulate_ex, mcpt_sequence_create_ex, mcpt_sequence_flags):
every instantiation of k_temporal_accumulate gives the bits of the CPU build of tp::accumulate_pixel_ex, flags included; with zeroed options the call is
mcpt_temporal_accumulate; a sequence with both switches on is the composition of the separate calls, bit for bit, and one with zeroed
options is a plain sequence; a failed frame leaves history, normals and flags alone; after the light has moved the clamp brings the
accumulated frame closer to the new lighting than the parent's blend does; and on a scene that never moves it costs no more than twice the
seed-to-seed spread of the unclamped error.

Measured on the MI355X (the 48 x 32 Cornell scene below, 4 spp per frame, aov_spp 2, RMSE of `accumulated` against 4096 spp; DESIGN
section 8f has the same figures):
  static scene, frame 16, seeds 1 / 101 / 201, both switches off: 0.123635 0.127133 0.123441, mean 0.124736, spread (max - min) 0.003693
  color_clamp, clamp_k 1:    0.117753 0.122580 0.117596, mean 0.119310 (1.47 spreads BELOW off); 13.7 / 13.0 / 13.2 % of the pixels clamped
  color_clamp, clamp_k 1.5:  0.118018 0.122493 0.117913, mean 0.119474; 8.8 / 8.3 / 8.3 % clamped
  color_clamp, clamp_k 2:    0.118659 0.122893 0.118420, mean 0.119991; 6.4 / 5.6 / 5.7 % clamped
  color_clamp, clamp_k 3:    0.119807 0.123869 0.119394, mean 0.121024; 3.6 / 3.4 / 3.5 % clamped
Every candidate stays inside the spread of the off figure (each is below it: at 4 spp the error is dominated by fireflies, and the clamp
also pulls a firefly that sits in the history back to its neighbourhood), so the default is the smallest, clamp_k 1.
  normal_test alone, static: 0.126720 0.130439 0.130093 (edge pixels whose folded normal is shorter than sqrt(0.9) restart every frame);
  flag bit 0 is set on 0 % of the pixels of this scene (zero motion reads one tap: a skipped tap leaves no history, so no flag).
  light moved before frame 13, RMSE against 4096 spp of the moved scene in frames 13 / 14 / 15 (the two references differ by 0.572):
    off 0.8840 0.5482 0.7074;  color_clamp 0.8789 0.5445 0.6960;  both switches 0.8794 0.5455 0.7058
  (the figure swings with each new frame's own fireflies, which the clamp does not touch: it clamps the history, not the frame);
  share of pixels with flag bit 1 (color_clamp): frame 12 (last static) 14.3 %, frames 13 / 14 / 15: 24.7 / 19.0 / 16.3 %.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import SHAPES, bits_equal  # noqa: E402
from test_history_cpu import HIST_KINDS, SWITCHES, build_driver, history_case, host_accumulate_ex, plain_args  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHORT, LIGHT = 1, 5  # cornell_demo, Scene::Add order: floor, short box, tall box, left, right, light, ...
ALL = ("fb", "accumulated", "denoised", "variance", "len", "aov", "motion", "rgba")
W, H, SPP, AOV_SPP = 48, 32, 4, 2
# The light moves by a third of the room's width (and a little down and back): further than either box is wide, so the boxes' shadows and
# the bright patch of the ceiling's bounce leave the pixels they were in, while the first hit of every pixel but the light's own stays.
LIGHT_MOVE = (-180.0, -20.0, 60.0)
CANDIDATES = (1.0, 1.5, 2.0, 3.0)


def translate(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], f32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("hist_gpu"))


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


# ---------------------------------------------------------------- 1. the kernel against the CPU build
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", HIST_KINDS)
def test_accumulate_ex_device_equals_host_build(hip, tiny, driver, kind, shape):
    Hh, Ww = shape
    args, opts, values = history_case(kind, Hh, Ww)
    for nt, cc in SWITCHES:
        hist = dict(normal_test=nt, color_clamp=cc, **values)
        got, got_var, got_len, got_flags = tiny.temporal_accumulate_ex(*args, **hist, **opts)
        want, want_var, want_len, want_flags = host_accumulate_ex(driver, hip, *args, history=hist, **opts)
        assert bits_equal(got, want), (nt, cc, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert bits_equal(got_var, want_var), (nt, cc)
        assert bits_equal(got_len, want_len), (nt, cc)
        assert np.array_equal(got_flags, want_flags), (nt, cc)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", HIST_KINDS)
def test_zeroed_history_opts_is_temporal_accumulate(hip, tiny, kind, shape):
    Hh, Ww = shape
    args, opts, values = history_case(kind, Hh, Ww)
    want, want_var, want_len = tiny.temporal_accumulate(*plain_args(args), **opts)
    for normals in (True, False):
        a = list(args)
        if not normals:
            a[3] = a[8] = None  # not read: may be null
        got, got_var, got_len, flags = tiny.temporal_accumulate_ex(*a, **opts)
        assert bits_equal(got, want) and bits_equal(got_var, want_var) and bits_equal(got_len, want_len)
        assert (flags == 0).all()


# ---------------------------------------------------------------- 2. the sequence is the composition of the calls
@pytest.mark.parametrize("specular_depth", [0, 1])
def test_sequence_with_rejection_is_the_composition_of_the_calls(pkg, hip, specular_depth):
    """Three frames; the short box moves between the first and the second.  The separate calls run on a second handle."""
    sd = pkg.scenes.cornell_demo(W, H, SPP)
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    seq = a.sequence(filter=True, aov_spp=AOV_SPP, specular_depth=specular_depth, normal_test=True, color_clamp=True)
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    hist_var, prev_depth, prev_normal = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    assert (seq.flags() == 0).all()  # before the first frame
    seen = 0
    for k in range(3):
        b.snapshot()
        if k == 1:
            m = translate(-40.0, 0, 20.0)
            b.update([(SHORT, m)])
            a.update([(SHORT, m)])
        rd = b.render_denoised(spp=SPP, seed=k + 1, aov_spp=AOV_SPP, specular_depth=specular_depth)
        c, aov = rd["fb"], rd["aov"]
        first = b.render_aovs(aov_spp=AOV_SPP, seed=k + 1) if specular_depth else aov
        motion = b.render_motion(seed=k + 1, aov_spp=AOV_SPP)
        normal = np.ascontiguousarray(first[..., 3:6])
        acc, acc_var, acc_len, flags = b.temporal_accumulate_ex(c, rd["variance"], motion, normal, hist, hist_var, prev_depth, length, prev_normal,
                                                                normal_test=True, color_clamp=True)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=ALL, spp=SPP, seed=k + 1)
        assert bits_equal(r["fb"], c), k
        assert bits_equal(r["aov"], aov), k
        assert bits_equal(r["motion"], motion), k
        assert bits_equal(r["accumulated"], acc) and bits_equal(r["len"], acc_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        assert np.array_equal(seq.flags(), flags), k
        if k == 0:
            assert (flags == 0).all() and (acc_len == 1).all()
        else:
            assert (acc_len > 1).any()
            seen |= int(np.bitwise_or.reduce(flags.reshape(-1)))
        hist, length, hist_var, prev_depth, prev_normal = acc, acc_len, acc_var, first[..., 6].copy(), normal
    assert seen & 2  # the clamp did act in these frames (4 spp: the history of one or two frames is often outside one deviation)
    for x in (seq, a, b):
        x.close()


def test_sequence_ex_with_zeroed_opts_is_a_plain_sequence(pkg, hip):
    sd = pkg.scenes.cornell_demo(W, H, SPP)
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    plain = a.sequence(filter=True, aov_spp=AOV_SPP)
    zeroed = hip.HipSequence(b, filter=True, aov_spp=AOV_SPP, history=hip.history_opts())
    for k in range(3):
        if k == 1:
            for hs in (a, b):
                hs.update([(SHORT, translate(-40.0, 0, 20.0))])
        r, q = plain.frame(want=ALL, spp=SPP, seed=k + 1), zeroed.frame(want=ALL, spp=SPP, seed=k + 1)
        for name in ALL:
            assert (np.array_equal if name == "rgba" else bits_equal)(r[name], q[name]), (k, name)
    assert r["len"].max() == 3
    for s in (plain, zeroed):
        with pytest.raises(hip.McptError) as e:  # neither keeps flags
            s.flags()
        assert e.value.code == 1 and "mcpt_sequence_flags" in str(e.value)
    for x in (plain, zeroed, a, b):
        x.close()


# ---------------------------------------------------------------- 3. a failed frame
def test_failed_frame_leaves_history_normals_and_flags(pkg, hip):
    sd = pkg.scenes.cornell_demo(W, H, SPP)
    a, b = hip.HipScene(sd), hip.HipScene(sd)
    kw = dict(filter=False, aov_spp=4, normal_test=True, color_clamp=True)
    s, twin = a.sequence(**kw), b.sequence(**kw)
    want = ("accumulated", "variance", "len")
    for k in range(2):
        r, q = s.frame(want=want, spp=4, seed=k + 1), twin.frame(want=want, spp=4, seed=k + 1)
    before = s.flags()
    assert before.any() and np.array_equal(before, twin.flags())
    with pytest.raises(hip.McptError) as e:
        s.frame(want=want, spp=2, seed=3)  # aov_spp 4 > spp 2
    assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value)
    assert np.array_equal(s.flags(), before)
    r, q = s.frame(want=want, spp=4, seed=3), twin.frame(want=want, spp=4, seed=3)
    for name in want:
        assert bits_equal(r[name], q[name]), name
    assert np.array_equal(s.flags(), twin.flags()) and r["info"]["frame_index"] == 2 and r["len"].max() == 3
    for x in (s, twin, a, b):
        x.close()


# ---------------------------------------------------------------- 4., 5. what the feature is for, and what it costs
def rmse(img, ref):
    return float(np.sqrt(((np.asarray(img, np.float64) - ref) ** 2).mean()))


def run_frames(hs, frames, base_seed, move_after=None, **seq_kw):
    """`frames` frames of a sequence on hs (seed base_seed + k for frame k); the light moves by LIGHT_MOVE before frame `move_after`.
    Returns the accumulated frames and, for a sequence with rejection, each frame's share of pixels with flag bit 0 and bit 1."""
    seq = hs.sequence(filter=False, aov_spp=AOV_SPP, **seq_kw)
    rejecting = bool(seq_kw.get("normal_test") or seq_kw.get("color_clamp"))
    acc, shares = [], []
    for k in range(frames):
        if k == move_after:
            hs.update([(LIGHT, translate(*LIGHT_MOVE))])
        acc.append(seq.frame(want=("accumulated",), spp=SPP, seed=base_seed + k)["accumulated"])
        if rejecting:
            fl = seq.flags()
            shares.append((float((fl & 1).astype(bool).mean()), float((fl & 2).astype(bool).mean())))
    seq.close()
    return acc, shares


@pytest.fixture(scope="module")
def references(pkg, hip):
    """4096-spp renders of the 48 x 32 scene as it is and with the light moved: computed once, shared, not modified."""
    sd = pkg.scenes.cornell_demo(W, H, SPP)
    hs = hip.HipScene(sd)
    static, _ = hs.render(spp=4096, seed=777)
    hs.update([(LIGHT, translate(*LIGHT_MOVE))])
    moved, _ = hs.render(spp=4096, seed=777)
    hs.close()
    static.setflags(write=False)
    moved.setflags(write=False)
    return sd, static.astype(np.float64), moved.astype(np.float64)


def test_clamp_follows_a_moved_light(hip, references):
    """12 static frames, the light moves, 3 more frames.  At the third frame after the move the accumulated frame is closer (RMSE against 4096
    spp of the moved scene) with color_clamp than with both switches off, which is the parent's blend: a direction, not a threshold.  And
    the clamp acts on more pixels in the first frame after the move than in the last static one."""
    sd, _, moved = references
    out = {}
    for name, kw in (("off", {}), ("clamp", dict(color_clamp=True)), ("both", dict(normal_test=True, color_clamp=True))):
        hs = hip.HipScene(sd)
        out[name] = run_frames(hs, 15, 1, move_after=12, **kw)
        hs.close()
    err = {name: [rmse(f, moved) for f in acc[12:]] for name, (acc, _) in out.items()}
    for name in ("off", "clamp", "both"):
        print("moved light, RMSE against 4096 spp of the moved scene, frames 1-3 after the move, %-5s: %s"
              % (name, " ".join("%.4f" % e for e in err[name])))
    shares = out["clamp"][1]
    print("color_clamp: share of pixels with flag bit 1, last static frame %.4f, frames after the move %s"
          % (shares[11][1], " ".join("%.4f" % s[1] for s in shares[12:])))
    print("both switches: share with bit 0 / bit 1 per frame: " + " ".join("%.3f/%.3f" % s for s in out["both"][1]))
    assert err["clamp"][2] < err["off"][2]
    assert shares[12][1] > shares[11][1]


def static_errors(hip, sd, static, **kw):
    """RMSE of the 16th accumulated frame of a scene that never moves, for the three seeds."""
    res = []
    for seed in (1, 101, 201):
        hs = hip.HipScene(sd)
        acc, shares = run_frames(hs, 16, seed, **kw)
        hs.close()
        res.append((rmse(acc[-1], static), shares[-1] if shares else None))
    return res


def test_static_cost_of_the_clamp(hip, references):
    """16 frames of the scene that never moves, three seeds: the RMSE (against 4096 spp) with color_clamp at its default clamp_k is at most
    that without it plus twice the spread (max - min) of the unclamped figure across the seeds, each measured here."""
    sd, static, _ = references
    off = [e for e, _ in static_errors(hip, sd, static)]
    on = static_errors(hip, sd, static, color_clamp=True)
    spread = max(off) - min(off)
    print("static scene, 16 frames, RMSE against 4096 spp: off %s (mean %.5f, spread %.5f)" % (" ".join("%.5f" % e for e in off), np.mean(off), spread))
    print("static scene, color_clamp with the default clamp_k: %s (mean %.5f); share of pixels clamped in frame 16: %s"
          % (" ".join("%.5f" % e for e, _ in on), np.mean([e for e, _ in on]), " ".join("%.3f" % s[1] for _, s in on)))
    assert np.mean([e for e, _ in on]) <= np.mean(off) + 2 * spread
