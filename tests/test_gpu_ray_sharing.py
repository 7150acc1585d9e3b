"""Shared continuation rays (k_shade in csrc/mcpt_kernels.hip): the channel paths of a sample that leave a
smooth-conductor vertex together continue on one ray instead of three copies of it.  Nothing may change but the number of rays
k_trace_closest walks: frames are equal bit for bit with the sharing on and off (MCPT_SHARE_RAYS=0), every work counter of mcpt_stats
is equal (closest_rays and ref_scene_rays count resolved rays), the oracle's frame is reproduced, the schedule does not matter, and on
a mirror floor the share of records that ride on a sibling's ray is what the roulette rate predicts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import material_zoo as zoo  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "paths", "vertices", "shaded", "closest_rays", "shadow_rays", "direct_vertices", "ref_scene_rays", "overflow_paths")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _quad(S, corners, towards):
    """Two triangles over the four corners (in order round the quad), wound so that the normal cross(v1 - v0, v2 - v0) points to the
    side `towards` lies on."""
    a, b, c, d = [np.asarray(p, np.float64) for p in corners]
    if np.dot(np.cross(b - a, c - a), np.asarray(towards, np.float64) - a) < 0:
        b, d = d, b
    t = np.zeros(2, S.TRI_DTYPE)
    t[0]["v0"], t[0]["v1"], t[0]["v2"] = a, b, c
    t[1]["v0"], t[1]["v1"], t[1]["v2"] = a, c, d
    return t


def floor_scene(pkg, width, height, rr_rate=0.4):
    """A silver-mirror floor that fills the view, under a constant sky, no emitter: every sample has one vertex, on the floor, and its
    continuation rays leave for the sky."""
    S = pkg.scenes
    b = S._Builder()
    b.add_mesh(_quad(S, [(-500, 0, -500), (-500, 0, 500), (500, 0, 500), (500, 0, -500)], (0, 1, 0)),
               b.material("silver_mirror", S.material_presets()["silver_mirror"]))
    cam = S.make_camera(width, height, 50, (0, 30, -5), (0, 0, 0))
    return b.finish(camera=cam, rr_rate=rr_rate, spp=8, background=np.float32([0.3, 0.5, 0.8]), name="mirror floor")


def conductor_box(pkg, width, height):
    """A closed box whose six walls are smooth conductors (silver and gold), a gold block on the floor and one emitter under the
    ceiling; the camera is inside.  rr_rate 0.9: paths of ten vertices on average whose channel siblings stay on one ray for many
    bounces."""
    S = pkg.scenes
    P = S.material_presets()
    b = S._Builder()
    silver, gold = b.material("silver_mirror", P["silver_mirror"]), b.material("gold_conductor", P["gold_conductor"])
    lo, hi, mid = np.float64([-20, 0, -20]), np.float64([20, 30, 20]), (0, 15, 0)
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    walls = [[(x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0)], [(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)],
             [(x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)], [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
             [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]]
    for k, w in enumerate(walls):
        b.add_mesh(_quad(S, w, mid), gold if k in (2, 5) else silver)
    # a tilted gold plate on the floor (two-sided use: both of its faces are seen)
    b.add_mesh(_quad(S, [(-8, 2, 2), (6, 2, 5), (7, 9, 9), (-7, 9, 6)], (0, 30, -20)), gold)
    b.add_mesh(_quad(S, [(-6, 29.5, -6), (-6, 29.5, 6), (6, 29.5, 6), (6, 29.5, -6)], mid),
               b.material("light", S._mat(S.ROUGH_CONDUCTOR, emission=(20, 18, 15))))
    cam = S.make_camera(width, height, 70, (3, 12, -17), (-2, 8, 6))
    return b.finish(camera=cam, rr_rate=0.9, spp=8, background=np.float32([0.05, 0.05, 0.08]), name="conductor box")


def _scene(hip, sd, monkeypatch, share, env=None, library=None):
    for k in ("MCPT_SHARE_RAYS", "MCPT_OVERLAP", "MCPT_QUEUE_AHEAD"):
        monkeypatch.delenv(k, raising=False)
    if not share:
        monkeypatch.setenv("MCPT_SHARE_RAYS", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    hs = hip.HipScene(sd, library=library)  # (the knobs are read once, when the scene is created)
    for k in ("MCPT_SHARE_RAYS", "MCPT_OVERLAP", "MCPT_QUEUE_AHEAD"):
        monkeypatch.delenv(k, raising=False)
    return hs


def _counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


def _on_off(hip, sd, monkeypatch, traced_primary=None, **kw):
    """Renders sd with the sharing off and on; asserts the identity of frames and counters and that the two ray counts add up to the
    continuation rays of mcpt_stats.  Returns (frame, Stats, traced, shared) of the run with the sharing on."""
    hs = _scene(hip, sd, monkeypatch, False)
    off, s_off = hs.render(**kw)
    t_off, sh_off = hs.ray_counts()
    hs.close()
    hs = _scene(hip, sd, monkeypatch, True)
    on, s_on = hs.render(**kw)
    traced, shared = hs.ray_counts()
    hs.close()
    print("\n[share] %s %s: %d continuation rays traced, %d shared (%.1f %%); sharing off: %d traced"
          % (sd.name, kw, traced, shared, 100.0 * shared / max(traced + shared, 1), t_off))
    assert np.array_equal(off, on, equal_nan=True), int((~_same_bits(off, on)).sum())
    assert _counters(s_on) == _counters(s_off), list(zip(COUNTERS, _counters(s_on), _counters(s_off)))
    assert s_on.iterations == s_off.iterations
    assert sh_off == 0 and t_off == traced + shared
    if traced_primary is not None:
        assert traced + shared == s_on.closest_rays - traced_primary
    return on, s_on, traced, shared


@pytest.fixture(scope="module")
def box48(pkg):
    return conductor_box(pkg, 48, 32)


@pytest.fixture(scope="module")
def box_reference(hip, box48):
    """The conductor box with the sharing off, default schedule: what every variant below must reproduce."""
    os.environ["MCPT_SHARE_RAYS"] = "0"
    try:
        hs = hip.HipScene(box48)
    finally:
        del os.environ["MCPT_SHARE_RAYS"]
    fb, st = hs.render(spp=8, seed=5, spp_per_pass=8)
    assert hs.ray_counts()[1] == 0
    hs.close()
    fb.setflags(write=False)
    return fb, _counters(st)


def test_on_off_identity_mirror_floor(pkg, hip, monkeypatch):
    sd = floor_scene(pkg, 48, 32)
    fb, st, traced, shared = _on_off(hip, sd, monkeypatch, traced_primary=48 * 32 * 8, spp=8, seed=3)
    assert st.samples == 48 * 32 * 8 and shared > 0
    assert np.isfinite(fb).all() and (fb > 0).any()  # (the sky's reflection, where roulette let a sample through)


def test_on_off_identity_chess(pkg, hip, monkeypatch):
    sd = pkg.scenes.chess_scene(width=96, height=54, spp=8)
    _, st, traced, shared = _on_off(hip, sd, monkeypatch, spp=8, seed=2)
    assert shared > 0 and traced > 0


def test_on_off_identity_conductor_box(pkg, hip, monkeypatch, box48, box_reference):
    fb, st, traced, shared = _on_off(hip, box48, monkeypatch, traced_primary=48 * 32 * 8, spp=8, seed=5, spp_per_pass=8)
    assert np.array_equal(fb, box_reference[0], equal_nan=True) and _counters(st) == box_reference[1]
    # deep sibling chains: far more vertices than first vertices (1 / (1 - 0.9) = 10 per path that never meets the emitter)
    assert st.vertices > 4 * st.paths and shared > 0


def test_on_off_identity_material_zoo(pkg, hip, monkeypatch):
    sd, _ = zoo.zoo_scene_full(96, 64, 4)
    _on_off(hip, sd, monkeypatch, spp=4, seed=1, spp_per_pass=3)


@pytest.mark.parametrize("name", ["mirror_floor", "conductor_box"])
def test_oracle_parity(pkg, oracle, hip, monkeypatch, tree_env, name, box48):
    """Renderer::Render with the reference's tree: the oracle's frame bit for bit, and its counters."""
    sd = floor_scene(pkg, 48, 32) if name == "mirror_floor" else box48
    tree_env("reference", "0")
    fb_ref, st_ref = oracle.OracleScene(sd).render(spp=8, seed=5)
    hs = _scene(hip, sd, monkeypatch, True)
    fb, st = hs.render(spp=8, seed=5, spp_per_pass=3)
    traced, shared = hs.ray_counts()
    hs.close()
    bad = ~_same_bits(fb_ref, fb)
    assert not bad.any(), "%d of %d framebuffer values differ" % (bad.sum(), bad.size)
    # (without an emitter the reference's directLighting finds no light to sample and casts no shadow ray, while ref_scene_rays
    # counts n_dir per shaded vertex whatever the scene: the floor's count is compared without that term)
    no_light = 0 if name == "conductor_box" else int(sd.n_dir_sample) * int(st.shaded)
    assert st.vertices == st_ref.vertices and st.ref_scene_rays - no_light == st_ref.scene_rays
    assert shared > 0


@pytest.mark.parametrize("variant", ["small_pool", "one_stream", "no_queue_ahead", "pass_4", "two_ranks"])
def test_schedule_variants(pkg, hip, monkeypatch, box48, box_reference, variant):
    """The frame and the counters do not depend on the schedule; how many records share a ray may."""
    ref, ref_counters = box_reference
    env, kw = {"small_pool": ({}, dict(pool_paths=3 * 4096)), "one_stream": ({"MCPT_OVERLAP": "0"}, {}),
               "no_queue_ahead": ({"MCPT_QUEUE_AHEAD": "0"}, {}), "pass_4": ({}, dict(spp_per_pass=4)), "two_ranks": ({}, {})}[variant]
    kw = dict(dict(spp=8, seed=5, spp_per_pass=8), **kw)
    hs = _scene(hip, box48, monkeypatch, True, env=env)
    if variant == "two_ranks":
        parts = [hs.render(tile_size=16, rank=r, nranks=2, **kw) for r in range(2)]
        fb = parts[0][0] + parts[1][0]
        assert not ((parts[0][0] != 0) & (parts[1][0] != 0)).any()
        counters = tuple(a + b for a, b in zip(_counters(parts[0][1]), _counters(parts[1][1])))
    else:
        fb, st = hs.render(**kw)
        counters = _counters(st)
    traced, shared = hs.ray_counts()
    hs.close()
    print("\n[share] conductor box, %s: %d traced, %d shared" % (variant, traced, shared))
    assert np.array_equal(ref, fb, equal_nan=True), int((~_same_bits(ref, fb)).sum())
    assert counters == ref_counters, list(zip(COUNTERS, counters, ref_counters))
    assert shared > 0


@pytest.mark.parametrize("rr", [0.4, 0.9])
def test_sharing_happens_on_a_mirror_floor(pkg, hip, monkeypatch, rr):
    """Every first vertex lies on the floor and sends 3 r records on, 1 - (1 - r)^3 of them on a ray of their own: the shared
    fraction of the records is 1 - (1 - (1 - r)^3) / (3 r).  At most one fresh triple in 21 is cut by a wave boundary (lanes 3k + c
    of 64-lane waves: <= 5 %); the rest of the margin is sampling noise over 49 152 samples."""
    W, H, spp = 64, 48, 16
    sd = floor_scene(pkg, W, H, rr_rate=rr)
    monkeypatch.setenv("MCPT_SKY_CULL", "0")  # (every sample is traced, whatever the cull would decide: primaries = W H spp)
    hs = _scene(hip, sd, monkeypatch, True)
    fb, st = hs.render(spp=spp, seed=7)
    traced, shared = hs.ray_counts()
    hs.close()
    expect = 1.0 - (1.0 - (1.0 - rr) ** 3) / (3.0 * rr)
    print("\n[share] mirror floor rr %.1f: %d traced, %d shared: %.4f of the records (expected %.4f, bound %.4f)"
          % (rr, traced, shared, shared / (traced + shared), expect, 0.85 * expect))
    assert st.samples == W * H * spp
    assert traced + shared == st.closest_rays - W * H * spp
    assert shared / (traced + shared) >= 0.85 * expect
    hs = _scene(hip, sd, monkeypatch, False)
    fb_off, st_off = hs.render(spp=spp, seed=7)
    t_off, s_off = hs.ray_counts()
    hs.close()
    assert s_off == 0 and t_off == traced + shared
    assert np.array_equal(fb, fb_off, equal_nan=True)


def test_explicit_paths_share_nothing(pkg, oracle, hip, monkeypatch, tree_env, box48):
    """mcpt_cast_rays: one ray per record, so no two records ever read one ray; the path values are the oracle's, knob on or off."""
    sd = box48
    os_ = oracle.OracleScene(sd)
    rng = np.random.default_rng(23)
    n = 6000
    pix = np.repeat(rng.integers(0, 48 * 32, size=n // 3), 3).astype(np.uint32)  # the three channel paths of a sample, side by side
    smp = np.repeat(rng.integers(0, 1000, size=n // 3), 3).astype(np.uint32)
    ch = np.tile(np.arange(3), n // 3).astype(np.int32)
    o, d = os_.camera_rays(pix, smp, seed=9)
    ref = os_.cast_rays(o, d, pix, smp, ch, seed=9)
    tree_env("reference", "0")
    values = []
    for share in (False, True):
        hs = _scene(hip, sd, monkeypatch, share)
        values.append(hs.cast_rays(o, d, pix, smp, ch, seed=9))
        traced, shared = hs.ray_counts()
        hs.close()
        assert shared == 0 and traced > n
    assert _same_bits(values[0], values[1]).all()
    bad = ~_same_bits(ref, values[1])
    assert not bad.any(), "%d of %d paths differ from the oracle" % (bad.sum(), n)
