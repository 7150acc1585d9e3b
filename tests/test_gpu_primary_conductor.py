"""First hits on smooth conductors finished inside the primary-ray kernel (primary_sample in csrc/mcpt_kernels.hip, DESIGN.md section 6;
MCPT_PRIMARY_CONDUCTOR=0 switches it off).  Nothing may change but which kernel does the work: frames are equal bit for bit, NaN
positions included, with the switch on and off, and so is every work counter of mcpt_stats (samples, paths, vertices, shaded,
closest_rays, shadow_rays, direct_vertices, ref_scene_rays, overflow_paths; the iteration count is printed: paths that end in the
primary kernel leave the loop an iteration earlier, and the kernel times and launch counts follow the schedule).  The scene is created
afresh for every switch value (the knobs are read once per scene); the pools are small, so that a render takes ten or more iterations.

The ring-wrap case needs the MCPT_RING_START hook, which the product library does not have, and the short path, which the checking build
does not have: it runs in the hooks build (build.build_hooks: the test hooks and the forced retry flavour with four stack entries,
without the direct-lighting-skip check).  The same build runs the retry case, where most reflected rays lose a stack entry.

`iterations` is the one field of mcpt_stats left out of the comparison, on purpose: a path that ends in the primary kernel leaves the loop
an iteration earlier, so the count falls with the switch on; it is printed."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import material_zoo as zoo  # noqa: E402
import mirror_scene as ms  # noqa: E402
from chain_scene import chain_scene  # noqa: E402
from conftest import TREES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_hooks(pkg, hip):
    """Path of the hooks build (libmcpt_hip_hooks.so: -DMCPT_TEST_HOOKS -DMCPT_FORCE_RETRY -DMCPT_STK_RETRY=4, short path compiled in)."""
    path = pkg.build.build_hooks()
    assert os.path.exists(path)
    return path

COUNTERS = ("samples", "paths", "vertices", "shaded", "closest_rays", "shadow_rays", "direct_vertices", "ref_scene_rays", "overflow_paths")
KNOB = "MCPT_PRIMARY_CONDUCTOR"
SMALL_POOL = 3 * 1024


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


def _scene(hip, sd, monkeypatch, on, library=None):
    monkeypatch.delenv(KNOB, raising=False)
    if not on:
        monkeypatch.setenv(KNOB, "0")
    hs = hip.HipScene(sd, library=library)
    monkeypatch.delenv(KNOB, raising=False)
    return hs


def _quad(S, corners, towards):
    a, b, c, d = [np.asarray(p, np.float64) for p in corners]
    if np.dot(np.cross(b - a, c - a), np.asarray(towards, np.float64) - a) < 0:
        b, d = d, b
    t = np.zeros(2, S.TRI_DTYPE)
    t[0]["v0"], t[0]["v1"], t[0]["v2"] = a, b, c
    t[1]["v0"], t[1]["v1"], t[1]["v2"] = a, c, d
    return t


def floor_only(pkg, width, height, rr_rate=0.4, eye=(0, 30, -5), target=(0, 0, 0), fov=50, light=None):
    """A silver-mirror floor (normal +y) that fills the view under a constant sky; `light`: (half size, height) of a quad emitter above
    the origin, facing down."""
    S = pkg.scenes
    b = S._Builder()
    b.add_mesh(_quad(S, [(-500, 0, -500), (-500, 0, 500), (500, 0, 500), (500, 0, -500)], (0, 1, 0)),
               b.material("silver_mirror", S.material_presets()["silver_mirror"]))
    if light is not None:
        e, y = light
        b.add_mesh(_quad(S, [(-e, y, -e), (-e, y, e), (e, y, e), (e, y, -e)], (0, 0, 0)),
                   b.material("light", S._mat(S.ROUGH_CONDUCTOR, emission=(20, 18, 15))))
    cam = S.make_camera(width, height, fov, eye, target, (0, 0, 1) if eye[0] == target[0] and eye[2] == target[2] else (0, 1, 0))
    return b.finish(camera=cam, rr_rate=rr_rate, spp=8, background=np.float32([0.3, 0.5, 0.8]), name="mirror floor")


def mirrors(pkg, emitter):
    """The scene of tests/mirror_scene.py; emitter False: the same without its light."""
    sd = ms.mirror_scene(pkg)
    if emitter:
        return sd
    S = pkg.scenes
    P = S.material_presets()
    b = S._Builder()
    b.add_mesh(ms._quad(S, (-20, 0, -20), (20, 0, -20), (20, 0, 20), (-20, 0, 20)), b.material("floor", P["silver_mirror"]))
    b.add_mesh(ms._box(S, (-10, 0, 2), (10, 24, 12)), b.material("box", S._mat(S.ROUGH_CONDUCTOR, 0.4, (0.6, 0.25, 0.8))))
    b.add_mesh(ms._quad(S, (-20, 0, 16), (20, 0, 16), (20, 24, 16), (-20, 24, 16)), b.material("back", S._mat(S.SMOOTH_CONDUCTOR, 0.001, (0.9, 0.9, 0.8))))
    b.add_sphere((-9, 3, -2), 3, b.material("mirror_sphere", P["silver_mirror"]))
    b.add_sphere((6, 3, -4), 3, b.material("glass", P["smooth_glass"]))
    return b.finish(camera=ms.camera(pkg), spp=ms.SPP, name="mirrors, no light", background=np.array([0.25, 0.3, 0.4], np.float32))


def chess(pkg, width, height, dof=True):
    S = pkg.scenes
    conf = json.loads(json.dumps(S.DEFAULT_CONF))
    conf["camera"]["useDOF"] = bool(dof)
    return S.chess_scene(conf, width=width, height=height, spp=8)


def deep_mirror_chain(pkg):
    """The 36-level chain of the cull tests as mirrors, seen from the side their normals point to: with the GPU-built tree the kernels run
    the retry flavour of the traversal stack, for the camera rays and for the reflected rays."""
    S = pkg.scenes
    sd = chain_scene(pkg, 36)
    mats = sd.materials.copy()
    mats[0] = np.asarray(S.material_presets()["silver_mirror"]).astype(S.MAT_DTYPE).reshape(())
    cam = S.make_camera(48, 32, 40, (0.3, 0.6, 40.0), (0.0, 0.0, 0.0))
    return S.SceneData(triangles=sd.triangles, materials=mats, objects=sd.objects, background=np.float32([0.3, 0.5, 0.8]), env_pixels=None,
                       camera=cam, rr_rate=0.6)


def _on_off(hip, sd, monkeypatch, render=None, library=None, **kw):
    """Renders sd with the switch off and on (a fresh scene each); asserts that frames and counters are identical.  Returns
    (frame, Stats, (samples, rays) of the short path, (traced, shared)) of the run with the switch on."""
    render = render or (lambda hs: hs.render(**kw))
    out = {}
    for on in (False, True):
        hs = _scene(hip, sd, monkeypatch, on, library=library)
        fb, st = render(hs)
        out[on] = (fb, st, hs.primary_conductor_counts(), hs.ray_counts())
        hs.close()
    (off, s_off, pc_off, rc_off), (on_, s_on, pc_on, rc_on) = out[False], out[True]
    print("\n[primary conductor] %s %s: %d of %d samples on the short path, %d reflected rays traced there; iterations %d (off: %d)"
          % (getattr(sd, "name", "scene"), kw, pc_on[0], s_on.samples, pc_on[1], s_on.iterations, s_off.iterations))
    bad = ~_same_bits(off, on_)
    assert not bad.any(), "%d of %d framebuffer values differ" % (bad.sum(), bad.size)
    assert _counters(s_on) == _counters(s_off), list(zip(COUNTERS, _counters(s_on), _counters(s_off)))
    assert pc_off == (0, 0)
    assert sum(rc_on) == sum(rc_off)  # resolved continuation rays
    return on_, s_on, pc_on, rc_on


# ------------------------------------------------------------------------------------------------ 1. switch on equals switch off
def _case(pkg, name):
    S = pkg.scenes
    if name == "mirrors_emitter":
        return mirrors(pkg, True), dict(spp=8, seed=3, pool_paths=SMALL_POOL)
    if name == "mirrors_no_emitter":
        return mirrors(pkg, False), dict(spp=8, seed=3, pool_paths=SMALL_POOL)
    if name in ("chess_dof", "chess_pinhole"):
        return chess(pkg, 96, 54, dof=name == "chess_dof"), dict(spp=8, seed=2, pool_paths=2 * SMALL_POOL)
    if name == "cornell_demo":
        return S.cornell_demo(64, 64, 8), dict(spp=8, seed=4, pool_paths=SMALL_POOL)
    if name == "zoo_full":
        return zoo.zoo_scene_full(96, 64, 8)[0], dict(spp=8, seed=1, spp_per_pass=3, pool_paths=2 * SMALL_POOL)
    if name == "zoo_small":
        return zoo.zoo_scene_small(96, 64, 8)[0], dict(spp=8, seed=1, pool_paths=2 * SMALL_POOL)
    if name in ("roulette_0.4", "roulette_0.9"):
        return floor_only(pkg, 48, 32, rr_rate=float(name[-3:])), dict(spp=8, seed=3, pool_paths=SMALL_POOL)
    if name == "pass_of_3":
        return mirrors(pkg, True), dict(spp=8, seed=5, spp_per_pass=3, pool_paths=SMALL_POOL)
    if name == "rank_1_of_2":
        return mirrors(pkg, True), dict(spp=8, seed=5, tile_size=16, rank=1, nranks=2, pool_paths=SMALL_POOL)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["mirrors_emitter", "mirrors_no_emitter", "chess_dof", "chess_pinhole", "cornell_demo", "zoo_full", "zoo_small",
                                  "roulette_0.4", "roulette_0.9", "pass_of_3", "rank_1_of_2"])
def test_on_off_identity(pkg, hip, monkeypatch, name):
    sd, kw = _case(pkg, name)
    _, st, pc, _ = _on_off(hip, sd, monkeypatch, **kw)
    assert st.iterations >= 10
    assert pc[0] > 0  # (every one of these scenes shows a mirror whose reflection is dark)


def test_on_off_identity_progressive(pkg, hip, monkeypatch):
    """Two calls that add up to one frame: sample_offset / accumulate."""
    sd = mirrors(pkg, True)

    def two_calls(hs):
        fb, st1 = hs.render(spp=4, spp_total=8, seed=6, pool_paths=SMALL_POOL)
        fb, st2 = hs.render(spp=4, spp_total=8, sample_offset=4, accumulate=1, seed=6, fb=fb, pool_paths=SMALL_POOL)
        return fb, st2
    fb, _, pc, _ = _on_off(hip, sd, monkeypatch, render=two_calls)
    assert pc[0] > 0
    hs = _scene(hip, sd, monkeypatch, True)
    whole, _ = hs.render(spp=8, seed=6, spp_per_pass=4, pool_paths=SMALL_POOL)
    hs.close()
    assert _same_bits(whole, fb).all()


@pytest.mark.parametrize("bvh,quant", TREES)
def test_on_off_identity_trees(pkg, hip, monkeypatch, tree_env, bvh, quant):
    tree_env(bvh, quant)
    _, _, pc, _ = _on_off(hip, mirrors(pkg, True), monkeypatch, spp=8, seed=3, pool_paths=SMALL_POOL)
    assert pc[0] > 0


def test_on_off_identity_retry_flavour(pkg, hip, monkeypatch, tree_env):
    tree_env("lbvh", None)
    sd = deep_mirror_chain(pkg)
    hs = hip.HipScene(sd)
    height = hs.info()["bvh_height"]
    hs.close()
    assert height > 24, height  # deeper than the plain stack classes: the retry flavour
    _, st, pc, _ = _on_off(hip, sd, monkeypatch, spp=8, seed=3, pool_paths=SMALL_POOL)
    assert pc[0] > 0 and st.vertices > st.paths


def test_on_off_identity_forced_retry(pkg, hip, hip_hooks, monkeypatch):
    """The hooks build walks every tree with the retry flavour and four stack entries, so that most rays, camera rays and reflected rays
    alike, lose an entry and their samples are done again by k_primary_retrace.  The frame is the product library's."""
    sd = mirrors(pkg, True)
    hs = _scene(hip, sd, monkeypatch, True)
    ref, st0 = hs.render(spp=8, seed=3, pool_paths=SMALL_POOL)
    pc0 = hs.primary_conductor_counts()
    hs.close()
    fb, st, pc, _ = _on_off(hip, sd, monkeypatch, library=hip_hooks, spp=8, seed=3, pool_paths=SMALL_POOL)
    assert _same_bits(ref, fb).all() and _counters(st) == _counters(st0)
    assert pc == pc0 and pc[0] > 0  # a sample that the retrace kernel finishes is counted once


def test_on_off_identity_ring_wrap(pkg, hip, hip_hooks, monkeypatch):
    """The free ring's counters wrap in the middle of the run, with the short path popping its slots (hooks build: see the module's docstring)."""
    sd = mirrors(pkg, True)
    hs = _scene(hip, sd, monkeypatch, True)
    ref, st0 = hs.render(spp=8, seed=3, pool_paths=SMALL_POOL)
    hs.close()
    monkeypatch.setenv("MCPT_RING_START", "0xfffff800")
    fb, st, pc, _ = _on_off(hip, sd, monkeypatch, library=hip_hooks, spp=8, seed=3, pool_paths=SMALL_POOL)
    monkeypatch.delenv("MCPT_RING_START")
    assert _same_bits(ref, fb).all() and _counters(st) == _counters(st0)
    assert pc[0] > 0 and st.vertices > st.paths  # records were handed on: slots were popped on both sides of the wrap


# ------------------------------------------------------------------------------------------------ 2. the oracle's frame
@pytest.mark.parametrize("name", ["mirror_floor", "chess"])
def test_oracle_parity(pkg, oracle, hip, monkeypatch, tree_env, name):
    sd = floor_only(pkg, 48, 32) if name == "mirror_floor" else chess(pkg, 64, 40)
    tree_env("reference", "0")
    fb_ref, st_ref = oracle.OracleScene(sd).render(spp=8, seed=5)
    hs = _scene(hip, sd, monkeypatch, True)
    fb, st = hs.render(spp=8, seed=5, spp_per_pass=3, pool_paths=SMALL_POOL)
    pc = hs.primary_conductor_counts()
    hs.close()
    bad = ~_same_bits(fb_ref, fb)
    assert not bad.any(), "%d of %d framebuffer values differ" % (bad.sum(), bad.size)
    assert st.vertices == st_ref.vertices and pc[0] > 0


# ------------------------------------------------------------------------------------------------ 3. fallbacks
def test_fallback_mirror_under_a_light(pkg, hip, monkeypatch):
    """The camera looks straight down from under a small emitter: every mirror direction points into the emitters' cone, direct_is_zero is
    false at every first hit and no sample takes the short path."""
    monkeypatch.setenv("MCPT_SKY_CULL", "0")
    sd = floor_only(pkg, 48, 32, eye=(0.2, 8, 0.1), target=(0.2, 0, 0.1), fov=6, light=(1.5, 10.0))
    _, st, pc, _ = _on_off(hip, sd, monkeypatch, spp=8, seed=3, pool_paths=SMALL_POOL)
    first_hits = 48 * 32 * 8  # every camera ray meets the floor
    assert st.samples == first_hits and st.shaded >= 3 * first_hits
    assert st.direct_vertices >= 3 * first_hits  # ... and its light samples are evaluated
    assert pc[0] == 0 < first_hits


def test_fallback_camera_below_the_floor(pkg, hip, monkeypatch):
    """Seen from below (wo.n < 0) the floor is met from inside: the ordinary path."""
    monkeypatch.setenv("MCPT_SKY_CULL", "0")
    sd = floor_only(pkg, 48, 32, eye=(0, -30, -5), target=(0, 0, 0))
    _, st, pc, _ = _on_off(hip, sd, monkeypatch, spp=8, seed=3, pool_paths=SMALL_POOL)
    first_hits = 48 * 32 * 8
    assert st.samples == first_hits and st.shaded == 3 * first_hits
    assert pc[0] < first_hits and pc[0] == 0


# ------------------------------------------------------------------------------------------------ 4. the path is taken
@pytest.mark.parametrize("rr", [0.4, 0.9])
def test_every_sample_of_a_mirror_floor_is_finished_in_the_primary_kernel(pkg, hip, monkeypatch, rr):
    monkeypatch.setenv("MCPT_SKY_CULL", "0")
    W, H, spp = 64, 48, 16
    sd = floor_only(pkg, W, H, rr_rate=rr)
    fb, st, pc, (traced, shared) = _on_off(hip, sd, monkeypatch, spp=spp, seed=7, pool_paths=4 * SMALL_POOL)
    assert st.samples == W * H * spp
    assert 3 * pc[0] == st.shaded and pc[0] == st.samples
    assert traced - pc[1] == 0  # the closest-hit queue kernel walked nothing: no record was ever created
    assert traced + shared == st.closest_rays - W * H * spp and shared > 0
    assert st.vertices == st.paths  # nothing was pushed: every path ended at its first vertex or in the sky
    assert np.isfinite(fb).all() and (fb > 0).any()


# ------------------------------------------------------------------------------------------------ 5. other entry points
def test_cast_rays_and_adaptive(pkg, hip, monkeypatch):
    sd = mirrors(pkg, True)
    rng = np.random.default_rng(11)
    n = 3000
    pix = np.repeat(rng.integers(0, ms.W * ms.H, size=n // 3), 3).astype(np.uint32)
    smp = np.repeat(rng.integers(0, 1000, size=n // 3), 3).astype(np.uint32)
    ch = np.tile(np.arange(3), n // 3).astype(np.int32)
    res = {}
    for on in (False, True):
        hs = _scene(hip, sd, monkeypatch, on)
        o, d = hs.camera_rays(pix, smp, seed=9)
        res[on] = (hs.cast_rays(o, d, pix, smp, ch, seed=9), hs.primary_conductor_counts(), hs.render_adaptive(4, 0.02, spp=16, seed=8, pool_paths=SMALL_POOL))
        hs.close()
    assert _same_bits(res[False][0], res[True][0]).all()
    assert res[True][1] == (0, 0)  # explicit paths bring their own rays: there is no primary kernel
    (fb0, spp0, err0, _, st0), (fb1, spp1, err1, _, st1) = res[False][2], res[True][2]
    assert _same_bits(fb0, fb1).all() and np.array_equal(spp0, spp1) and _same_bits(err0, err1).all()
    assert _counters(st0) == _counters(st1)
