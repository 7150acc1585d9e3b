"""mcpt_render_probe_lit on the GPU: frames lit by a baked probe volume.

Expected frames are compositions of calls that exist without the feature (tests/probe_lit_cases.py): centre_rays / camera_rays,
intersect, p = o + d * (float)t in numpy float32, the AOV record (or the material table and query_closest's normal), the host forms of
the two grid lookups, cast_rays for the sky and the emitters.  Device bits are compared with them.  Frames are 32 x 24 with centre rays
and 37 x 23 (851 pixels: a ragged last wave) with jittered rays at aov_spp 3; volumes are 3 x 2 x 3 probes baked at 64 spp with 64 depth
samples.  Device buffers are made without torch and every output sits between two runs of 64 guard elements that must survive.  torch
and a non-default stream: tests/probe_lit_torch_child.py, a child process."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirror_scene as ms  # noqa: E402
import probe_depth_cases as pdc  # noqa: E402
import probe_lit_cases as plc  # noqa: E402
from add_cases import extend_numpy, split  # noqa: E402
from chain_scene import chain_scene  # noqa: E402
from deform_cases import PLASTIC_SPHERE, SHORT, deformed_scene, object_positions, translate, wave  # noqa: E402
from material_edit_cases import LEFT, edited_scene, emits, env_map, with_fields  # noqa: E402
from ray_query_cases import Rays, closest, scene_extent  # noqa: E402
from sensor_query_cases import SENTINEL, same_bits  # noqa: E402
from visibility_cases import mask_hiding  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 32, 24
WJ, HJ, SPPJ = 37, 23, 3
NAMES = ["sah", "lbvh", "ploc", "chess", "chain", "env", "dim"]
DIM = (0.7, 0.5, 0.3)  # an emission below 1: emit * |cos| never reaches the clamp, so the cosine is in the value


def assert_equal(got, want, what=""):
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: got %r, want %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], np.asarray(got)[bad][0], np.asarray(want)[bad][0])


def cornell_camera(pkg, w, h):
    """From below and in front of the box's opening up into the room: the ceiling light spans 2.2 degrees of elevation, more than the 1.7
    degrees between the rows of a 24-row frame (from the demo camera it is thinner than one row), the boxes and spheres are in view, and
    the columns at the sides look past the box at the sky (half-width 349 at the opening, the box's is 278)."""
    return pkg.scenes.make_camera(w, h, 40, (278, 150, -700), (278, 420, 300))


def dimmed(sd):
    """The description with every emitter's emission replaced by DIM."""
    mats = sd.materials.copy()
    for i in np.flatnonzero(emits(mats)):
        mats[i] = with_fields(mats[i], emission=DIM)
    return dataclasses.replace(sd, materials=mats)


def make_scene(pkg, name):
    """(description with its camera at the test's size, creation keywords, grid, max_distance) of a named case."""
    S = pkg.scenes
    if name == "chess":
        sd = S.chess_scene(width=48, height=27, spp=4)
        kw = dict(builder="sah", quantise=1)
    elif name == "chain":
        sd = chain_scene(pkg, 40)
        sd = dataclasses.replace(sd, camera=S.make_camera(W, H, 60, (-0.4, -0.6, -4.0), (-0.5, -0.5, 0.0)))
        return sd, dict(builder="lbvh"), ((-2.0, -2.0, -2.0), (2.0, 4.0, 2.0), (3, 2, 3)), 3.0
    elif name == "env":
        sd = dataclasses.replace(S.cornell_demo(W, H, 4), env_pixels=env_map(16, 8, seed=3), camera=cornell_camera(pkg, W, H))
        kw = dict(builder="sah")
    elif name == "rc":
        sd = dataclasses.replace(S.cornell_rc(WJ, HJ, 4), camera=cornell_camera(pkg, WJ, HJ))
        kw = dict(builder="sah")
    elif name == "dim":
        sd = dimmed(dataclasses.replace(S.cornell_demo(W, H, 4), camera=cornell_camera(pkg, W, H)))
        kw = dict(builder="sah")
    elif name == "mirrors":  # (with a dim light, so that the emitter seen in the mirrors is not the clamp's 1)
        sd = dimmed(ms.mirror_scene(pkg, W, H))
        return sd, dict(builder="sah"), ((-16.0, 2.0, -16.0), (16.0, 20.0, 14.0), (3, 2, 3)), 20.0
    else:
        sd = dataclasses.replace(S.cornell_demo(W, H, 4), camera=cornell_camera(pkg, W, H))
        kw = dict(builder=name)
    return sd, kw, plc.scene_grid(sd), float(f32(0.3 * scene_extent(sd)))


class Case:
    def __init__(self, pkg, hip, name):
        self.name = name
        self.sd, self.kw, self.grid, self.md = make_scene(pkg, name)
        self.hs = hip.HipScene(self.sd, **self.kw)
        self.vol = plc.Volume(self.hs, self.grid, 64, 64, self.md, normal_bias=float(f32(0.01 * self.md)))
        self.cam = self.sd.camera
        self._want = {}

    def want(self, hip, visible):
        """The restated centre frame at depth 0, made once per lookup."""
        if visible not in self._want:
            aov = self.hs.render_aovs(centre=True, camera=self.cam)
            self._want[visible] = plc.restate_depth0(self.hs, hip, self.sd, self.vol, visible, self.cam, aov=aov)
            self._want[visible]["aov"] = aov
        return self._want[visible]


@pytest.fixture(scope="module")
def cases(pkg, hip):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(pkg, hip, name)
        return made[name]

    yield get
    for c in made.values():
        c.hs.close()


# ---------------------------------------------------------------- 1. depth 0, centre rays
@pytest.mark.parametrize("visible", [True, False], ids=["visible", "plain"])
@pytest.mark.parametrize("name", NAMES)
def test_centre_frame_equals_the_restatement(hip, cases, name, visible):
    c = cases(name)
    if name in ("sah", "lbvh", "ploc"):
        assert c.hs.info()["lds_resident"] == 1
    if name == "chain":
        assert c.hs.info()["bvh_height"] > 24  # deeper than every LDS stack: the retry flavour and its retrace list
    want = c.want(hip, visible)
    kind = want["kind"][..., 0]
    Hc, Wc = kind.shape
    lit, pos, info = plc.lit_frame(c.hs, c.vol, visible, centre=True, camera=c.cam)
    n_s, n_e, n_m = (int((kind == k).sum()) for k in (plc.SURFACE, plc.EMITTER, plc.MISS))
    print("\n[probe lit] %s, %s: %d x %d, %d surface, %d emitter, %d sky pixels; %d chunk(s), workspace %d, %.3g ms"
          % (name, "visible" if visible else "plain", Wc, Hc, n_s, n_e, n_m, info["chunks"], info["in_workspace"], info["ms_total"]))
    assert n_s > 0.2 * kind.size
    if name in ("sah", "lbvh", "ploc", "env", "dim"):
        assert n_e > 0  # the Cornell light is in view
    if name in ("env", "chess", "chain"):
        assert n_m > 0
    assert_equal(lit, want["lit"], "%s: lit" % name)
    assert_equal(pos, want["position"], "%s: position" % name)
    assert not pos[kind == plc.MISS].any()
    assert info["samples"] == Wc * Hc and info["lookups"] == want["lookups"] == n_s
    # without a position buffer the frame is the same
    lit2, none, _ = plc.lit_frame(c.hs, c.vol, visible, position=False, centre=True, camera=c.cam)
    assert none is None
    assert_equal(lit2, lit, "%s: without position" % name)
    if name == "dim":  # below the clamp: emission x |cos|, which differs from row to row of the light
        em = lit[kind == plc.EMITTER]
        assert (em > 0).all() and (em < f32(DIM)).all() and len(np.unique(em[:, 0])) > 1
    if name == "env":  # the map is in the frame, not the constant background
        sky = lit[kind == plc.MISS]
        assert len(np.unique(sky.round(4), axis=0)) > 4


def test_the_two_lookups_differ(hip, cases):
    """The premise of running every case twice: on the Cornell scene the occlusion-aware frame is not the plain one."""
    c = cases("sah")
    a, b = c.want(hip, True)["lit"], c.want(hip, False)["lit"]
    assert (a != b).any(axis=2).mean() > 0.2


# ---------------------------------------------------------------- 2. jittered rays, three samples per pixel
@pytest.mark.parametrize("visible", [True, False], ids=["visible", "plain"])
def test_jittered_frame_equals_the_fold(hip, cases, visible):
    c = cases("rc")
    want = plc.restate_depth0(c.hs, hip, c.sd, c.vol, visible, c.cam, centre=False, spp=SPPJ, seed=7)
    lit, pos, info = plc.lit_frame(c.hs, c.vol, visible, aov_spp=SPPJ, seed=7, camera=c.cam)
    kind = want["kind"]
    mixed = ((kind != kind[..., :1]).any(axis=2)).sum()
    print("\n[probe lit] jittered %d x %d x %d: %d pixels whose samples end differently" % (WJ, HJ, SPPJ, int(mixed)))
    assert mixed > 0 and (kind == plc.MISS).any() and (kind == plc.EMITTER).any()
    assert_equal(lit, want["lit"], "jittered lit")
    assert_equal(pos, want["position"], "jittered position")
    assert info["samples"] == WJ * HJ * SPPJ and info["lookups"] == want["lookups"]
    other, _, _ = plc.lit_frame(c.hs, c.vol, visible, aov_spp=SPPJ, seed=8, camera=c.cam, position=False)
    assert (other != lit).any()  # the seed is read
    # aov_spp 0 is one sample
    one, _, i1 = plc.lit_frame(c.hs, c.vol, visible, aov_spp=1, seed=7, camera=c.cam, position=False)
    zero, _, i0 = plc.lit_frame(c.hs, c.vol, visible, aov_spp=0, seed=7, camera=c.cam, position=False)
    assert_equal(zero, one, "aov_spp 0")
    assert i0["samples"] == i1["samples"] == WJ * HJ


# ---------------------------------------------------------------- 3. chains
# The largest deviations measured on an MI355X on this scene (the larger of depth 1 and 2), of which the test allows four times as much:
# float32 reflection of a direction through two bounces has no tighter derivable bound.
POSITION_DEV = 1.92e-6  # |position - float64 terminal point|, scene units (the scene spans 40: half a float32 ulp at 32)
EMITTER_DEV = 3.37e-8   # |lit - float64 emitter rule| = throughput x emission (0.7, 0.5, 0.3) x |cos|, all below the clamp


@pytest.mark.parametrize("depth", [1, 2])
def test_chains(hip, oracle, cases, depth):
    """Centre rays through the mirrors of tests/mirror_scene.py.  Bit for bit: non-emitter terminal hits against albedo x lookup of the
    frame's own position output with the chain AOV's albedo and normal, terminal misses against albedo x background, depth 0 against
    case 1's frame.  Against the float64 walk of tests/probe_lit_cases.py, within four times the measured deviation: position
    (measured 1.92e-6 in a scene that spans 40) and the emitters seen in a mirror, whose emission stays below the clamp so that
    throughput x emission x |cos| is what is compared (measured 2.55e-8 at depth 1, 3.37e-8 at depth 2, about half a float32 ulp of the values)."""
    c = cases("mirrors")
    vis = True
    aov = c.hs.render_aovs(centre=True, camera=c.cam, specular_depth=depth).reshape(-1, 8)
    lit, pos, info = plc.lit_frame(c.hs, c.vol, vis, centre=True, camera=c.cam, specular_depth=depth)
    lit, pos = lit.reshape(-1, 3), pos.reshape(-1, 3)
    walk = plc.chain_walk(oracle, c.hs, c.sd, c.cam, depth)
    kind = walk["kind"]
    s, e, m = kind == plc.SURFACE, kind == plc.EMITTER, kind == plc.MISS
    chained = walk["bounces"] > 0
    print("\n[probe lit] chains depth %d: %d surface, %d emitter, %d sky terminals; %d pixels followed a bounce, %d of them to an emitter"
          % (depth, int(s.sum()), int(e.sum()), int(m.sum()), int(chained.sum()), int((chained & e).sum())))
    assert (chained & s).sum() > 50 and (chained & m).sum() > 10 and (chained & e).sum() > 0
    assert np.array_equal(aov[:, 7] > 0, ~m)
    alb, nf = aov[:, 0:3], aov[:, 3:6]
    E = c.vol.lookup(hip, pos[s], nf[s], vis)
    assert_equal(lit[s], alb[s] * np.fmax(E, f32(0)), "terminal surfaces")
    assert_equal(lit[m], alb[m] * np.asarray(c.sd.background, f32)[None, :], "terminal misses")
    assert not pos[m].any()
    assert info["lookups"] == int(s.sum()) and info["samples"] == W * H
    # float64: the terminal points, and the emitters
    dev_p = float(np.abs(pos[~m].astype(f64) - walk["p64"][~m]).max())
    emit = c.sd.materials["emission"][plc.prim_materials(c.sd)[walk["prim"][e]]].astype(f64)
    cs = np.abs(np.einsum("ij,ij->i", -walk["d"][e], walk["n"][e]))
    want_e = alb[e].astype(f64) * np.clip(emit * cs[:, None], 0, 1)
    dev_e = float(np.abs(lit[e].astype(f64) - want_e).max())
    print("[probe lit] chains depth %d: max |position - float64 walk| = %.3g, max |emitter - float64 rule| = %.3g" % (depth, dev_p, dev_e))
    assert dev_p <= 4 * POSITION_DEV and dev_e <= 4 * EMITTER_DEV
    # an emitter behind a mirror shows as the emitter, not as the sky, and below the clamp
    seen = chained & e
    assert (lit[seen] > 0).all() and (lit[seen] < f32(DIM)).all() and (np.clip(emit * cs[:, None], 0, 1) < 1).all()


def test_chain_depth_zero_is_the_plain_frame(hip, cases):
    c = cases("mirrors")
    want = c.want(hip, True)
    lit, pos, _ = plc.lit_frame(c.hs, c.vol, True, centre=True, camera=c.cam, specular_depth=0)
    assert_equal(lit, want["lit"], "mirrors, depth 0")
    assert_equal(pos, want["position"], "mirrors, depth 0, position")
    deep, _, _ = plc.lit_frame(c.hs, c.vol, True, centre=True, camera=c.cam, specular_depth=2, position=False)
    assert (deep != lit).any(axis=2).mean() > 0.1  # the mirrors are in view


# ---------------------------------------------------------------- 4. chunks and buffers
def test_chunks_and_buffers(pkg, hip, cases):
    """A scene that has never rendered works in buffers of the call's own; after a render with the smallest pool (768 paths: chunks of at
    most 1088 rays, so the 32 x 24 centre frame is one chunk whatever the pool) case 1's view at 64 x 48 centre rays and the jittered
    frame of 2553 rays are cut into three chunks each inside the workspace.  Every run equals the restated frame; a second call allocates nothing."""
    c, j = cases("sah"), cases("rc")
    want_c = c.want(hip, True)
    want_j = plc.restate_depth0(j.hs, hip, j.sd, j.vol, True, j.cam, centre=False, spp=SPPJ, seed=7)
    big = cornell_camera(pkg, 64, 48)  # case 1's view at 3072 centre rays: three chunks of the 768-path pool
    want_b = plc.restate_depth0(c.hs, hip, c.sd, c.vol, True, big, aov=c.hs.render_aovs(centre=True, camera=big))
    for case, cam, want, kw, chunks in ((c, c.cam, want_c, dict(centre=True), 1), (c, big, want_b, dict(centre=True), 3),
                                        (j, j.cam, want_j, dict(aov_spp=SPPJ, seed=7), 3)):
        hs = hip.HipScene(case.sd, **case.kw)
        vol = plc.Volume(hs, case.grid, 64, 64, case.md, normal_bias=case.vol.nb)  # (the bake may leave a workspace behind: printed below)
        assert np.array_equal(vol.sh, case.vol.sh) and np.array_equal(vol.mom, case.vol.mom)
        lit, pos, info = plc.lit_frame(hs, vol, True, camera=cam, **kw)
        fresh_ws = info["in_workspace"]
        assert_equal(lit, want["lit"], "first call")
        assert_equal(pos, want["position"], "first call, position")
        hs.render(camera=cam, spp=1, seed=1, pool_paths=768)
        lit, pos, info = plc.lit_frame(hs, vol, True, camera=cam, **kw)
        assert info["in_workspace"] == 1
        assert info["chunks"] >= chunks, info
        assert_equal(lit, want["lit"], "after a render, %d chunks" % info["chunks"])
        assert_equal(pos, want["position"], "after a render, position")
        before = hs.probe_buffers()
        lit2, _, info2 = plc.lit_frame(hs, vol, True, camera=cam, **kw)
        assert hs.probe_buffers() == before and info2["chunks"] == info["chunks"]
        assert_equal(lit2, lit, "second call")
        o, d = hs.centre_rays(np.arange(64, dtype=np.uint32), camera=cam)
        assert closest(hs, Rays(o, d))[1]["grew"] in (0, 1)
        assert closest(hs, Rays(o, d))[1]["grew"] == 0
        plc.lit_frame(hs, vol, True, camera=cam, **kw)
        assert closest(hs, Rays(o, d))[1]["grew"] == 0 and hs.probe_buffers() == before
        print("\n[probe lit] %s %d x %d: in_workspace %d before any render, then 1 with %d chunk(s)"
              % (case.name, int(cam["width"]), int(cam["height"]), fresh_ws, info["chunks"]))
        hs.close()
    # a scene on which nothing but the lit call has run: buffers of the call's own
    hs = hip.HipScene(c.sd, **c.kw)
    lit, pos, info = plc.lit_frame(hs, c.vol, True, camera=c.cam, centre=True)
    assert info["in_workspace"] == 0 and info["chunks"] == 1
    assert_equal(lit, want_c["lit"], "a scene that has never rendered")
    assert_equal(pos, want_c["position"], "a scene that has never rendered, position")
    hs.close()


# ---------------------------------------------------------------- 5. the live scene
def test_live_scene(pkg, hip, cases):
    """Baked once; after an update, a deformation, a hidden object, an addition and a material edit the frame from the OLD volume equals
    the restatement on a fresh scene of the edited description."""
    c = cases("sah")
    sd, (objs, tris) = split(hip, c.sd, [PLASTIC_SPHERE])
    hs = hip.HipScene(sd, builder="sah")
    frames = []

    def check(fresh_sd, what):
        fresh = hip.HipScene(fresh_sd, builder="sah")
        aov = fresh.render_aovs(centre=True, camera=c.cam)
        for visible in (True, False):
            want = plc.restate_depth0(fresh, hip, fresh_sd, c.vol, visible, c.cam, aov=aov)
            lit, pos, info = plc.lit_frame(hs, c.vol, visible, centre=True, camera=c.cam)
            assert_equal(lit, want["lit"], what)
            assert_equal(pos, want["position"], what + ", position")
            assert info["lookups"] == want["lookups"]
        fresh.close()
        frames.append(lit)
        if len(frames) > 1:
            assert (frames[-1] != frames[-2]).any(), what + ": the edit is not in the frame"

    check(sd, "as created")
    m = translate(40, 0, -30)
    hs.update([(SHORT, m)])
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    check(now, "update")
    P = wave(object_positions(sd, SHORT))
    hs.deform([(SHORT, P)])
    now = deformed_scene(pkg, hip, sd, {SHORT: P}, {SHORT: m})
    check(now, "deform")
    hs.set_visibility([(SHORT, False)])
    csd, _ = hip.compact_scene(now, mask_hiding(now, [SHORT]))
    check(csd, "set_visibility")
    hs.set_visibility([(SHORT, True)])
    hs.add_objects(objs, tris if len(tris) else None)
    now = extend_numpy(now, objs, tris, [])
    check(now, "add_objects")
    left = int(now.objects["material"][LEFT])
    edits = [(left, with_fields(now.materials[left], base_reflectance=(0.2, 0.3, 0.9)))]
    hs.set_materials(edits)
    check(edited_scene(now, edits), "set_materials")
    hs.close()


# ---------------------------------------------------------------- 6. nothing else moved
def test_a_lit_call_leaves_the_scene_as_it_was(hip, cases):
    c = cases("sah")
    hs = hip.HipScene(c.sd, **c.kw)
    o, d = hs.centre_rays(np.arange(W * H, dtype=np.uint32), camera=c.cam)

    def state():
        fb, _ = hs.render(camera=c.cam, spp=2, seed=5)
        aov = hs.render_aovs(aov_spp=2, seed=3, camera=c.cam, specular_depth=1)
        q = closest(hs, Rays(o, d), want=("t", "prim", "normal"))[0]
        return fb, aov, q

    fb0, aov0, q0 = state()
    for kw in (dict(centre=True), dict(aov_spp=SPPJ, seed=2, specular_depth=2)):
        plc.lit_frame(hs, c.vol, True, camera=c.cam, **kw)
        plc.lit_frame(hs, c.vol, False, camera=c.cam, **kw)
    fb1, aov1, q1 = state()
    assert_equal(fb1, fb0, "render")
    assert_equal(aov1, aov0, "render_aovs")
    assert np.array_equal(q1["t"], q0["t"]) and np.array_equal(q1["prim"], q0["prim"])
    assert_equal(q1["normal"], q0["normal"], "query_closest")
    hs.close()


# ---------------------------------------------------------------- 7. the wall
def quad(a, b, c, d):
    """Two triangles (a, b, c), (a, c, d): the normal is (b - a) x (c - a)."""
    return [(a, b, c), (a, c, d)]


def box_tris(pkg, lo, hi, outward=True):
    """The twelve triangles of an axis-aligned box, every normal pointing out of it (outward) or into it."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),
             ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),
             ((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))]
    t = []
    for f in faces:
        t += quad(*(f if outward else f[::-1]))
    tris = np.zeros(len(t), dtype=pkg.scenes.TRI_DTYPE)
    for k, (a, b, c) in enumerate(t):
        tris["v0"][k], tris["v1"][k], tris["v2"][k] = f32(a), f32(b), f32(c)
    return tris


def two_rooms(pkg):
    """The two sealed rooms of tests/test_gpu_probe_depth.py: a room [0, 4] x [0, 2] x [0, 2] whose walls face inward, cut in two by a slab
    0.1 thick at x = 2; a square emitter below the ceiling of room A (x < 2) only; background 0.  The camera stands in room B and looks at
    the edge where the shared wall meets the floor, from 0.4 away."""
    S = pkg.scenes
    b = S._Builder()
    white = b.material("white", S.material_presets()["rough_white_conductor"])
    light = b.material("light", S._mat(S.ROUGH_CONDUCTOR, emission=S.light_emission(1.0)))
    b.add_mesh(box_tris(pkg, (0, 0, 0), (4.0, 2.0, 2.0), outward=False), white)
    b.add_mesh(box_tris(pkg, (1.95, 0.0, 0.0), (2.05, 2.0, 2.0), outward=True), white)
    lt = np.zeros(2, dtype=S.TRI_DTYPE)
    for k, (a, bb, cc) in enumerate(quad((0.6, 1.99, 0.6), (1.4, 1.99, 0.6), (1.4, 1.99, 1.4), (0.6, 1.99, 1.4))):  # normal (0, -1, 0)
        lt["v0"][k], lt["v1"][k], lt["v2"][k] = f32(a), f32(bb), f32(cc)
    b.add_mesh(lt, light)
    # (every point in view lies within 0.45 of the wall, between the probe columns x = 1.5 and x = 2.5: farther into room B a cell has dark
    # probes only and the plain lookup is 0 as well)
    cam = S.make_camera(W, H, 40, (2.45, 1.0, 1.0), (2.05, 0.0, 1.0))
    return b.finish(camera=cam, rr_rate=0.7, spp=4, name="rooms", background=np.zeros(3, f32))


def test_light_does_not_leak_through_a_wall(pkg, hip):
    """The premise: a path-traced frame from the dark room is exactly 0 on every pixel.  The plain lit frame is positive on every hit pixel
    (it leaks through the slab), and the summed occlusion-aware frame lies strictly below the summed plain one.  Printed and recorded in
    DESIGN.md, not asserted: the ratio of the two sums."""
    sd = two_rooms(pkg)
    hs = hip.HipScene(sd, builder="sah")
    fb, _ = hs.render(spp=4, seed=3)
    assert (fb == 0).all(), "room B is not dark: the scene of this test is wrong"
    grid = ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (4, 2, 2))
    vol = plc.Volume(hs, grid, 512, 512, 3.0, normal_bias=0.02)
    assert (vol.cnt[:, 1] == 0).all()
    plain, pos, info = plc.lit_frame(hs, vol, False, centre=True)
    vis, _, _ = plc.lit_frame(hs, vol, True, centre=True)
    assert info["lookups"] == W * H  # a sealed room: every pixel is a hit
    assert (pos[..., 0] >= 2.05 - 1e-4).all() and (pos[..., 0] < 2.5).all()  # ... in room B, in the cells the wall cuts
    assert (pos[..., 1] < 1e-4).any() and (pos[..., 1] > 0.1).any()  # the floor and the wall
    assert (plain > 0).all(), "the plain frame does not leak on %d values: the test would show nothing" % int((plain <= 0).sum())
    ratio = vis.astype(f64).sum() / plain.astype(f64).sum()
    print("\n[probe lit] leak through the wall: sum visible / sum plain = %.4g over %d pixels; plain mean %.4g" % (ratio, W * H, plain.mean()))
    assert (vis >= 0).all() and vis.astype(f64).sum() < plain.astype(f64).sum()
    hs.close()


# ---------------------------------------------------------------- 8. refusals on a live handle; torch
def test_refusals_on_a_live_handle(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    cam = np.ascontiguousarray(c.cam)
    pcam = cam.ctypes.data_as(C.c_void_p)
    host = np.zeros((H * W * 3 + 18 * 192,), f32)
    lit, pos = pdc.Guarded((H, W, 3)), pdc.Guarded((H, W, 3))
    g = hip.ProbeGrid((C.c_float * 3)(*c.grid[0]), (C.c_float * 3)(*c.grid[1]), (C.c_int32 * 3)(*c.grid[2]), (C.c_int32 * 3)(0, 0, 0))
    v = hip.ProbeVisibility(c.vol.nb, c.vol.bm, (C.c_int32 * 2)(0, 0))
    D = c.vol.dev
    info = hip.LitInfo()

    def call(o=None, sh=D["sh"].ptr, mom=D["moments"].ptr, cnt=D["counts"].ptr, vis=v, out_lit=lit.ptr, out_pos=pos.ptr, grid=g):
        o = o or hip.LitOpts(1, 0, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0))
        pv = hip.ProbeVolume(C.pointer(grid), sh, mom, cnt, C.pointer(vis) if vis is not None else None)
        po = hip.LitOutputs(out_lit, out_pos, (C.c_void_p * 2)(None, None))
        return L.mcpt_render_probe_lit(hs.h, pcam, C.byref(o), C.byref(pv), C.byref(po), None, C.byref(info))

    bad_grid = hip.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 0, 1), (C.c_int32 * 3)(3, 2, 3), (C.c_int32 * 3)(0, 0, 0))
    for kw, word in ((dict(sh=host.ctypes.data), b"device"), (dict(mom=host.ctypes.data), b"device"), (dict(cnt=host.ctypes.data), b"device"),
                     (dict(out_lit=host.ctypes.data), b"device"), (dict(out_pos=host.ctypes.data), b"device"),
                     (dict(mom=None), b"all null"), (dict(vis=None), b"all null"), (dict(out_lit=None), b"null"), (dict(sh=None), b"null"),
                     (dict(o=hip.LitOpts(2, 0, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0))), b"centre"),
                     (dict(o=hip.LitOpts(1, 9, 0, 1, (C.c_int32 * 4)(0, 0, 0, 0))), b"specular_depth"),
                     (dict(o=hip.LitOpts(1, 0, 0, 1, (C.c_int32 * 4)(0, 0, 1, 0))), b"reserved"), (dict(grid=bad_grid), b"spacing"),
                     (dict(vis=hip.ProbeVisibility(-1.0, 0.25, (C.c_int32 * 2)(0, 0))), b"normal_bias")):
        rc = call(**kw)
        assert rc == 1 and b"mcpt_render_probe_lit" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert info.samples == 0 and info.chunks == 0
    assert (lit.get() == f32(SENTINEL)).all() and (pos.get() == f32(SENTINEL)).all()  # nothing was written
    # ... and the handle still renders the frame
    assert call() == 0 and info.samples == W * H
    assert_equal(lit.get(), c.want(hip, True)["lit"], "after the refusals")
    # the Python side: a buffer of the wrong size never reaches the library
    with pytest.raises(ValueError):
        hs.render_probe_lit(*c.grid, D["sh"], out={"lit": pdc.Guarded((H, W + 1, 3))}, camera=c.cam)
    with pytest.raises(ValueError):
        hs.render_probe_lit(*c.grid, D["sh"], moments=D["moments"], out={"lit": lit}, camera=c.cam)


def test_torch_tensors_on_a_side_stream():
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_lit_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["on_side_stream"] and rec["outputs_are_torch"]
    assert rec["lit_differ"] == 0 and rec["position_differ"] == 0 and rec["plain_differ"] == 0 and rec["chain_differ"] == 0
    assert rec["non_contiguous_refused"]
