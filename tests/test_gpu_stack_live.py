"""Live edits that move a tree across a stack class border under a handle that already has its workspace and its query context:
add_objects, set_visibility and deform on the flipped chain of tests/stack_cases.py with the linear builder, whose tree is rebuilt on
every edit.  Every case first renders one sample per pixel and runs one query of each kind, so that the workspace (sized without
retrace lists below 25 levels), the query context's retrace capacity and the feature pass's choice of buffers exist for the OLD class.

After every edit the feature pass runs once BEFORE the first render (its rays then do not fit the workspace's retrace list and fall
back to the call's own buffers), and then everything tests/test_gpu_stack_classes.py asks of a created scene is asked of the edited
one: height, residency, every entry point against the oracle on the rays the model counts -- and all of it, with a frame and the feature
buffers at specular depth 2, equals a freshly created scene of the edited description bit for bit.

PLOC: the chains the builder model offers for it (tests/bvh_model.py, "nestedsorted": boxes nested in order of size) are concentric, and
on rays through the common centre the model of the walk holds ONE entry (of height - 1 = 17 to 24): no ray there counts.  The borders are crossed with PLOC all the
same, by adding and hiding the next larger box, and the edited handle is held to a fresh scene bit for bit; which entry of a PLOC tree's
stack an answer comes from is not pinned."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from add_cases import extend_numpy  # noqa: E402
from bvh_model import _box_triangle, _scene, build_model  # noqa: E402
from deform_cases import deformed_scene  # noqa: E402
from stack_cases import (Expect, dumped_tree, entry_points, first_part, flipped_chain, last_entry_case, lit, model_tree, narrow_camera,  # noqa: E402
                         pulled_in, same, split_chain)

pytestmark = pytest.mark.gpu

f32 = np.float32
INFO = ("n_nodes", "bvh_height", "quantised", "lds_resident", "n_lights")
SETS = ("mixed-2100", "axis-257", "tilt-1")
FRAME = dict(spp=1, seed=3)
AOV = dict(aov_spp=1, seed=3, specular_depth=2)


def warm_up(hs, cam, o, d):
    """One frame and one query of each kind: the handle's allocations now fit the class it was created in."""
    hs.render(camera=cam, **FRAME)
    return entry_points(hs, o[:64], d[:64])


def assert_equals_fresh(hs, fresh, sets, cam, aov_first, what, prim_map=None):
    """Info, every entry point on every ray, a frame and the feature buffers: bit for bit.  prim_map: live ids -> ids of the compacted
    description, when something is hidden."""
    a, b = hs.info(), fresh.info()
    assert [a[k] for k in INFO] == [b[k] for k in INFO], (what, a, b)
    assert same(aov_first, fresh.render_aovs(camera=cam, **AOV)).all(), "%s: the feature pass before the first render differs" % what
    assert same(hs.render(camera=cam, **FRAME)[0], fresh.render(camera=cam, **FRAME)[0]).all(), "%s: the frame differs" % what
    assert same(hs.render_aovs(camera=cam, **AOV), fresh.render_aovs(camera=cam, **AOV)).all(), "%s: the feature pass differs" % what
    got = {}
    for name in SETS:
        o, d = sets[name]
        got[name] = entry_points(hs, o, d)
        ref = entry_points(fresh, o, d)
        for k, v in got[name].items():
            if prim_map is not None and k.endswith("prim"):
                v = np.where(v >= 0, prim_map[np.maximum(v, 0)], v)
                got[name][k] = v
            bad = ~same(v, ref[k])
            assert not bad.any(), "%s, %s: %s differs from the fresh scene on %d values" % (what, name, k, bad.sum())
    return got


class Live:
    """A handle under edit, and the check of one state of it against the model, the oracle and a fresh scene."""

    def __init__(self, pkg, hip, oracle, n, quantise, start):
        self.pkg, self.hip, self.oracle, self.n, self.quantise = pkg, hip, oracle, n, quantise
        self.cam = narrow_camera(pkg, n)
        self.hs = hip.HipScene(start, builder="lbvh", quantise=quantise)

    def check(self, sd_now, height, resident, what, mask=None, keep=frozenset([1])):
        """sd_now: the edited description (with `mask`, compacted for the fresh scene); the feature pass comes first."""
        aov_first = self.hs.render_aovs(camera=self.cam, **AOV)
        prim_map = None
        if mask is not None:
            sd_now, prim_map = self.hip.compact_scene(sd_now, mask)
        fresh = self.hip.HipScene(sd_now, builder="lbvh", quantise=self.quantise)
        info = self.hs.info()
        assert info["bvh_height"] == height, "%s: height %d, the model says %d" % (what, info["bvh_height"], height)
        assert info["lds_resident"] == resident, (what, info)
        tree = dumped_tree(fresh.dump_bvh())
        expect = Expect(self.oracle, sd_now, tree, keep, self.n)
        got = assert_equals_fresh(self.hs, fresh, expect.sets, self.cam, aov_first, what, prim_map)
        for name in SETS:
            expect.check(name, got[name])
        expect.close()
        fresh.close()


def keep_of(pkg, n, quantise):
    """The triangle to leave un-flipped, by the model on the model's own tree of the chain (float or quantised boxes)."""
    from chain_scene import chain_scene
    return last_entry_case(pkg, n, model_tree(chain_scene(pkg, n), bool(quantise)))


# ---------------------------------------------------------------- add, hide, show
@pytest.mark.parametrize("quantise", [1, 0])
@pytest.mark.parametrize("n", [26, 19, 22, 11])
def test_add_hide_show_across_a_border(pkg, hip, oracle, n, quantise):
    """The chain of n - 1 triangles (height n - 2: 24, 17, 20, 9) gets the next chain triangle as a new object: 24 -> 25 plain to retry (the
    retrace lists must appear), 17 -> 18, 20 -> 21 a larger plain stack, 9 -> 10 LDS-resident to not resident; hiding it goes back, showing
    it forth again."""
    keep = keep_of(pkg, n, quantise)
    assert keep == keep_of(pkg, n - 1, quantise) and n - 1 not in keep
    sd = split_chain(lit(flipped_chain(pkg, n, keep)))
    start, (objs, tris) = first_part(sd)
    L = Live(pkg, hip, oracle, n, quantise, start)
    sets = Expect(oracle, start, model_tree(start, bool(quantise)), keep, n).sets
    warm_up(L.hs, L.cam, *sets["mixed-2100"])
    low, high = (1 if n - 2 <= 9 else 0), 0
    assert L.hs.info()["bvh_height"] == n - 2 and L.hs.info()["lds_resident"] == low
    first, _ = L.hs.add_objects(objs, tris)
    assert first == 1
    added = extend_numpy(start, objs, tris)
    assert added.triangles.tobytes() == sd.triangles.tobytes() and added.objects.tobytes() == sd.objects.tobytes()
    L.check(sd, n - 1, high, "add_objects", keep=keep)
    L.hs.set_visibility([(1, False)])
    L.check(sd, n - 2, low, "hidden", mask=np.array([True, False]), keep=keep)
    L.hs.set_visibility([(1, True)])
    L.check(sd, n - 1, high, "shown again", keep=keep)
    L.hs.close()


# ---------------------------------------------------------------- deform
@pytest.mark.parametrize("quantise", [1, 0])
def test_deform_across_the_retry_border(pkg, hip, oracle, quantise):
    """Triangle 25 of the chain of 26 with its far edge pulled in to half its length: its centroid shares the leading Morton bit of an
    earlier triangle and the tree has 24 levels (the builder model picks the factor).  mcpt_scene_deform moves the edge out to where the
    chain has it: 25 levels, the retry flavour; and back in."""
    n = 26
    keep = keep_of(pkg, n, quantise)
    sd = split_chain(lit(flipped_chain(pkg, n, keep)))
    factor, P_in = pulled_in(sd, n - 1)
    tri = sd.triangles[n - 1]
    P_out = np.stack([tri["v0"], tri["v1"], tri["v2"]]).astype(f32)[None]
    start = deformed_scene(pkg, hip, sd, {1: P_in})
    assert build_model(start, "lbvh")[0]["stack_entries"] == n - 2
    L = Live(pkg, hip, oracle, n, quantise, start)
    sets = Expect(oracle, sd, model_tree(sd, bool(quantise)), keep, n).sets
    warm_up(L.hs, L.cam, *sets["mixed-2100"])
    assert L.hs.info()["bvh_height"] == n - 2
    print("\nfar edge of triangle %d pulled in by the factor %g: %d levels" % (n - 1, factor, n - 2))
    L.hs.deform([(1, P_out)])
    out = deformed_scene(pkg, hip, sd, {1: P_out})
    assert out.triangles["v0"].tobytes() == sd.triangles["v0"].tobytes()
    L.check(out, n - 1, 0, "deformed out", keep=keep)
    L.hs.deform([(1, P_in)])
    hs_in = hip.HipScene(start, builder="lbvh", quantise=quantise)
    assert L.hs.info()["bvh_height"] == hs_in.info()["bvh_height"] == n - 2
    aov_first = L.hs.render_aovs(camera=L.cam, **AOV)
    assert_equals_fresh(L.hs, hs_in, sets, L.cam, aov_first, "deformed back in")  # (a shorter chain with two triangles side by side: the model's verdict is not asked)
    hs_in.close()
    L.hs.close()


# ---------------------------------------------------------------- deeper than the stack
@pytest.mark.parametrize("quantise", [1, 0])
def test_an_edit_beyond_48_levels_is_refused(pkg, hip, oracle, quantise):
    """48 -> 49: the addition is refused with MCPT_ERR_LIMIT, info() and every answer are what they were, and a legal edit follows: the
    far edge of triangle 48 pulled in (47 levels)."""
    n = 50
    keep = keep_of(pkg, n - 1, quantise)
    sd = split_chain(lit(flipped_chain(pkg, n, keep)))
    start, (objs, tris) = first_part(sd)
    L = Live(pkg, hip, oracle, n - 1, quantise, start)
    expect = Expect(oracle, start, dumped_tree(L.hs.dump_bvh()), keep, n - 1)
    L.hs.render(camera=L.cam, **FRAME)
    info = L.hs.info()
    assert info["bvh_height"] == 48
    before = {name: entry_points(L.hs, *expect.sets[name]) for name in SETS}
    frame = L.hs.render(camera=L.cam, **FRAME)[0]
    for name in SETS:
        expect.check(name, before[name])
    with pytest.raises(hip.McptError) as e:
        L.hs.add_objects(objs, tris)
    assert e.value.code == 4 and "deeper than the traversal stack" in str(e.value), str(e.value)  # MCPT_ERR_LIMIT
    after = L.hs.info()
    assert [after[k] for k in INFO + ("n_prims",)] == [info[k] for k in INFO + ("n_prims",)]
    assert len(L.hs.sd.triangles) == n - 1
    for name in SETS:
        now = entry_points(L.hs, *expect.sets[name])
        for k, v in now.items():
            assert same(v, before[name][k]).all(), (name, k)
    assert same(L.hs.render(camera=L.cam, **FRAME)[0], frame).all()
    expect.close()
    # a legal edit: the whole mesh again, triangle 48 with its far edge pulled in
    one = split_chain(start)  # (triangle 48 as an object of its own, for pulled_in's positions only)
    factor, P48 = pulled_in(one, n - 2)
    tri = start.triangles
    P = np.stack([tri["v0"], tri["v1"], tri["v2"]], axis=1).astype(f32)
    P[n - 2] = P48[0]
    L.hs.deform([(0, P)])
    now = deformed_scene(pkg, hip, start, {0: P})
    fresh = hip.HipScene(now, builder="lbvh", quantise=quantise)
    assert L.hs.info()["bvh_height"] == fresh.info()["bvh_height"] == 47
    aov_first = L.hs.render_aovs(camera=L.cam, **AOV)
    assert_equals_fresh(L.hs, fresh, expect.sets, L.cam, aov_first, "after the refusal")
    fresh.close()
    L.hs.close()


# ---------------------------------------------------------------- PLOC
def nested(pkg, ks):
    """Boxes nested in order of size around one centre, one triangle each (tests/bvh_model.py, "nestedsorted"): PLOC's tree is a chain."""
    return lit(_scene(pkg, [[_box_triangle((512 - int(k),) * 3, 2 * int(k)) for k in ks]]))


@pytest.mark.parametrize("n", [25, 18, 21])
def test_ploc_add_and_hide_across_a_border(pkg, hip, n):
    """n - 1 nested boxes (PLOC: n - 1 levels, by the builder model) get the next larger one as a new object, lose it by hiding and get it
    back: 24 | 25, 17 | 18, 20 | 21.  Rays from outside through the common centre region; the edited handle equals a fresh scene."""
    sd = split_chain(nested(pkg, range(1, n + 1)))
    start, (objs, tris) = first_part(sd)
    assert build_model(start, "ploc")[0]["stack_entries"] == n - 1 and build_model(sd, "ploc")[0]["stack_entries"] == n
    rng = np.random.default_rng(n)
    u = rng.normal(size=(600, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (512 + 200 * u).astype(f32)
    d = (512 + rng.uniform(-1.5, 1.5, (600, 3)) - o).astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    d[:100:2, 0] = 0.0  # zero components among them
    sets = {"mixed-2100": (o, d), "axis-257": (o[:257], d[:257]), "tilt-1": (o[150:151], d[150:151])}
    cam = pkg.scenes.make_camera(8, 8, 2.0, (512, 512, 200), (512, 512, 512))
    hs = hip.HipScene(start, builder="ploc")
    warm_up(hs, cam, o, d)
    assert hs.info()["bvh_height"] == n - 1

    def check(sd_now, height, what, mask=None):
        aov_first = hs.render_aovs(camera=cam, **AOV)
        prim_map = None
        if mask is not None:
            sd_now, prim_map = hip.compact_scene(sd_now, mask)
        fresh = hip.HipScene(sd_now, builder="ploc")
        assert hs.info()["bvh_height"] == height, (what, hs.info()["bvh_height"], height)
        got = assert_equals_fresh(hs, fresh, sets, cam, aov_first, what, prim_map)
        assert (got["mixed-2100"]["prim"] >= 0).mean() > 0.5
        fresh.close()

    hs.add_objects(objs, tris)
    check(sd, n, "add_objects")
    hs.set_visibility([(1, False)])
    check(sd, n - 1, "hidden", mask=np.array([True, False]))
    hs.set_visibility([(1, True)])
    check(sd, n, "shown again")
    hs.close()
