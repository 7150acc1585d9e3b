"""Every traversal stack class held at its last entry (tests/stack_cases.py): the flipped chain of n triangles under the linear builder,
n = 10, 11, 18, 19, 21, 22, 25, 26 and 49, that is heights 9 | 10 (LDS-resident, 8 entries | 16), 17 | 18 (16 | kStkB), 20 | 21 (kStkB | 24),
24 | 25 (24 | the retry flavour) and 48 (the deepest tree the scratch stack of the retrace takes), with float and with quantised nodes,
and once on the checking build, whose four LDS entries send every ray here through the retrace kernels.

The float64 model of the walk says which rays count: they hold height - 1 entries, their answer is the entry pushed last, and every box
and triangle decision has slack.  On those rays every entry point must return the oracle's answer -- the same primitive, t bit for bit,
the occlusion rule of tests/ray_query_cases.py in float64, per-path values bit for bit -- and nothing is asserted on the others.  A stack
one entry short returns a miss and "visible" on exactly these rays (tests/test_stack_model_cpu.py).  No tolerance anywhere."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bvh_model import build_model  # noqa: E402
from chain_scene import chain_scene  # noqa: E402
from stack_cases import NS, Expect, bits, dumped_tree, entry_points, flipped_chain, last_entry_case, lit, narrow_camera, ray_sets, same  # noqa: E402

pytestmark = pytest.mark.gpu

CREATED = NS[:-1]  # (n = 50: 49 levels, refused -- tests/test_gpu_stack_live.py)
f32 = np.float32


class Case:
    """The flipped chain of n triangles in HBM, `keep` chosen by the model on the tree the device built, the model's verdict on every
    ray and the oracle's answers: made once, shared, never changed."""

    def __init__(self, pkg, hip, oracle, n, quantise, library=None):
        self.n = n
        plain = hip.HipScene(chain_scene(pkg, n), builder="lbvh", quantise=quantise, library=library)
        self.plain_info, self.plain_dump = plain.info(), plain.dump_bvh()
        plain.close()
        self.tree = dumped_tree(self.plain_dump)
        self.keep = last_entry_case(pkg, n, self.tree)
        self.sd = lit(flipped_chain(pkg, n, self.keep))
        self.hs = hip.HipScene(self.sd, builder="lbvh", quantise=quantise, library=library)
        self.expect = Expect(oracle, self.sd, self.tree, self.keep, n)
        self.model, self.sets = self.expect.model, self.expect.sets
        self._got = {}

    def got(self, name):
        if name not in self._got:
            self._got[name] = entry_points(self.hs, *self.sets[name])
        return self._got[name]


@pytest.fixture(scope="module")
def cases(pkg, hip, oracle):
    made = {}

    def get(n, quantise, library=None):
        key = (n, quantise, library)
        if key not in made:
            made[key] = Case(pkg, hip, oracle, n, quantise, library)
        return made[key]

    yield get
    for c in made.values():
        c.hs.close()
        c.expect.close()


FLAVOURS = [0, 1]
SETS = sorted(ray_sets(10))


# ---------------------------------------------------------------- height, tree, stack class
@pytest.mark.parametrize("quantise", FLAVOURS)
@pytest.mark.parametrize("n", CREATED)
def test_height_tree_and_class(pkg, cases, n, quantise):
    """The device's tree is the model's, node by node, for the plain chain and for the flipped one; the height is n - 1 (the test does
    not adapt: it fails with both numbers); a chain of 9 levels is LDS-resident and one of 10 is not."""
    c = cases(n, quantise)
    model = build_model(chain_scene(pkg, n), "lbvh")
    assert model[0]["stack_entries"] == n - 1
    for what, info, dump in (("chain", c.plain_info, c.plain_dump), ("flipped chain", c.hs.info(), c.hs.dump_bvh())):
        assert info["bvh_height"] == n - 1, "%s: the device reports height %d, the model %d" % (what, info["bvh_height"], n - 1)
        d_info, boxes, children, q = dump
        assert d_info["stack_entries"] == n - 1 and d_info["root"] == model[0]["root"]
        bad = np.flatnonzero((children != model[2]).any(axis=1))
        assert len(bad) == 0, "%s: children differ at nodes %s: device %s, model %s" % (what, bad[:8], children[bad[:8]].tolist(), model[2][bad[:8]].tolist())
        bad = np.flatnonzero((bits(boxes) != bits(model[1])).any(axis=1))
        assert len(bad) == 0, "%s: boxes differ at nodes %s: device %s, model %s" % (what, bad[:8], boxes[bad[:1]].tolist(), model[1][bad[:1]].tolist())
        assert np.array_equal(f32(d_info["root_min"]), f32(model[0]["root_min"])) and np.array_equal(f32(d_info["root_max"]), f32(model[0]["root_max"]))
        assert (q is not None) == bool(quantise) == bool(info["quantised"])
        assert info["lds_resident"] == (1 if n - 1 <= 9 else 0), "%s: height %d, lds_resident %d" % (what, n - 1, info["lds_resident"])
    if quantise:  # flipping changes no box, so no quantised box either
        assert np.array_equal(c.plain_dump[3], c.hs.dump_bvh()[3])


# ---------------------------------------------------------------- the entry points
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("quantise", FLAVOURS)
@pytest.mark.parametrize("n", CREATED)
def test_entry_points_at_the_last_entry(cases, n, quantise, name):
    c = cases(n, quantise)
    c.expect.check(name, c.got(name))


# ---------------------------------------------------------------- k_primary
@pytest.mark.parametrize("quantise", FLAVOURS)
@pytest.mark.parametrize("n", CREATED)
def test_primary_rays_at_the_last_entry(pkg, hip, oracle, cases, n, quantise):
    """k_primary: an 8 x 8 camera at the home ray's origin with a field of view as narrow as the tilted rays.  The model counts its rays
    (sample 0 of every pixel, as mcpt_camera_rays returns them); the sky cull sends every pixel through the walk (more than four boxes
    overlap it); the frame at one sample per pixel is the oracle's on the counting pixels, bit for bit, and differs from the sky there."""
    c = cases(n, quantise)
    cam = narrow_camera(pkg, n)
    pix = np.arange(64, dtype=np.uint32)
    o, d = c.hs.camera_rays(pix, np.zeros(64, np.uint32), seed=3, camera=cam)
    counting, _ = c.model.counting(o, d)
    print("\nn %d: %d of 64 camera rays count" % (n, counting.sum()))
    assert counting.mean() >= 0.5
    may_hit, cand, _ = c.hs.classify(camera=cam)
    assert (may_hit == 1).all() and (cand[:, 0] == -2).all(), "the sky cull does not send every pixel through the tree walk"
    fb, _ = c.hs.render(spp=1, seed=3, camera=cam)
    osc = oracle.OracleScene(dataclasses.replace(c.sd, camera=cam))
    ro, rd = osc.camera_rays(pix, np.zeros(64, np.uint32), seed=3)
    assert same(ro, o).all() and same(rd, d).all()
    want, _ = osc.render(spp=1, seed=3)
    osc.close()
    fb, want = np.asarray(fb, f32).reshape(64, 3), np.asarray(want, f32).reshape(64, 3)
    assert not (want[counting] == np.array(c.sd.background, f32)).all(axis=1).any(), "the oracle sees the sky on a counting pixel"
    bad = counting[:, None] & ~same(fb, want)
    assert not bad.any(), "render: %d values of counting pixels differ from the oracle" % bad.sum()


# ---------------------------------------------------------------- the checking build
@pytest.mark.parametrize("name", ["mixed-2100", "tilt-257"])
def test_checking_build(cases, hip_check, name):
    """-DMCPT_FORCE_RETRY -DMCPT_STK_RETRY=4: a ray that holds 23 entries loses one at its fifth push, so every ray here is listed and
    answered by k_retrace_closest, k_query_occluded_retrace, k_retrace_shadow and k_sensor_primary_retrace with the scratch stack."""
    c = cases(25, 1, hip_check)
    assert c.hs.info()["bvh_height"] == 24 and c.hs.info()["lds_resident"] == 0
    c.expect.check(name, c.got(name))
