"""The device tree builders (csrc/mcpt_lbvh.hip) held to tests/bvh_model.py, a plain restatement of them: on small scenes with integer
coordinates (where the model is exact whatever the compiler fuses, see its docstring) the tree in HBM equals the model's node by node --
children, boxes bit for bit, root, height -- for the linear BVH and for PLOC, at the sizes around the 256-lane block, with every
centroid equal, with a zero extent, with spheres among the meshes and at every PLOC search radius.  A tree that is merely valid
(tests/test_gpu_lbvh.py) but built from a swapped axis, a radius off by one or a sphere's ordinal does not pass.  Closest hits through
each tree are the oracle's bit for bit, and the four builders report the same primitive."""
import math

import numpy as np
import pytest
from bvh_model import CASES, _random_triangles, _scene, build_model, case_scene, prim_boxes
from test_bvh_host import check_tree

pytestmark = pytest.mark.gpu

N_RAYS = 2000


def _rays(sd, seed):
    """Origins outside the root box (on a sphere around it), aimed at points inside it: half of them anywhere in the root box, half inside
    the box of a random primitive, so that small primitives are hit too."""
    rng = np.random.default_rng(seed)
    pmn, pmx, _ = prim_boxes(sd)
    pmn, pmx = pmn.astype(np.float64), pmx.astype(np.float64)
    lo, hi = pmn.min(axis=0), pmx.max(axis=0)
    u = rng.normal(size=(N_RAYS, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (lo + hi) / 2 + (np.linalg.norm(hi - lo) + 1.0) * u  # farther from the centre than any corner of the box
    pick = rng.integers(0, len(pmn), N_RAYS)
    aim_lo, aim_hi = np.where(np.arange(N_RAYS)[:, None] % 2 == 0, lo, pmn[pick]), np.where(np.arange(N_RAYS)[:, None] % 2 == 0, hi, pmx[pick])
    tgt = rng.uniform(aim_lo, aim_hi)
    o = o.astype(np.float32)
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    assert ((o < lo) | (o > hi)).any(axis=1).all()
    return o, d


def _coincident(sd):
    """-> (shared[primitive id]: another primitive has the same geometry, largest[primitive id]: the largest id among those that share it).
    A hit on such a primitive is shared; which of the sharers is reported is a convention (the larger id wins a tie), not a property
    of the tree."""
    tri = sd.triangles
    key = np.concatenate([tri["v0"], tri["v1"], tri["v2"]], axis=1)
    _, inverse, counts = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    largest = np.zeros(len(counts), np.int64)
    np.maximum.at(largest, inverse, np.arange(len(tri)))
    n_obj = len(sd.objects)
    return (np.concatenate([counts[inverse] > 1, np.zeros(n_obj, bool)]),
            np.concatenate([largest[inverse], len(tri) + np.arange(n_obj)]))


def _check_hits(sd, hip, oracle, seed, make_scene):
    """make_scene(builder, quantise) -> HipScene.  t bit-equal to the oracle for every builder; ids equal across builders, equal to the
    oracle's wherever the hit is not shared by coincident primitives, and the largest of the sharers' where it is."""
    o, d = _rays(sd, seed)
    t_ref, p_ref = oracle.OracleScene(sd).intersect(o, d)
    coincident, largest = _coincident(sd)
    shared = coincident[np.maximum(p_ref, 0)] & (p_ref >= 0)
    assert (p_ref >= 0).mean() > 0.05, "the rays miss the scene"
    for quantise in (0, 1):
        first = None
        for builder in ("sah", "reference", "lbvh", "ploc"):
            t, p = make_scene(builder, quantise).intersect(o, d)
            assert np.array_equal(t.view(np.uint64), t_ref.view(np.uint64)), (builder, quantise, int((t != t_ref).sum()))
            assert np.array_equal(p[~shared], p_ref[~shared]), (builder, quantise)
            assert np.array_equal(p[shared], largest[p_ref[shared]]), (builder, quantise, "the larger id wins a tie")
            if first is None:
                first = p
            assert np.array_equal(p, first), (builder, quantise, "primitive ids depend on the builder")


def _assert_tree_equals_model(sd, hs, builder, model):
    info, boxes, children, qboxes = hs.dump_bvh()
    m_info, m_boxes, m_children, _ = model
    assert info["n_nodes"] == m_info["n_nodes"] == len(boxes)
    assert np.array_equal(children, m_children), "children differ at nodes %s" % np.nonzero((children != m_children).any(axis=1))[0][:8]
    assert np.array_equal(boxes.view(np.uint32), m_boxes.view(np.uint32)), "boxes differ at nodes %s" % np.nonzero((boxes != m_boxes).any(axis=1))[0][:8]
    assert info["root"] == m_info["root"]
    assert info["stack_entries"] == m_info["stack_entries"] == hs.info()["bvh_height"]
    assert np.array_equal(np.float32(info["root_min"]), np.float32(m_info["root_min"])) and np.array_equal(np.float32(info["root_max"]), np.float32(m_info["root_max"]))
    assert hs.info()["builder"] == (2 if builder == "lbvh" else 3)
    h = check_tree(sd, info, boxes, children, qboxes)
    assert h + 1 == info["stack_entries"]
    return info, qboxes


@pytest.mark.parametrize("name", CASES)
def test_device_trees_equal_the_model(pkg, oracle, hip, name):
    sd = case_scene(pkg, name)
    n = len(sd.triangles) + int((sd.objects["kind"] == 1).sum())
    for builder in ("lbvh", "ploc"):
        model = build_model(sd, builder)
        for quantise in (-1, 0, 1):  # automatic, never, always: the tree is the same; the quantised copy must contain it (check_tree)
            info, qboxes = _assert_tree_equals_model(sd, hip.HipScene(sd, builder=builder, quantise=quantise), builder, model)
            assert quantise < 0 or (qboxes is not None) == bool(quantise)
        if name.startswith("identical") and builder == "ploc":  # coincident primitives: pairs, not a chain
            assert info["stack_entries"] <= 2 * math.ceil(math.log2(n)) + 2
    _check_hits(sd, hip, oracle, 17, lambda builder, quantise: hip.HipScene(sd, builder=builder, quantise=quantise))


@pytest.mark.parametrize("radius", [1, 2, 16, 64, 100])
@pytest.mark.parametrize("n", [257, 513])
def test_ploc_search_radius(pkg, hip, monkeypatch, n, radius):
    """MCPT_PLOC_RADIUS, clamped to 1..64: clusters 255 / 256 (and 511 / 512 of the first rounds) look across a block edge, through the
    halo of k_ploc_nn's LDS tile."""
    sd = case_scene(pkg, "random-%d" % n)
    monkeypatch.setenv("MCPT_PLOC_RADIUS", str(radius))
    _assert_tree_equals_model(sd, hip.HipScene(sd, builder="ploc"), "ploc", build_model(sd, "ploc", ploc_radius=radius))


def test_host_built_top_over_ploc_clusters(pkg, oracle, hip, monkeypatch):
    """n = 2048 with MCPT_PLOC_TOP=64: top = min(64, n / 16 = 128) = 64, so the rounds stop at (at most) 64 clusters and the host's binned SAH
    builds the tree above them.  The top is not modelled: the tree invariants, the node count and the hits are checked."""
    n = 2048
    sd = _scene(pkg, [_random_triangles(n, seed=2048, lo=400, hi=600)])
    monkeypatch.setenv("MCPT_PLOC_TOP", "64")
    hs = hip.HipScene(sd, builder="ploc")
    info, boxes, children, qboxes = hs.dump_bvh()
    assert info["n_nodes"] == n - 1 == len(boxes)
    h = check_tree(sd, info, boxes, children, qboxes)
    assert h + 1 == info["stack_entries"] == hs.info()["bvh_height"]
    assert info["root"] == n - 2  # the top's nodes come last, its root last of all
    monkeypatch.setenv("MCPT_PLOC_TOP", "0")  # never: merged down to the root on the device
    assert not np.array_equal(hip.HipScene(sd, builder="ploc").dump_bvh()[2], children)
    monkeypatch.setenv("MCPT_PLOC_TOP", "64")
    _check_hits(sd, hip, oracle, 18, lambda builder, quantise: hip.HipScene(sd, builder=builder, quantise=quantise))
