"""tests/bvh_model.py, the restatement of the device tree builders that tests/test_gpu_builders_model.py holds the kernels to, checked
without a GPU: its trees satisfy the invariants of tests/test_bvh_host.py on every comparison scene, its pieces agree with slower
statements of the same thing, and the cases that can be worked out by hand come out as worked out."""
import math

import numpy as np
import pytest
from bvh_model import CASES, IDENTICAL, build_model, case_scene, lbvh_hierarchy, morton_codes, ploc_nearest, prim_boxes, spread21
from test_bvh_host import check_tree


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("name", CASES)
def test_model_trees_satisfy_the_tree_invariants(pkg, name, builder):
    sd = case_scene(pkg, name)
    info, boxes, children, qboxes = build_model(sd, builder)
    n = len(sd.triangles) + int((sd.objects["kind"] == 1).sum())
    assert info["n_nodes"] == n - 1 == len(boxes) == len(children)
    inner = children[children >= 0]
    assert len(set(inner.tolist())) == n - 2 and info["root"] not in inner  # every node but the root is the child of exactly one node
    h = check_tree(sd, info, boxes, children, qboxes)
    assert h + 1 == info["stack_entries"]  # levels, leaves included
    assert n.bit_length() <= info["stack_entries"] <= 48


def test_spread_matches_a_bit_by_bit_loop():
    rng = np.random.default_rng(1)
    for x in [0, 1, 2, 0x1fffff, 0x100000, 0x0aaaaa, 0x155555] + rng.integers(0, 1 << 21, 200).tolist():
        want = 0
        for b in range(21):
            want |= ((x >> b) & 1) << (3 * b)
        assert spread21(x) == want
    assert spread21(0x3fffff) == spread21(0x1fffff)  # bits above the 21st are dropped


def test_morton_code_by_hand():
    """Three unit boxes: centroids (0.5, 0.5, 0.5), (1.5, 0.5, 0.5) and (2.5, 2.5, 2.5).  u = 0, 0.5, 1 on x and 0, 0, 1 on y and z;
    q = 0, 2^20, 2^21 - 1 (the clamp); x sits one bit above y, y one above z."""
    pmin = np.float32([[0, 0, 0], [1, 0, 0], [2, 2, 2]])
    codes = morton_codes(pmin, pmin + np.float32(1))
    assert codes == [0, 1 << (3 * 20 + 2), (1 << 63) - 1]
    # one axis without extent: inv = 0 there, and the other axes are unaffected
    pmin = np.float32([[0, 7, 0], [4, 7, 0], [4, 7, 8]])
    codes = morton_codes(pmin, pmin)
    full = spread21(0x1fffff)
    assert codes == [0, full << 2, (full << 2) | full]


def test_hierarchy_by_hand():
    """Karras's example shape on five keys, then equal keys: those are told apart by position, which gives a balanced tree."""
    assert lbvh_hierarchy([1, 2]) == [(~0, ~1)]
    # keys 0b0001 0b0010 0b0100 0b0101 0b1000: the top split is before the last key, then {0,1} | {2,3}
    assert lbvh_hierarchy([1, 2, 4, 5, 8]) == [(3, ~4), (~0, ~1), (~2, ~3), (1, 2)]
    assert lbvh_hierarchy([7] * 4) == [(1, 2), (~0, ~1), (~2, ~3)]
    assert lbvh_hierarchy([7] * 3) == [(1, ~2), (~0, ~1)]


@pytest.mark.parametrize("n", IDENTICAL)
def test_identical_boxes_pair_up(pkg, n):
    """n copies of one triangle.  Every area is equal, so the tie rule alone decides: clusters (2k, 2k+1) merge in every round -- ceil(log2 n)
    rounds, ceil(log2 n) + 1 levels.  Under the rule the kernel had before (the smaller index) only clusters 0 and 1 were mutual: n - 1
    rounds and a chain of n levels, which the scene loader refuses beyond 48."""
    sd = case_scene(pkg, "identical-%d" % n)
    info, boxes, children, _ = build_model(sd, "ploc")
    lg = math.ceil(math.log2(n))
    assert info["rounds"] == lg and info["stack_entries"] == lg + 1
    assert info["stack_entries"] <= 2 * lg + 2  # (the bound the device test asserts)
    assert children[:n // 2].tolist() == [[~(2 * k), ~(2 * k + 1)] for k in range(n // 2)]  # first round: leaves in slot order
    assert info["root"] == n - 2
    old, _, old_children, _ = build_model(sd, "ploc", tie="smaller")
    assert old["rounds"] == n - 1 and old["stack_entries"] == n
    assert old_children[0].tolist() == [~0, ~1] and old_children[1].tolist() == [0, ~2]
    if n == 8:
        assert children.tolist() == [[~0, ~1], [~2, ~3], [~4, ~5], [~6, ~7], [0, 1], [2, 3], [4, 5]]
    lb, _, _, _ = build_model(sd, "lbvh")
    assert lb["stack_entries"] == lg + 1  # equal codes split by position


def test_nested_boxes_in_order_of_size_chain_whatever_the_tie_rule(pkg):
    """Not a tie: box k contains box k - 1, so the smallest union of cluster k is with k - 1, whose own is with k - 2; only the two
    smallest are mutual.  One merge per round, n levels -- which is why the comparison scene "nested-65" is shuffled."""
    sd = case_scene(pkg, "nestedsorted-20")
    for tie in ("paired", "smaller"):
        info, _, children, _ = build_model(sd, "ploc", tie=tie)
        assert info["rounds"] == 19 and info["stack_entries"] == 20
        assert children.tolist() == [[~0, ~1]] + [[k - 1, ~(k + 1)] for k in range(1, 19)]
    assert build_model(case_scene(pkg, "nested-65"), "ploc")[0]["stack_entries"] == 43


def test_tie_rule_is_symmetric_and_only_decides_ties(pkg):
    """With strictly ordered areas (random float boxes) the tie rule never acts: the tree is the one the former rule built.  With ties,
    the best pair is still mutual in every round (build_model asserts progress) and nearest neighbours stay within the radius."""
    rng = np.random.default_rng(11)
    lo = rng.uniform(0, 100, (200, 3)).astype(np.float32)
    hi = lo + rng.uniform(0.1, 3, (200, 3)).astype(np.float32)
    for radius in (1, 3, 16):
        a, b = ploc_nearest(lo, hi, radius, "paired"), ploc_nearest(lo, hi, radius, "smaller")
        assert np.array_equal(a, b) and (np.abs(a - np.arange(200)) <= radius).all() and (a != np.arange(200)).all()
    sd = case_scene(pkg, "random-257")
    pmin, pmax, _ = prim_boxes(sd)
    for radius in (1, 2, 64):
        nn = ploc_nearest(pmin, pmax, radius)
        assert (nn >= 0).all() and (nn < 257).all() and (np.abs(nn - np.arange(257)) <= radius).all()
        assert (nn[nn] == np.arange(257)).any()


def test_sphere_ids_and_radius_clamp(pkg):
    sd = case_scene(pkg, "mixed")
    n_tri = len(sd.triangles)
    assert sd.objects["kind"].tolist() == [0, 1, 0, 1]
    pmin, pmax, ids = prim_boxes(sd)
    assert ids.tolist() == list(range(n_tri)) + [n_tri + 1, n_tri + 3]
    assert (pmin[n_tri] == pmin[5]).all() and (pmax[n_tri] == pmax[5]).all()  # each sphere shares its box with a triangle
    assert (pmin[n_tri + 1] == pmin[n_tri - 1]).all() and (pmax[n_tri + 1] == pmax[n_tri - 1]).all()
    for builder in ("lbvh", "ploc"):
        _, _, children, _ = build_model(sd, builder)
        assert sorted((~children[children < 0]).tolist()) == ids.tolist()
    sd = case_scene(pkg, "random-257")
    for asked, used in ((100, 64), (0, 1)):
        a, b = build_model(sd, "ploc", ploc_radius=asked), build_model(sd, "ploc", ploc_radius=used)
        assert np.array_equal(a[2], b[2]) and a[0] == b[0]
    assert not np.array_equal(build_model(sd, "ploc", ploc_radius=1)[2], build_model(sd, "ploc", ploc_radius=2)[2])
