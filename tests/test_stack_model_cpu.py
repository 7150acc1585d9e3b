"""tests/stack_cases.py checked without a GPU, on the model trees of tests/bvh_model.py: the chain of n triangles has n - 1 levels, the
flipped chain has the same tree, its rays hold a stack of height - 1 entries and take their answer from the last one, and a stack one
entry short changes that answer -- which it does not on the plain chain scene, the reason the flipped one exists.  Run with -s for the
figures: per n the height, the entries held, the position the answer came from and the answer under cap = height - 2."""
import numpy as np
import pytest
from bvh_model import build_model
from chain_scene import chain_scene
from stack_cases import FAR, HOME_D, HOME_O, NS, Counter, dumped_tree, flipped_chain, last_entry_case, model_tree, quantise_model, ray_sets
from test_bvh_host import check_tree


@pytest.mark.parametrize("n", NS)
def test_chain_height_and_unchanged_tree(pkg, n):
    plain = build_model(chain_scene(pkg, n), "lbvh")
    assert plain[0]["stack_entries"] == n - 1
    for keep in ((), (1,), tuple(range(0, n, 2))):
        flipped = build_model(flipped_chain(pkg, n, keep), "lbvh")
        assert flipped[0] == plain[0] and np.array_equal(flipped[1], plain[1]) and np.array_equal(flipped[2], plain[2]), keep
    qinfo, q = quantise_model(plain[0], plain[1])
    check_tree(chain_scene(pkg, n), qinfo, plain[1], plain[2], q)  # the quantised boxes contain the exact ones, within three cells
    assert dumped_tree((qinfo, plain[1], plain[2], q)).grid is not None and dumped_tree(plain).grid is None


@pytest.mark.parametrize("quantised", [False, True], ids=["float", "quantised"])
@pytest.mark.parametrize("n", NS)
def test_last_entry_case(pkg, n, quantised):
    """The case construction works, and the negative control: with cap = height - 2 the answer of every counting ray changes, a hit to a
    miss and occluded to visible.  The window walk of a shadow query with the light beyond every box enters nothing (no box reaches
    the window around `dist`) and holds no entry: only the occluder walk fills the stack."""
    tree = model_tree(chain_scene(pkg, n), quantised)
    h = tree.height
    assert h == n - 1
    keep = last_entry_case(pkg, n, tree)
    if not quantised:
        assert keep == {1}  # (under the quantised boxes the model chooses: near / far is decided by the grid)
    sd = flipped_chain(pkg, n, keep)
    model = Counter(sd, tree, keep)
    home = model.one(HOME_O, HOME_D, "closest", None)
    assert model.counts(home)
    short = model.one(HOME_O, HOME_D, "closest", None, cap=h - 2)
    print("\nn %d %s: height %d, keep %s, home ray holds %d entries, answer (primitive %d) from position %d; cap %d: primitive %d, %d push dropped"
          % (n, "quantised" if quantised else "float", h, sorted(keep), home.held, home.prim, home.pos, h - 2, short.prim, short.dropped))
    for name, (o, d) in ray_sets(n, large=300).items():
        for mode, dist in (("closest", None), ("occluder", FAR)):
            counting, full = model.counting(o, d, mode, dist)
            assert counting.mean() >= 0.5, (name, mode, counting.mean())
            capped = [model.one(o[i], d[i], mode, dist, cap=h - 2) for i in range(len(o))]
            for i in np.flatnonzero(counting):
                assert capped[i].dropped == 1 and capped[i].held == h - 2
                if mode == "closest":
                    assert full[i].prim in keep and capped[i].prim == -1
                else:
                    assert full[i].occluded and not capped[i].occluded
        w = model.one(o[0], d[0], "window", FAR)
        assert w.held == 0 and not w.found and not w.occluded, name
        print("  %-10s %4d rays, %4d count (closest and occluder); one entry short: hit -> miss, occluded -> visible on all of them; "
              "window walk: %d entries" % (name, len(o), int(counting.sum()), w.held))


@pytest.mark.parametrize("n", NS)
def test_plain_chain_does_not_depend_on_the_stack(pkg, n):
    """The finding that made the flipped chain necessary: on chain_scene the same rays fill the stack as well, but the winning triangle
    is reached by descent and never popped, so one entry less, or ten, return the same hit."""
    sd = chain_scene(pkg, n)
    tree = model_tree(sd)
    h = tree.height
    for name, (o, d) in ray_sets(n, large=300).items():
        if not name.endswith("-257"):
            continue
        for i in range(32):
            full = tree.walk(sd, o[i], d[i])
            assert full.held == h - 1 and full.prim == 0 and full.pos == -1
            for cap in (h - 2, max(h - 11, 0)):
                short = tree.walk(sd, o[i], d[i], cap=cap)
                assert (short.prim, short.t) == (full.prim, full.t) and short.dropped >= 1
            occ = tree.walk(sd, o[i], d[i], "occluder", FAR)
            assert occ.occluded and occ.pos == -1 and tree.walk(sd, o[i], d[i], "occluder", FAR, cap=h - 2).occluded
    print("\nn %d: plain chain, height %d: %d entries held, primitive 0 from the parked leaf (position -1); cap %d and %d: the same hit" % (n, h, h - 1, h - 2, max(h - 11, 0)))
