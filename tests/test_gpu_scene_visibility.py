"""mcpt_scene_set_visibility on the GPU: after the call a scene behaves like a scene freshly created from compact(desc'), the current
description without its hidden objects (mcpt_compact_scene), with the same build options.  Primitive ids are stable in the live scene, so
they are translated through prim_map before they are compared; everything else is compared as it is.

With the host builders (sah, reference) that is bit for bit, the tree dump included.  With the device builders (lbvh, ploc) the rule of
tests/test_gpu_scene_update.py applies: hits equal ray for ray, a frame within 3 floats (a box-grazing ray may take another branch).
Every comparison is between the edited handle and a fresh scene; nothing is compared with a recorded number."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deform_cases import (INFO_FIELDS, assert_same_frame, assert_same_tree, cornell_rays, deformed_scene, object_positions, rotate_y, same_bits,  # noqa: E402
                          translate, wave)
from visibility_cases import (LIGHT, PLASTIC_SPHERE, SHORT, TALL, live_ids, mask_hiding, translate_children, translate_ids)  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
DEVICE_BUILDERS = ("lbvh", "ploc")
TREE_FIELDS = ("n_nodes", "bvh_height", "quantised", "n_lights")  # (n_prims and lds_resident follow the stored records: include/mcpt.h)


def assert_same_info(hs, fresh):
    a, b = hs.info(), fresh.info()
    assert [a[k] for k in TREE_FIELDS] == [b[k] for k in TREE_FIELDS], (a, b)


def assert_same_hits(hs, fresh, o, d, prim_map):
    """Hits of the live scene, ids translated, against the fresh compacted scene's; `t` bit for bit.  Returns the live ids."""
    ta, pa = hs.intersect(o, d)
    tb, pb = fresh.intersect(o, d)
    pt = translate_ids(pa, prim_map)
    assert (pt != -2).all(), "%d rays hit a hidden primitive" % int((pt == -2).sum())
    assert np.array_equal(pt, pb), "primitive ids differ on %d rays" % int((pt != pb).sum())
    assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    return pa


def assert_same_tree_translated(hs, fresh, prim_map):
    (ia, ba, ca, qa), (ib, bb, cb, qb) = hs.dump_bvh(), fresh.dump_bvh()
    for k in ia:
        if k != "n_leaf_prims":  # (the first instance leaf: n_triangles + n_objects of the stored records; no instances here)
            assert np.array_equal(np.asarray(ia[k]), np.asarray(ib[k])), k
    assert ba.tobytes() == bb.tobytes() and translate_children(ca, prim_map).tobytes() == cb.tobytes()
    assert (qa is None) == (qb is None) and (qa is None or qa.tobytes() == qb.tobytes())


def assert_equals_compact(hip, hs, sd_now, mask, builder, quant=-1, spp=4, seed=5, n_random=6000):
    """The whole comparison of `hs` (current description sd_now, mask) with a fresh scene of the compacted description."""
    dev = builder in DEVICE_BUILDERS
    csd, prim_map = hip.compact_scene(sd_now, mask)
    fresh = hip.HipScene(csd, builder=builder, quantise=quant)
    assert_same_info(hs, fresh)
    if not dev:
        assert_same_tree_translated(hs, fresh, prim_map)
    W, H = int(sd_now.camera["width"].reshape(-1)[0]), int(sd_now.camera["height"].reshape(-1)[0])
    o, d = cornell_rays(hs, W, H, spp, n_random=n_random)
    prim = assert_same_hits(hs, fresh, o, d, prim_map)
    a, sa = hs.render(spp=spp, seed=seed)
    b, sb = fresh.render(spp=spp, seed=seed)
    assert_same_frame(a, b, dev, builder)
    assert abs(int(sa.vertices) - int(sb.vertices)) <= (3 if dev else 0)
    return fresh, prim_map, prim, a


@pytest.mark.parametrize("builder,quant", [("sah", -1), ("sah", 0), ("reference", 0), ("reference", 1), ("lbvh", -1), ("lbvh", 0), ("ploc", -1), ("ploc", 0)])
def test_hidden_objects_equal_a_fresh_compacted_scene(pkg, hip, builder, quant):
    """One call hides a mesh (the short box) and a sphere (the plastic one)."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder, quantise=quant)
    before, _ = hs.render(spp=4, seed=5)
    info = hs.set_visibility([(SHORT, False), (PLASTIC_SPHERE, False)])
    assert info["path"] == (1 if dev else 0) and info["n_moved_tris"] == int(sd.objects["n_tri"][SHORT])
    mask = mask_hiding(sd, [SHORT, PLASTIC_SPHERE])
    got_mask, n_vis = hs.visibility()
    assert np.array_equal(got_mask, mask.astype(np.uint8)) and n_vis == len(sd.triangles) - int(sd.objects["n_tri"][SHORT]) + 2
    assert hs.info()["n_prims"] == len(sd.triangles) + len(sd.objects)  # the stored records
    fresh, prim_map, prim, frame = assert_equals_compact(hip, hs, sd, mask, builder, quant)
    assert (prim >= 0).mean() > 0.5
    hidden = np.concatenate([live_ids(sd, SHORT), live_ids(sd, PLASTIC_SPHERE)])
    assert not np.isin(prim, hidden).any()
    assert (~same_bits(frame, before)).sum() > 100  # the objects did leave
    # the other entry points that take the scene
    assert_same_frame(hs.render_aovs(aov_spp=2, seed=5, specular_depth=2), fresh.render_aovs(aov_spp=2, seed=5, specular_depth=2), dev, "aovs")
    assert_same_frame(hs.render_motion(seed=5, aov_spp=2), fresh.render_motion(seed=5, aov_spp=2), dev, "motion")
    n = 4000
    rng = np.random.default_rng(9)
    px, sm, ch = rng.integers(0, 48 * 48, n).astype(np.uint32), rng.integers(0, 64, n).astype(np.uint32), rng.integers(0, 3, n).astype(np.int32)
    co, cd = hs.camera_rays(px, sm, seed=2)
    bad = ~same_bits(hs.cast_rays(co, cd, px, sm, ch, seed=2), fresh.cast_rays(co, cd, px, sm, ch, seed=2))
    assert bad.sum() <= (2 if dev else 0)


@pytest.mark.parametrize("builder", ["sah", "reference", "lbvh", "ploc"])
def test_show_again(pkg, hip, builder):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder)
    never = hip.HipScene(sd, builder=builder)
    hs.set_visibility([(SHORT, False), (PLASTIC_SPHERE, False), (TALL, False)])
    info = hs.set_visibility([(o, True) for o in range(len(sd.objects))])
    assert info["path"] == (1 if dev else 0) and info["n_moved_tris"] == int(sd.objects["n_tri"][[SHORT, TALL]].sum())
    mask, n_vis = hs.visibility()
    assert mask.all() and n_vis == len(sd.triangles) + 3
    a, b = hs.info(), never.info()
    assert [a[k] for k in INFO_FIELDS] == [b[k] for k in INFO_FIELDS], (a, b)  # (lds_resident and n_prims included)
    if not dev:
        assert_same_tree(hs, never)
    o, d = cornell_rays(hs, 48, 48, 4)
    ta, pa = hs.intersect(o, d)
    tb, pb = never.intersect(o, d)
    assert np.array_equal(pa, pb) and np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    assert_same_frame(hs.render(spp=4, seed=3)[0], never.render(spp=4, seed=3)[0], dev, builder)


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_edits_while_hidden(pkg, hip, builder):
    """A hidden object is moved, another mesh is deformed, and a host-path call (the light moves) comes in between: the records of the
    hidden object must be current on both paths when it is shown."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder)
    hs.set_visibility([(TALL, False)])
    turn = rotate_y(0.4, (368, 165, 351), shift=(-40, 0, -60))
    assert hs.update([(TALL, turn)])["path"] == (1 if dev else 0)
    light = translate(-60, -40, 30)
    assert hs.update([(LIGHT, light)])["path"] == 0
    P = wave(object_positions(sd, SHORT))
    assert hs.deform([(SHORT, P)])["path"] == (1 if dev else 0)
    sd_now = deformed_scene(pkg, hip, sd, {SHORT: P}, {TALL: turn, LIGHT: light})
    # still hidden: the compacted current description
    assert_equals_compact(hip, hs, sd_now, mask_hiding(sd, [TALL]), builder)
    assert hs.set_visibility([(TALL, True)])["path"] == (1 if dev else 0)
    fresh = hip.HipScene(sd_now, builder=builder)
    if not dev:
        assert_same_tree(hs, fresh)
    o, d = cornell_rays(hs, 48, 48, 4)
    ta, pa = hs.intersect(o, d)
    tb, pb = fresh.intersect(o, d)
    assert np.array_equal(pa, pb) and np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    assert np.isin(pa, live_ids(sd, TALL)).sum() > 100  # the tall box is seen again, where the update put it
    assert_same_frame(hs.render(spp=4, seed=5)[0], fresh.render(spp=4, seed=5)[0], dev, builder)
    u = np.random.default_rng(2).uniform(0, 1, (500, 4)).astype(f32)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()


@pytest.mark.parametrize("builder", ["sah", "reference", "lbvh", "ploc"])
def test_hiding_the_light_takes_the_host_path(pkg, hip, builder):
    """The light tables, the emitters' bounding sphere and n_lights are host-built: an emitter is hidden and shown on path 0."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    hs = hip.HipScene(sd, builder=builder)
    assert hs.info()["n_lights"] == 1
    u = np.random.default_rng(2).uniform(0, 1, (2000, 4)).astype(f32)
    original = hs.sample_light(u)
    info = hs.set_visibility([(LIGHT, False)])
    assert info["path"] == 0 and info["n_moved_tris"] == int(sd.objects["n_tri"][LIGHT])
    assert hs.info()["n_lights"] == 0
    fresh, _, _, _ = assert_equals_compact(hip, hs, sd, mask_hiding(sd, [LIGHT]), builder)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()
    assert not same_bits(hs.sample_light(u), original).all()
    assert hs.set_visibility([(LIGHT, True)])["path"] == 0
    assert hs.info()["n_lights"] == 1
    assert same_bits(hs.sample_light(u), original).all()


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_one_of_two_emitters(pkg, hip, builder):
    """A second emitter, a sphere: with either hidden the light table holds the other, and a sphere's light record keeps the sphere's slot."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    mats = sd.materials.copy()
    glow = int(sd.objects["material"][PLASTIC_SPHERE])
    assert (sd.objects["material"] == glow).sum() == 1
    mats["emission"][glow] = (4, 3, 2)
    sd = dataclasses.replace(sd, materials=mats)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder)
    assert hs.info()["n_lights"] == 2
    u = np.random.default_rng(2).uniform(0, 1, (2000, 4)).astype(f32)
    original = hs.sample_light(u)
    for hidden in (LIGHT, PLASTIC_SPHERE):
        assert hs.set_visibility([(o, o != hidden) for o in (LIGHT, PLASTIC_SPHERE)])["path"] == 0
        assert hs.info()["n_lights"] == 1
        fresh, _, _, _ = assert_equals_compact(hip, hs, sd, mask_hiding(sd, [hidden]), builder)
        assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()
    assert hs.set_visibility([(PLASTIC_SPHERE, True)])["path"] == 0
    assert hs.info()["n_lights"] == 2 and same_bits(hs.sample_light(u), original).all()
    # a non-emitter afterwards goes back to the builder's own path, from what the host path left
    assert hs.set_visibility([(SHORT, False)])["path"] == (1 if dev else 0)
    assert_equals_compact(hip, hs, sd, mask_hiding(sd, [SHORT]), builder)


@pytest.fixture(scope="module")
def chess(pkg):
    return pkg.scenes.chess_scene(width=64, height=36, spp=2)


# the first piece, the last object and two adjacent pieces; and, second, the king as well: its 2312 triangles put the first slot of the
# object after it 4 lanes into a block (the pawns have 2560 = 10 x 256 triangles each, the light and the board 2 each)
CHESS_HIDDEN = ([0, 17, 6, 7], [0, 16, 6, 7])


@pytest.mark.parametrize("builder", DEVICE_BUILDERS)
@pytest.mark.parametrize("hidden", CHESS_HIDDEN, ids=["issue", "king"])
def test_segment_edges_on_a_multi_block_scene(hip, chess, builder, hidden):
    sd = chess
    assert len(sd.objects) == 18 and len(sd.triangles) > 38000 and len(set(sd.objects["n_tri"].tolist())) >= 4
    hs = hip.HipScene(sd, builder=builder)
    info = hs.set_visibility([(o, False) for o in hidden])
    assert info["path"] == 1 and info["n_moved_tris"] == int(sd.objects["n_tri"][hidden].sum())
    mask = mask_hiding(sd, hidden)
    csd, prim_map = hip.compact_scene(sd, mask)
    fresh = hip.HipScene(csd, builder=builder)
    assert_same_info(hs, fresh)
    bi = fresh.dump_bvh()[0]
    rng = np.random.default_rng(6)
    lo, hi = np.array(bi["root_min"], f32), np.array(bi["root_max"], f32)
    o2 = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), size=(6000, 3)).astype(f32)
    d2 = rng.uniform(lo, hi, size=(6000, 3)).astype(f32) - o2
    d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(f32)
    pix = np.repeat(np.arange(64 * 36, dtype=np.uint32), 2)
    o1, d1 = hs.camera_rays(pix, np.tile(np.arange(2, dtype=np.uint32), 64 * 36), seed=7)
    prim = assert_same_hits(hs, fresh, np.concatenate([o1, o2]), np.concatenate([d1, d2]), prim_map)
    assert (prim >= 0).mean() > 0.2
    assert_same_frame(hs.render(spp=2, seed=4)[0], fresh.render(spp=2, seed=4)[0], True, builder)


def test_refusals_change_nothing(pkg, hip, chess):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    everything = [(o, False) for o in range(len(sd.objects))]
    for builder in ("sah", "ploc"):
        hs = hip.HipScene(sd, builder=builder)
        hs.set_visibility([(TALL, False)])
        frame, _ = hs.render(spp=4, seed=2)
        mask = hs.visibility()[0]
        bads = [[(len(sd.objects), False)], [(-1, True)], [(SHORT, False), (SHORT, True)], [(SHORT, 2)], everything]
        if builder == "ploc":  # one visible primitive (a sphere): the device builders need two; refused before the builder is reached
            bads.append([(o, False) for o in range(len(sd.objects)) if o != PLASTIC_SPHERE])
        for bad in bads:
            with pytest.raises(hip.McptError) as e:
                hs.set_visibility(bad)
            assert e.value.code == 1 and "mcpt_scene_set_visibility" in str(e.value), bad
            assert np.array_equal(hs.visibility()[0], mask)
            assert same_bits(frame, hs.render(spp=4, seed=2)[0]).all(), bad
    one = hip.HipScene(sd, builder="sah")  # a host-built scene may keep a single primitive, as creation allows
    one.set_visibility([(o, False) for o in range(len(sd.objects)) if o != PLASTIC_SPHERE])
    assert one.visibility()[1] == 1 and one.info()["n_nodes"] == 0
    inst = hip.HipScene(chess, builder="sah", instancing=True)
    assert inst.info()["n_instances"] == 14
    frame, _ = inst.render(spp=1, seed=2)
    with pytest.raises(hip.McptError) as e:
        inst.set_visibility([(16, False)])
    assert e.value.code == 1 and "instancing" in str(e.value)
    assert inst.visibility()[0].all() and same_bits(frame, inst.render(spp=1, seed=2)[0]).all()


def test_group_set_visibility(pkg, hip):
    """Two replicas on one device: mcpt_group_set_visibility, then mcpt_group_render, equals mcpt_render of the single scene."""
    sd = pkg.scenes.cornell_demo(64, 48, 4)
    items = [(SHORT, False), (PLASTIC_SPHERE, False), (LIGHT, True)]
    g = hip.HipGroup(sd, [0, 0])
    g.set_visibility(items)
    hs = hip.HipScene(sd)
    hs.set_visibility(items)
    a, _ = g.render(spp=4, seed=6)
    b, _ = hs.render(spp=4, seed=6)
    assert same_bits(a, b).all()
    assert not same_bits(a, hip.HipScene(sd).render(spp=4, seed=6)[0]).all()
    with pytest.raises(hip.McptError) as e:
        g.set_visibility([(99, False)])
    assert e.value.code == 1
    assert same_bits(a, g.render(spp=4, seed=6)[0]).all()
    g.close()


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_no_op(pkg, hip, builder):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    hs = hip.HipScene(sd, builder=builder)
    hs.set_visibility([(SHORT, False)])
    tree = hs.dump_bvh()
    for items in ([], [(SHORT, False)], [(SHORT, False), (TALL, True), (LIGHT, True)]):
        info = hs.set_visibility(items)
        assert info["build_ms"] == 0 and info["n_moved_tris"] == 0
        again = hs.dump_bvh()
        assert again[1].tobytes() == tree[1].tobytes() and again[2].tobytes() == tree[2].tobytes()
    assert np.array_equal(hs.visibility()[0], mask_hiding(sd, [SHORT]).astype(np.uint8))
