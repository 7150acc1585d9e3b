"""mcpt_scene_update on the GPU: after an update a scene behaves exactly like a scene freshly created from the moved description desc'
(the creation description with the current transforms applied by mcpt_transform_triangles) with the same build options.

With the host builders (sah, reference) that is bit for bit, the tree dump included.  With the device builders (lbvh, ploc) the rule of
tests/test_gpu_lbvh.py applies: hits equal ray for ray, a frame within 3 floats (a box-grazing ray may take another branch).  Every
comparison here is between the updated handle and a fresh scene; nothing is compared with a recorded number."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
INFO_FIELDS = ("n_nodes", "bvh_height", "quantised", "lds_resident", "n_lights", "n_prims")
DEVICE_BUILDERS = ("lbvh", "ploc")
# cornell_demo, Scene::Add order: floor, short box, tall box, left, right, light, glass sphere, plastic sphere, mirror sphere
FLOOR, SHORT, TALL, LIGHT, GLASS_SPHERE, PLASTIC_SPHERE, MIRROR_SPHERE = 0, 1, 2, 5, 6, 7, 8


def translate(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], f32)


def rotate_y(angle, centre, shift=(0, 0, 0)):
    """Rotation about the vertical axis through `centre`, then a translation."""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = np.asarray(centre, float) - R @ np.asarray(centre, float) + np.asarray(shift, float)
    return np.concatenate([R, t[:, None]], axis=1).astype(f32)


def reflect_x(cx):
    return np.array([[-1, 0, 0, 2 * cx], [0, 1, 0, 0], [0, 0, 1, 0]], f32)


def moved_scene(pkg, hip, sd, transforms):
    """desc': `transforms` maps object index -> 3x4 matrix (the CURRENT transform of every object that has one)."""
    tris, objs = sd.triangles.copy(), sd.objects.copy()
    for o, m in transforms.items():
        if objs["kind"][o] == 0:
            a, n = int(objs["first_tri"][o]), int(objs["n_tri"][o])
            tris[a:a + n] = hip.transform_triangles(m, np.ascontiguousarray(tris[a:a + n]))
        else:  # the centre goes through the same host function as a vertex
            one = np.zeros(1, pkg.scenes.TRI_DTYPE)
            one["v0"][0] = objs["center"][o]
            objs["center"][o] = hip.transform_triangles(m, one)["v0"][0]
    return dataclasses.replace(sd, triangles=tris, objects=objs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_frame(a, b, device_built, what=""):
    differing = int((~same_bits(a, b)).sum())
    assert differing <= (3 if device_built else 0), (what, differing)


def assert_same_hits(upd, fresh, o, d):
    ta, pa = upd.intersect(o, d)
    tb, pb = fresh.intersect(o, d)
    assert np.array_equal(pa, pb), "primitive ids differ on %d rays" % int((pa != pb).sum())
    assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    return pa


def assert_same_info(upd, fresh):
    a, b = upd.info(), fresh.info()
    assert [a[k] for k in INFO_FIELDS] == [b[k] for k in INFO_FIELDS], (a, b)


def assert_same_tree(upd, fresh):
    (ia, ba, ca, qa), (ib, bb, cb, qb) = upd.dump_bvh(), fresh.dump_bvh()
    for k in ia:
        assert np.array_equal(np.asarray(ia[k]), np.asarray(ib[k])), k
    assert ba.tobytes() == bb.tobytes() and ca.tobytes() == cb.tobytes()
    assert (qa is None) == (qb is None) and (qa is None or qa.tobytes() == qb.tobytes())


def cornell_rays(hs, W, H, spp, n_random=10000, seed=3):
    """The W x H x spp camera rays plus random rays through the box."""
    pix = np.repeat(np.arange(W * H, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), W * H)
    o, d = hs.camera_rays(pix, smp, seed=7)
    rng = np.random.default_rng(seed)
    o2 = rng.uniform([10, 10, -700], [540, 540, 540], (n_random, 3)).astype(f32)
    d2 = rng.normal(0, 1, (n_random, 3)).astype(f32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    return np.concatenate([o, o2]), np.concatenate([d, d2.astype(f32)])


THREE_MOVES = {SHORT: rotate_y(0.35, (185, 82, 169), shift=(25, 0, -30)), PLASTIC_SPHERE: translate(-60, 35, -90), TALL: reflect_x(368.0)}


@pytest.mark.parametrize("builder,quant", [("sah", -1), ("sah", 0), ("reference", 0), ("reference", 1), ("lbvh", -1), ("lbvh", 0), ("ploc", -1), ("ploc", 0)])
def test_update_equals_a_fresh_scene(pkg, hip, builder, quant):
    """One update moves a rotated and translated mesh, a translated sphere and a reflected mesh."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder, quantise=quant)
    before, _ = hs.render(spp=4, seed=5)
    info = hs.update(THREE_MOVES.items())
    assert info["path"] == (1 if dev else 0) and info["n_moved_tris"] == int(sd.objects["n_tri"][[SHORT, TALL]].sum())
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, THREE_MOVES), builder=builder, quantise=quant)
    assert_same_info(hs, fresh)
    if not dev:
        assert_same_tree(hs, fresh)
    o, d = cornell_rays(hs, 48, 48, 4)
    prim = assert_same_hits(hs, fresh, o, d)
    assert (prim >= 0).mean() > 0.5
    a, sa = hs.render(spp=4, seed=5)
    b, sb = fresh.render(spp=4, seed=5)
    assert_same_frame(a, b, dev, builder)
    assert abs(int(sa.vertices) - int(sb.vertices)) <= (3 if dev else 0)
    assert (~same_bits(a, before)).sum() > 100  # the objects did move
    # the other entry points that take the scene
    assert_same_frame(hs.render_aovs(aov_spp=2, seed=5, specular_depth=2), fresh.render_aovs(aov_spp=2, seed=5, specular_depth=2), dev, "aovs")
    n = 4000
    rng = np.random.default_rng(9)
    px, sm, ch = rng.integers(0, 48 * 48, n).astype(np.uint32), rng.integers(0, 64, n).astype(np.uint32), rng.integers(0, 3, n).astype(np.int32)
    co, cd = hs.camera_rays(px, sm, seed=2)
    bad = ~same_bits(hs.cast_rays(co, cd, px, sm, ch, seed=2), fresh.cast_rays(co, cd, px, sm, ch, seed=2))
    assert bad.sum() <= (2 if dev else 0)


@pytest.mark.parametrize("builder", ["sah", "reference", "lbvh", "ploc"])
def test_moving_the_light_takes_the_host_path(pkg, hip, builder):
    """The light tables, the emitters' bounding sphere and the half-space rule's plane are host-built: an emissive object moves on path 0."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    dev = builder in DEVICE_BUILDERS
    moves = {LIGHT: rotate_y(0.5, (278, 548, 279), shift=(-70, -45, 40))}
    hs = hip.HipScene(sd, builder=builder)
    assert hs.update(moves.items())["path"] == 0
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, moves), builder=builder)
    u = np.random.default_rng(2).uniform(0, 1, (2000, 4)).astype(f32)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()
    assert not same_bits(hs.sample_light(u), hip.HipScene(sd, builder=builder).sample_light(u)).all()
    assert_same_info(hs, fresh)
    a, _ = hs.render(spp=4, seed=8)
    b, _ = fresh.render(spp=4, seed=8)
    assert_same_frame(a, b, dev, builder)
    # and a later update on the device path starts from what the host path left
    both = dict(moves)
    both[SHORT] = THREE_MOVES[SHORT]
    assert hs.update([(SHORT, THREE_MOVES[SHORT])])["path"] == (1 if dev else 0)
    fresh2 = hip.HipScene(moved_scene(pkg, hip, sd, both), builder=builder)
    assert same_bits(hs.sample_light(u), fresh2.sample_light(u)).all()
    c, _ = hs.render(spp=4, seed=8)
    e, _ = fresh2.render(spp=4, seed=8)
    assert_same_frame(c, e, dev, builder)


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_transforms_are_absolute(pkg, hip, builder):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    dev = builder in DEVICE_BUILDERS
    T1, T2 = translate(40, 0, 60), rotate_y(-0.6, (185, 82, 169), shift=(0, 20, 0))
    TA = translate(-30, 0, -50)
    hs = hip.HipScene(sd, builder=builder)
    original = hip.HipScene(sd, builder=builder)
    o, d = cornell_rays(hs, 48, 48, 4)
    hs.update([(SHORT, T1)])
    hs.update([(SHORT, T2)])
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, {SHORT: T2}), builder=builder)  # T2 alone: T1 left nothing behind
    assert_same_hits(hs, fresh, o, d)
    assert_same_frame(hs.render(spp=4, seed=1)[0], fresh.render(spp=4, seed=1)[0], dev)
    hs.update([(TALL, TA), (MIRROR_SPHERE, translate(0, -100, 0))])  # SHORT is not listed: it keeps T2
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, {SHORT: T2, TALL: TA, MIRROR_SPHERE: translate(0, -100, 0)}), builder=builder)
    assert_same_info(hs, fresh)
    prim = assert_same_hits(hs, fresh, o, d)
    assert_same_frame(hs.render(spp=4, seed=1)[0], fresh.render(spp=4, seed=1)[0], dev)
    if not dev:
        assert_same_tree(hs, fresh)
    # objects never listed still have their creation-time records: rays that reach them hit as in the original scene, bit for bit
    t0, p0 = original.intersect(o, d)
    t1, _ = hs.intersect(o, d)
    first, n = sd.objects["first_tri"], sd.objects["n_tri"]
    never = np.zeros(len(sd.triangles) + len(sd.objects), bool)
    for ob in (FLOOR, 3, 4, LIGHT):
        never[first[ob]:first[ob] + n[ob]] = True
    never[len(sd.triangles) + GLASS_SPHERE] = never[len(sd.triangles) + PLASTIC_SPHERE] = True
    sel = (prim >= 0) & (prim == p0) & never[np.maximum(prim, 0)]
    assert sel.sum() > 5000 and np.array_equal(t0[sel].view(np.uint64), t1[sel].view(np.uint64))
    assert hs.update([])["n_moved_tris"] == 0  # n == 0: a valid no-op
    assert_same_hits(hs, fresh, o, d)


def _scene_65(pkg):
    """One triangle more than the LDS-resident kernels hold (kSmallTris = 64): 63 triangles and a two-triangle light."""
    s = pkg.scenes
    P = s.material_presets()
    b = s._Builder()
    rng = np.random.default_rng(1)
    tri = np.zeros(63, s.TRI_DTYPE)
    base = rng.uniform(-20, 20, (63, 3)).astype(f32)
    tri["v0"], tri["v1"], tri["v2"] = base, base + rng.normal(0, 4, (63, 3)).astype(f32), base + rng.normal(0, 4, (63, 3)).astype(f32)
    b.add_mesh(tri, b.material("rough_plastic", P["rough_plastic"]))
    lt = np.zeros(2, s.TRI_DTYPE)
    lt["v0"], lt["v1"], lt["v2"] = [(-10, 40, -10)] * 2, [(10, 40, -10), (10, 40, 10)], [(10, 40, 10), (-10, 40, 10)]
    b.add_mesh(lt, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(20, 20, 20))))
    cam = s.make_camera(48, 32, 60, (0, 0, -70), (0, 0, 0))
    return b.finish(camera=cam, rr_rate=0.5, spp=2, name="65 triangles")


@pytest.mark.parametrize("small", [True, False])
def test_lds_resident_flavour_survives_an_update(pkg, hip, monkeypatch, small):
    if small:
        monkeypatch.delenv("MCPT_SMALL_SCENE", raising=False)
    else:
        monkeypatch.setenv("MCPT_SMALL_SCENE", "0")
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    for builder in ("sah", "lbvh"):  # (the PLOC tree of this scene has 11 levels: more than the LDS-resident kernels' stack holds)
        hs = hip.HipScene(sd, builder=builder)
        assert hs.info()["lds_resident"] == (1 if small else 0)
        hs.update(THREE_MOVES.items())
        if builder == "sah" or not small:  # (the height of a rebuilt LBVH is the builder's: the comparison with the fresh scene below decides)
            assert hs.info()["lds_resident"] == (1 if small else 0)
        fresh = hip.HipScene(moved_scene(pkg, hip, sd, THREE_MOVES), builder=builder)
        assert_same_info(hs, fresh)
        o, d = cornell_rays(hs, 48, 48, 1, n_random=4000)
        assert_same_hits(hs, fresh, o, d)
        assert_same_frame(hs.render(spp=4, seed=3)[0], fresh.render(spp=4, seed=3)[0], builder in DEVICE_BUILDERS, builder)


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_scene_one_triangle_beyond_the_lds_limit(pkg, hip, monkeypatch, builder):
    monkeypatch.delenv("MCPT_SMALL_SCENE", raising=False)
    sd = _scene_65(pkg)
    moves = {0: rotate_y(0.8, (0, 0, 0), shift=(3, -2, 5))}
    hs = hip.HipScene(sd, builder=builder)
    assert hs.info()["lds_resident"] == 0
    assert hs.update(moves.items())["path"] == (1 if builder == "lbvh" else 0)
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, moves), builder=builder)
    assert hs.info()["lds_resident"] == 0
    assert_same_info(hs, fresh)
    rng = np.random.default_rng(4)
    o = rng.uniform(-60, 60, (6000, 3)).astype(f32)
    d = (rng.uniform(-20, 20, (6000, 3)) - o).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    prim = assert_same_hits(hs, fresh, o, d)
    assert (prim >= 0).sum() > 200
    assert_same_frame(hs.render(spp=2, seed=1)[0], fresh.render(spp=2, seed=1)[0], builder == "lbvh")


def test_chess_pieces_move_on_the_device_path(pkg, hip):
    """The chess scene (38 k triangles, many workgroups of the update kernel) with the PLOC builder: the king and a glass pawn move."""
    sd = pkg.scenes.chess_scene(width=96, height=54, spp=2)
    KING, PAWN = 16, 0
    assert sd.objects["n_tri"][KING] > 1000 and sd.materials["type"][sd.objects["material"][PAWN]] == 2  # a mesh; smooth glass
    moves = {KING: rotate_y(0.9, (0, 0, 0), shift=(120, 0, -300)), PAWN: translate(35, 0, 180)}
    hs = hip.HipScene(sd, builder="ploc")
    before, _ = hs.render(spp=2, seed=4)
    assert np.isfinite(before).all()
    info = hs.update(moves.items())
    assert info["path"] == 1 and info["n_moved_tris"] == int(sd.objects["n_tri"][[KING, PAWN]].sum())
    after, _ = hs.render(spp=2, seed=4)
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, moves), builder="ploc")
    assert_same_info(hs, fresh)
    assert_same_frame(after, fresh.render(spp=2, seed=4)[0], True)
    assert (~same_bits(after, before)).sum() > 0  # (the two pieces cover few pixels of a 96 x 54 frame; the frame did change)
    bi, _, _, _ = hs.dump_bvh()
    rng = np.random.default_rng(6)
    lo, hi = np.array(bi["root_min"], f32), np.array(bi["root_max"], f32)
    o = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), size=(10000, 3)).astype(f32)
    d = rng.uniform(lo, hi, size=(10000, 3)).astype(f32) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    prim = assert_same_hits(hs, fresh, o, d)
    assert (prim >= 0).mean() > 0.2


def test_refused_updates_leave_the_scene_as_it_was(pkg, hip):
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    for builder in ("sah", "ploc"):
        hs = hip.HipScene(sd, builder=builder)
        hs.update([(SHORT, THREE_MOVES[SHORT])])
        frame, _ = hs.render(spp=4, seed=2)
        nan = translate(1, 2, 3)
        nan[1, 2] = np.nan
        for bad in ([(len(sd.objects), translate(1, 0, 0))], [(-1, translate(1, 0, 0))], [(TALL, translate(1, 0, 0)), (TALL, translate(2, 0, 0))],
                    [(TALL, translate(50, 0, 0)), (SHORT, nan)]):
            with pytest.raises(hip.McptError) as e:
                hs.update(bad)
            assert e.value.code == 1
            again, _ = hs.render(spp=4, seed=2)
            assert same_bits(frame, again).all(), bad
    chess = pkg.scenes.chess_scene(width=64, height=36, spp=1)
    inst = hip.HipScene(chess, builder="sah", instancing=True)
    assert inst.info()["n_instances"] == 14
    frame, _ = inst.render(spp=1, seed=2)
    with pytest.raises(hip.McptError) as e:
        inst.update([(16, translate(10, 0, 0))])
    assert e.value.code == 1 and "instancing" in str(e.value)
    assert same_bits(frame, inst.render(spp=1, seed=2)[0]).all()


def test_group_update(pkg, hip):
    """Two replicas on one device: mcpt_group_update, then mcpt_group_render, equals mcpt_render of the updated single scene."""
    sd = pkg.scenes.cornell_demo(64, 48, 4)
    moves = dict(THREE_MOVES)
    moves[LIGHT] = translate(-40, -30, 20)
    g = hip.HipGroup(sd, [0, 0])
    g.update(moves.items())
    hs = hip.HipScene(sd)
    hs.update(moves.items())
    a, _ = g.render(spp=4, seed=6)
    b, _ = hs.render(spp=4, seed=6)
    assert same_bits(a, b).all()
    with pytest.raises(hip.McptError) as e:
        g.update([(99, translate(1, 0, 0))])
    assert e.value.code == 1
    assert same_bits(a, g.render(spp=4, seed=6)[0]).all()
    g.close()


def test_direct_lighting_skips_stay_zero_after_an_update(pkg, hip, hip_check):
    """The checking build evaluates the light samples at vertices the product skips: none may contribute after the light-facing geometry and
    the light itself have moved (the half-space rule's plane and the emitters' bounding sphere follow the update)."""
    sd = pkg.scenes.cornell_demo(48, 48, 4)
    hc = hip.HipScene(sd, library=hip_check)
    assert b"checking build" in hc.L.mcpt_version()
    hc.update(THREE_MOVES.items())
    hc.update([(LIGHT, rotate_y(0.5, (278, 548, 279), shift=(-70, -45, 40)))])
    fb, _ = hc.render(spp=4, seed=3)
    c = hc.debug_counters()
    assert int(c[14]) > 0 and int(c[15]) == 0, [int(x) for x in c]
    both = dict(THREE_MOVES)
    both[LIGHT] = rotate_y(0.5, (278, 548, 279), shift=(-70, -45, 40))
    fresh = hip.HipScene(moved_scene(pkg, hip, sd, both), library=hip_check)
    assert same_bits(fb, fresh.render(spp=4, seed=3)[0]).all()
    hc.close()
