"""mcpt_scene_add_objects on the GPU: after the call a scene behaves like a scene freshly created from extend(desc', addition), the
current description followed by the added objects (mcpt_extend_scene), with the same build options -- compacted with the current mask
when something is hidden.

The comparison rules are those of tests/deform_cases.py, unchanged: with the host builders (sah, reference) bit for bit, the tree dump
included; with the device builders (lbvh, ploc) hits equal ray for ray and a frame within 3 floats.  Every comparison is between the
edited handle and a fresh scene; nothing is compared with a recorded number.  Frames are 64 x 64 at 4 samples per pixel."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from add_cases import extend_numpy, ids_of, reordered, same_description, split  # noqa: E402
from deform_cases import (DEVICE_BUILDERS, PX_TOL, STRIP_SIZES, assert_equals_fresh, assert_same_frame, camera_and_random_rays, cornell_rays,  # noqa: E402
                          deformed_scene, object_positions, rotate_y, same_bits, strips_scene, translate, wave)

pytestmark = pytest.mark.gpu

f32 = np.float32
# cornell_demo, Scene::Add order: floor, short box, tall box, left, right, light, glass sphere, plastic sphere, mirror sphere
FLOOR, SHORT, TALL, LEFT, RIGHT, LIGHT, GLASS_SPHERE, PLASTIC_SPHERE, MIRROR_SPHERE = range(9)
W = H = 64
SPP = 4
TREE_FIELDS = ("n_nodes", "bvh_height", "quantised", "n_lights")  # (with something hidden, n_prims and lds_resident follow the stored records)
BUILDERS8 = [("sah", -1), ("sah", 0), ("reference", 0), ("reference", 1), ("lbvh", -1), ("lbvh", 0), ("ploc", -1), ("ploc", 0)]


@pytest.fixture(scope="module")
def cornell(pkg):
    return pkg.scenes.cornell_demo(W, H, SPP)


def green(pkg, textured=0):
    s = pkg.scenes
    return s._mat(s.ROUGH_CONDUCTOR, 0.2, (0.2, 0.9, 0.3), textured=textured)


def path_of(builder, emitter=False):
    return 1 if builder in DEVICE_BUILDERS and not emitter else 0


@pytest.mark.parametrize("builder,quant", BUILDERS8)
def test_added_objects_equal_a_fresh_scene(pkg, hip, cornell, builder, quant):
    """cornell_demo without the short box and the plastic sphere; both are added in one call, the box with a new material."""
    dev = builder in DEVICE_BUILDERS
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    objs["material"][0] = len(kept.materials)
    mats = [green(pkg)]
    hs = hip.HipScene(kept, builder=builder, quantise=quant)
    before, _ = hs.render(spp=SPP, seed=5)
    first, info = hs.add_objects(objs, tris, mats)
    assert first == len(kept.objects) and info["path"] == path_of(builder) and info["n_moved_tris"] == len(tris)
    want = extend_numpy(kept, objs, tris, mats)
    assert same_description(hs.sd, want)
    moved_back = reordered(hip, cornell, [SHORT, PLASTIC_SPHERE])  # the reordered description, but for the box's new material
    assert want.triangles.tobytes() == moved_back.triangles.tobytes() and np.array_equal(want.objects["first_tri"], moved_back.objects["first_tri"])
    fresh = hip.HipScene(want, builder=builder, quantise=quant)
    o, d = cornell_rays(hs, W, H, SPP)
    prim = assert_equals_fresh(hs, fresh, o, d, dev, spp=SPP, seed=5, what=builder)
    for k in range(2):  # both added objects are seen, under the ids of the extended description
        assert np.isin(prim, ids_of(want, first + k)).sum() > 50
    assert (~same_bits(before, hs.render(spp=SPP, seed=5)[0])).sum() > 100
    a, b = hs.render_aovs(aov_spp=2, seed=5), fresh.render_aovs(aov_spp=2, seed=5)  # normals, albedo (the new material), depth
    assert_same_frame(a, b, dev, "aovs")
    u = np.random.default_rng(2).uniform(0, 1, (500, 4)).astype(f32)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()  # the light tables stay valid: triangle ids of old objects are stable
    mask, n_vis = hs.visibility()
    assert mask.all() and len(mask) == len(want.objects) and n_vis == len(want.triangles) + int((want.objects["kind"] == 1).sum())


@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_added_triangles_beside_a_sphere_light(pkg, hip, cornell, builder):
    """The kept scene holds an emissive sphere.  A mesh that does not emit is added (path 1 on the device builders: the light tables stay
    where they are), so the sphere light's primitive id, n_triangles + object, moves up under a LightRec that did not change."""
    dev = builder in DEVICE_BUILDERS
    mats = cornell.materials.copy()
    glow = int(cornell.objects["material"][PLASTIC_SPHERE])
    assert (cornell.objects["material"] == glow).sum() == 1
    mats["emission"][glow] = (4, 3, 2)
    sd = dataclasses.replace(cornell, materials=mats)
    kept, (objs, tris) = split(hip, sd, [SHORT])
    ball = PLASTIC_SPHERE - 1  # its place in `kept`
    hs = hip.HipScene(kept, builder=builder)
    assert hs.info()["n_lights"] == 2
    o, d = cornell_rays(hs, W, H, SPP)
    assert (hs.intersect(o, d)[1] == len(kept.triangles) + ball).sum() > 50
    first, info = hs.add_objects(objs, tris)
    assert info["path"] == path_of(builder) and hs.info()["n_lights"] == 2
    want = extend_numpy(kept, objs, tris)
    fresh = hip.HipScene(want, builder=builder)
    prim = assert_equals_fresh(hs, fresh, o, d, dev, spp=SPP, seed=5, what=builder)
    assert (prim == len(want.triangles) + ball).sum() > 50 and len(want.triangles) > len(kept.triangles)
    u = np.random.default_rng(2).uniform(0, 1, (1000, 4)).astype(f32)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()
    assert_same_frame(hs.render_aovs(aov_spp=2, seed=5), fresh.render_aovs(aov_spp=2, seed=5), dev, "aovs")


@pytest.mark.parametrize("builder", DEVICE_BUILDERS)
def test_segment_edges(pkg, hip, builder):
    """Floor and light only; the strips of 1, 63, 64, 65 and 257 triangles arrive in one call: segment borders inside a wave, on a wave's
    edge and across the 256-lane block.  Their material is textured and they carry texture coordinates, so every word of both records
    decides what a hit or a pixel shows."""
    sd = strips_scene(pkg, W, H)
    strips = list(range(len(STRIP_SIZES)))
    kept, (objs, tris) = split(hip, sd, strips)
    assert [int(n) for n in objs["n_tri"]] == list(STRIP_SIZES) and np.abs(tris["t1"]).max() > 0
    objs["material"][:] = len(kept.materials)
    mats = [green(pkg, textured=1)]
    hs = hip.HipScene(kept, builder=builder)
    first, info = hs.add_objects(objs, tris, mats)
    assert info["path"] == 1 and info["n_moved_tris"] == sum(STRIP_SIZES) and first == 2
    want = extend_numpy(kept, objs, tris, mats)
    fresh = hip.HipScene(want, builder=builder)
    o, d = camera_and_random_rays(hs, W, H, SPP, [-420, -50, -100], [420, 60, 30])
    eye = np.array([0, 10, -420], f32)  # and one ray from the camera at the centroid of every added triangle
    aim = ((tris["v0"] + tris["v1"] + tris["v2"]) / f32(3) - eye).astype(np.float64)
    aim = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(f32)
    o, d = np.concatenate([o, np.tile(eye, (len(aim), 1))]), np.concatenate([d, aim])
    prim = assert_equals_fresh(hs, fresh, o, d, True, spp=SPP, seed=5, what=builder)
    seen = np.isin(np.arange(len(kept.triangles), len(want.triangles)), prim)
    assert seen.mean() > 0.9, seen.mean()  # (a strip's neighbour may be nearer along the ray at a shared corner)
    for k in range(len(STRIP_SIZES)):
        assert np.isin(prim, ids_of(want, first + k)).any(), k
    assert_same_frame(hs.render_aovs(aov_spp=2, seed=5), fresh.render_aovs(aov_spp=2, seed=5), True, "aovs")


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_later_edits_act_on_added_objects(pkg, hip, cornell, builder):
    dev = builder in DEVICE_BUILDERS
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    hs = hip.HipScene(kept, builder=builder)
    first, _ = hs.add_objects(objs, tris)
    sd = extend_numpy(kept, objs, tris)
    box, ball = first, first + 1
    o, d = cornell_rays(hs, W, H, SPP, n_random=3000)

    def check(sd_now, what, mask=None):
        if mask is None:
            assert_equals_fresh(hs, hip.HipScene(sd_now, builder=builder), o, d, dev, spp=SPP, seed=5, what=what)
            return
        # hidden: the compacted fresh scene, live ids translated through prim_map as tests/test_gpu_scene_visibility.py does
        compacted, prim_map = hip.compact_scene(sd_now, mask)
        fresh = hip.HipScene(compacted, builder=builder)
        a, b = hs.info(), fresh.info()
        assert [a[k] for k in TREE_FIELDS] == [b[k] for k in TREE_FIELDS], (a, b)
        ta, pa = hs.intersect(o, d)
        tb, pb = fresh.intersect(o, d)
        assert np.array_equal(np.where(pa >= 0, prim_map[np.maximum(pa, 0)], pa), pb) and np.array_equal(ta.view(np.uint64), tb.view(np.uint64)), what
        assert_same_frame(hs.render(spp=SPP, seed=5)[0], fresh.render(spp=SPP, seed=5)[0], dev, what)

    turn = rotate_y(0.3, (185, 82, 169), shift=(20, 0, -30))
    assert hs.update([(box, turn), (ball, translate(-30, 10, 0))])["path"] == path_of(builder)
    moves = {box: turn, ball: translate(-30, 10, 0)}
    check(deformed_scene(pkg, hip, sd, {}, moves), "update")
    P = wave(object_positions(sd, box), amp=8.0)
    assert hs.deform([(box, P)])["path"] == path_of(builder)
    check(deformed_scene(pkg, hip, sd, {box: P}, moves), "deform")
    mats = sd.objects.copy()
    cur = int(sd.objects["material"][box])
    mats["material"][box] = next(m for m in range(len(sd.materials)) if m != cur and not sd.materials["emission"][m].any())
    assert hs.set_materials(assign=[(box, int(mats["material"][box]))])["path"] == 2
    sd2 = dataclasses.replace(sd, objects=mats)
    check(deformed_scene(pkg, hip, sd2, {box: P}, moves), "material")
    mask = np.ones(len(sd.objects), bool)
    mask[box] = False
    assert hs.set_visibility([(box, False)])["path"] == path_of(builder)
    check(deformed_scene(pkg, hip, sd2, {box: P}, moves), "hidden", mask)
    assert hs.set_visibility([(box, True)])["path"] == path_of(builder)
    check(deformed_scene(pkg, hip, sd2, {box: P}, moves), "shown")


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_add_while_hidden_and_moved(pkg, hip, cornell, builder):
    """The tall box is hidden and the glass sphere has moved when the addition arrives: mask and transforms survive."""
    dev = builder in DEVICE_BUILDERS
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    tall, glass = TALL - 1, GLASS_SPHERE - 1  # their places in `kept`
    hs = hip.HipScene(kept, builder=builder)
    hs.set_visibility([(tall, False)])
    move = translate(40, 20, -30)
    hs.update([(glass, move), (LEFT - 1, translate(-5, 0, 0))])
    first, info = hs.add_objects(objs, tris)
    assert info["path"] == path_of(builder)
    mask, _ = hs.visibility()
    want_mask = np.ones(len(kept.objects) + 2, bool)
    want_mask[tall] = False
    assert np.array_equal(mask.astype(bool), want_mask)
    now = deformed_scene(pkg, hip, extend_numpy(kept, objs, tris), {}, {glass: move, LEFT - 1: translate(-5, 0, 0)})
    compacted, prim_map = hip.compact_scene(now, want_mask)
    fresh = hip.HipScene(compacted, builder=builder)
    a, b = hs.info(), fresh.info()
    assert [a[k] for k in TREE_FIELDS] == [b[k] for k in TREE_FIELDS], (a, b)
    o, d = cornell_rays(hs, W, H, SPP, n_random=3000)
    ta, pa = hs.intersect(o, d)
    tb, pb = fresh.intersect(o, d)
    assert np.array_equal(np.where(pa >= 0, prim_map[np.maximum(pa, 0)], pa), pb) and np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    assert_same_frame(hs.render(spp=SPP, seed=5)[0], fresh.render(spp=SPP, seed=5)[0], dev, builder)
    hs.set_visibility([(tall, True)])  # and shown again it equals the plain extended scene
    assert_equals_fresh(hs, hip.HipScene(now, builder=builder), o, d, dev, spp=SPP, seed=5, what="shown")


def small_scene(pkg, n_tri=60, n_extra_objects=0):
    """n_tri triangles in one mesh and a two-triangle light, in the style of deform_cases.scene_65; n_extra_objects one-triangle meshes."""
    s = pkg.scenes
    P = s.material_presets()
    b = s._Builder()
    rng = np.random.default_rng(1)
    tri = np.zeros(n_tri, s.TRI_DTYPE)
    base = rng.uniform(-20, 20, (n_tri, 3)).astype(f32)
    tri["v0"], tri["v1"], tri["v2"] = base, base + rng.normal(0, 4, (n_tri, 3)).astype(f32), base + rng.normal(0, 4, (n_tri, 3)).astype(f32)
    b.add_mesh(tri, b.material("rough_plastic", P["rough_plastic"]))
    lt = np.zeros(2, s.TRI_DTYPE)
    lt["v0"], lt["v1"], lt["v2"] = [(-10, 40, -10)] * 2, [(10, 40, -10), (10, 40, 10)], [(10, 40, 10), (-10, 40, 10)]
    b.add_mesh(lt, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(20, 20, 20))))
    for k in range(n_extra_objects):
        b.add_mesh(random_triangles(pkg, 1, seed=100 + k), b.material("rough_plastic", P["rough_plastic"]))
    cam = s.make_camera(W, H, 60, (0, 0, -70), (0, 0, 0))
    return b.finish(camera=cam, rr_rate=0.5, spp=SPP, name="small")


def random_triangles(pkg, n, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, pkg.scenes.TRI_DTYPE)
    base = rng.uniform(-20, 20, (n, 3)).astype(f32)
    t["v0"], t["v1"], t["v2"] = base, base + rng.normal(0, 4, (n, 3)).astype(f32), base + rng.normal(0, 4, (n, 3)).astype(f32)
    return t


def mesh_object(pkg, n_tri, material):
    o = np.zeros(1, pkg.scenes.OBJ_DTYPE)
    o["kind"], o["material"], o["first_tri"], o["n_tri"] = 0, material, 0, n_tri
    return o


def sphere_object(pkg, centre, radius, material):
    o = np.zeros(1, pkg.scenes.OBJ_DTYPE)
    o["kind"], o["material"], o["center"], o["radius"] = 1, material, np.asarray(centre, f32), f32(radius)
    return o


@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("n_add,resident", [(1, 1), (2, None), (3, 0)])
def test_lds_boundary_triangles(pkg, hip, builder, n_add, resident):
    """62 stored triangles; the LDS-resident kernels hold 64: 63 stay resident, 65 do not.  At 64, the limit itself, the height of the new tree
    decides as well (kSmallStk), so that case is held against the fresh scene alone."""
    sd = small_scene(pkg)
    assert len(sd.triangles) == 62
    hs = hip.HipScene(sd, builder=builder)
    assert hs.info()["lds_resident"] == 1
    tris = random_triangles(pkg, n_add, seed=7)
    hs.add_objects(mesh_object(pkg, n_add, 0), tris)
    assert resident is None or hs.info()["lds_resident"] == resident
    fresh = hip.HipScene(extend_numpy(sd, mesh_object(pkg, n_add, 0), tris), builder=builder)
    o, d = camera_and_random_rays(hs, W, H, SPP, [-30, -30, -70], [30, 45, 30], n_random=3000)
    assert_equals_fresh(hs, fresh, o, d, builder in DEVICE_BUILDERS, spp=SPP, seed=5, what=builder)


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_lds_boundary_sphere_slots(pkg, hip, builder):
    """One SphereRec slot per object: 16 objects are resident, the 17th ends that."""
    sd = small_scene(pkg, n_tri=20, n_extra_objects=14)
    assert len(sd.objects) == 16
    hs = hip.HipScene(sd, builder=builder)
    assert hs.info()["lds_resident"] == 1
    ball = sphere_object(pkg, (5, -5, 0), 6.0, 0)
    first, _ = hs.add_objects(ball, None)
    assert first == 16 and hs.info()["lds_resident"] == 0
    fresh = hip.HipScene(extend_numpy(sd, ball, None), builder=builder)
    o, d = camera_and_random_rays(hs, W, H, SPP, [-30, -30, -70], [30, 45, 30], n_random=3000)
    prim = assert_equals_fresh(hs, fresh, o, d, builder in DEVICE_BUILDERS, spp=SPP, seed=5, what=builder)
    assert (prim == len(sd.triangles) + 16).sum() > 50


@pytest.mark.parametrize("builder", ["sah", "reference", "lbvh", "ploc"])
@pytest.mark.parametrize("kind", ["mesh", "sphere"])
def test_added_emitters_take_the_host_path(pkg, hip, cornell, builder, kind):
    s = pkg.scenes
    dev = builder in DEVICE_BUILDERS
    glow = s._mat(s.ROUGH_CONDUCTOR, emission=(6, 5, 4))
    M = len(cornell.materials)
    if kind == "mesh":
        lt = np.zeros(2, s.TRI_DTYPE)
        lt["v0"], lt["v1"], lt["v2"] = [(100, 300, 100)] * 2, [(180, 300, 100), (180, 300, 180)], [(180, 300, 180), (100, 300, 180)]
        objs, tris = mesh_object(pkg, 2, M), lt
    else:
        objs, tris = sphere_object(pkg, (400, 300, 150), 35.0, M), None
    hs = hip.HipScene(cornell, builder=builder)
    assert hs.info()["n_lights"] == 1
    first, info = hs.add_objects(objs, tris, [glow])
    assert info["path"] == 0 and hs.info()["n_lights"] == 2
    fresh = hip.HipScene(extend_numpy(cornell, objs, tris, [glow]), builder=builder)
    o, d = cornell_rays(hs, W, H, SPP, n_random=3000)
    assert_equals_fresh(hs, fresh, o, d, dev, spp=SPP, seed=5, what=builder)
    u = np.random.default_rng(2).uniform(0, 1, (1000, 4)).astype(f32)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()
    if dev:  # a non-emitter afterwards goes back to the device path, from what the host path left
        ball = sphere_object(pkg, (150, 60, 100), 40.0, 0)
        assert hs.add_objects(ball, None)[1]["path"] == 1
        fresh2 = hip.HipScene(extend_numpy(extend_numpy(cornell, objs, tris, [glow]), ball, None), builder=builder)
        assert_equals_fresh(hs, fresh2, o, d, dev, spp=SPP, seed=5, what=builder)


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_snapshot_is_extended(pkg, hip, cornell, builder):
    """Move, snapshot, move again, add: the motion pass indexes the snapshot by live primitive id, so it must have grown with the scene; the
    added objects are in it as added, at rest."""
    dev = builder in DEVICE_BUILDERS
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    tall, glass = TALL - 1, GLASS_SPHERE - 1
    m1 = {tall: translate(-10, 0, 5), glass: translate(0, 12, 0)}
    m2 = {tall: translate(-40, 0, 25), glass: translate(15, 30, -10)}
    hs = hip.HipScene(kept, builder=builder)
    hs.update(list(m1.items()))
    hs.snapshot()
    hs.update(list(m2.items()))
    first, _ = hs.add_objects(objs, tris)
    want = extend_numpy(kept, objs, tris)
    fresh = hip.HipScene(want, builder=builder)
    fresh.update(list(m1.items()))
    fresh.snapshot()
    fresh.update(list(m2.items()))
    a, b = hs.render_motion(seed=5, aov_spp=SPP), fresh.render_motion(seed=5, aov_spp=SPP)
    assert_same_frame(a, b, dev, "motion")
    # pixels whose every sample hits an added object: valid, and no object motion under a camera that does not move
    pix, smp = np.repeat(np.arange(W * H, dtype=np.uint32), SPP), np.tile(np.arange(SPP, dtype=np.uint32), W * H)
    o, d = hs.camera_rays(pix, smp, seed=5)
    _, prim = hs.intersect(o, d)
    added = np.concatenate([ids_of(want, first), ids_of(want, first + 1)])
    moved = np.concatenate([ids_of(want, tall), ids_of(want, glass)])
    on_added = np.isin(prim, added).reshape(H, W, SPP).all(-1)
    on_moved = np.isin(prim, moved).reshape(H, W, SPP).all(-1)
    assert on_added.sum() > 50 and on_moved.sum() > 50
    assert (a[on_added][:, 3] == 1).all() and np.abs(a[on_added][:, 0:2]).max() < PX_TOL
    assert np.abs(a[on_moved][:, 0:2]).max() > 1.0  # (the objects that did move report it)
    # the next snapshot has the new size
    hs.snapshot()
    fresh.snapshot()
    assert_same_frame(hs.render_motion(seed=6, aov_spp=2), fresh.render_motion(seed=6, aov_spp=2), dev, "motion after the next snapshot")


def test_a_sequence_survives(pkg, hip, cornell):
    """Live: frame, add X, frame.  Control: a scene of the extended description with X hidden takes frame, show X, frame.  Every output of both
    frames is bit-identical (sah)."""
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    want = extend_numpy(kept, objs, tris)
    n = len(kept.objects)
    outputs = ("fb", "accumulated", "denoised", "variance", "len", "aov", "motion", "rgba")
    live = hip.HipScene(kept, builder="sah")
    control = hip.HipScene(want, builder="sah")
    control.set_visibility([(n, False), (n + 1, False)])
    sl, sc = live.sequence(W, H), control.sequence(W, H)
    f1, g1 = sl.frame(want=outputs, spp=SPP, seed=1), sc.frame(want=outputs, spp=SPP, seed=1)
    live.add_objects(objs, tris)
    control.set_visibility([(n, True), (n + 1, True)])
    f2, g2 = sl.frame(want=outputs, spp=SPP, seed=2), sc.frame(want=outputs, spp=SPP, seed=2)
    for k in outputs:
        assert f1[k].tobytes() == g1[k].tobytes(), ("frame 1", k)
        assert f2[k].tobytes() == g2[k].tobytes(), ("frame 2", k)
    assert f2["info"]["frame_index"] == 1 and (f2["len"] > 1).mean() > 0.5  # the history was kept
    assert not np.array_equal(f1["fb"], f2["fb"])
    assert live.info()["n_prims"] == control.info()["n_prims"] == len(want.triangles) + len(want.objects)
    sl.close()
    sc.close()


def test_refusals_change_nothing(pkg, hip, cornell):
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    n_short = int(objs["n_tri"][0])

    def with_objects(field, ob, value):
        o2 = objs.copy()
        o2[field][ob] = value
        return o2, tris, None

    def with_vertex(field, value):
        t2 = tris.copy()
        t2[field][3, 1] = value
        return objs, t2, None

    centre = objs.copy()
    centre["center"][1] = (np.inf, 0, 0)
    bad_type = green(pkg)
    bad_type["type"] = -1
    cases = [with_objects("first_tri", 0, 1), with_objects("n_tri", 0, n_short + 1), with_objects("n_tri", 0, 0), with_objects("kind", 1, 5),
             with_objects("material", 0, len(kept.materials)), with_objects("material", 1, -1), with_objects("radius", 1, np.nan), (centre, tris, None),
             (np.concatenate([objs[:1], objs[:1]]), tris, None), with_vertex("v0", np.nan), with_vertex("v2", np.inf), (objs[:0], tris, None),
             (objs, tris, [bad_type])]
    for builder in ("sah", "ploc"):
        hs = hip.HipScene(kept, builder=builder)
        hs.snapshot()
        frame, _ = hs.render(spp=SPP, seed=2)
        tree = hs.dump_bvh()
        info = hs.info()

        def unchanged(what):
            assert len(hs.visibility()[0]) == len(kept.objects), what
            again = hs.dump_bvh()
            assert again[1].tobytes() == tree[1].tobytes() and again[2].tobytes() == tree[2].tobytes(), what
            assert hs.info() == info and same_bits(frame, hs.render(spp=SPP, seed=2)[0]).all(), what

        for k, (o, t, m) in enumerate(cases):
            with pytest.raises(hip.McptError) as e:
                hs.add_objects(o, t, m)
            assert e.value.code == 1 and "mcpt_scene_add_objects" in str(e.value), k
            assert hs.sd is kept
            unchanged(k)
        # what the wrapper cannot express: negative counts, a null array, a reserved word, totals beyond int32, null arguments
        for fields in ({"n_objects": -1}, {"n_triangles": -2}, {"n_materials": -1}, {"objects": None}, {"triangles": None}, {"n_triangles": 0x7fffffff},
                       {"n_objects": 0x7ffffff0}, {"reserved": (C.c_int32 * 4)(0, 0, 0, 9)}):
            a, keep = hip._addition(kept, objs, tris, None)
            for f, v in fields.items():
                setattr(a, f, v)
            assert hs.L.mcpt_scene_add_objects(hs.h, C.byref(a), None, None) == 1, fields
            unchanged(fields)
        a, keep = hip._addition(kept, objs, tris, None)
        a.n_materials = 1  # a positive count with a null array
        assert hs.L.mcpt_scene_add_objects(hs.h, C.byref(a), None, None) == 1
        assert hs.L.mcpt_scene_add_objects(hs.h, None, None, None) == 1
        unchanged("null")
        hs.add_objects(objs, tris)  # and the handle still takes a good addition
        assert len(hs.visibility()[0]) == len(kept.objects) + 2
    chess = pkg.scenes.chess_scene(width=64, height=36, spp=2)
    inst = hip.HipScene(chess, builder="sah", instancing=True)
    assert inst.info()["n_instances"] > 0
    frame, _ = inst.render(spp=1, seed=2)
    tree = inst.dump_bvh()
    with pytest.raises(hip.McptError) as e:
        inst.add_objects(sphere_object(pkg, (0, 1, 0), 0.5, 0), None)
    assert e.value.code == 1 and "instancing" in str(e.value)
    assert len(inst.visibility()[0]) == len(chess.objects) and same_bits(frame, inst.render(spp=1, seed=2)[0]).all()
    again = inst.dump_bvh()
    assert again[1].tobytes() == tree[1].tobytes() and again[2].tobytes() == tree[2].tobytes() and again[0]["n_instances"] == tree[0]["n_instances"]


def test_group_add_objects(pkg, hip, cornell):
    """Two replicas on one device: mcpt_group_add_objects, then mcpt_group_render, equals a group of the fresh description."""
    kept, (objs, tris) = split(hip, cornell, [SHORT, PLASTIC_SPHERE])
    objs["material"][0] = len(kept.materials)
    mats = [green(pkg)]
    g = hip.HipGroup(kept, [0, 0])
    first, _ = g.add_objects(objs, tris, mats)
    assert first == len(kept.objects)
    want = extend_numpy(kept, objs, tris, mats)
    assert same_description(g.sd, want)
    fresh = hip.HipGroup(want, [0, 0])
    a, _ = g.render(spp=SPP, seed=6)
    b, _ = fresh.render(spp=SPP, seed=6)
    assert same_bits(a, b).all()
    assert not same_bits(a, hip.HipScene(kept).render(spp=SPP, seed=6)[0]).all()
    bad = objs.copy()
    bad["material"][1] = 99
    with pytest.raises(hip.McptError) as e:
        g.add_objects(bad, tris)
    assert e.value.code == 1 and "mcpt_group_add_objects" in str(e.value)
    assert same_bits(a, g.render(spp=SPP, seed=6)[0]).all()
    g.close()
    fresh.close()
