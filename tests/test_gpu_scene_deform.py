"""mcpt_scene_deform on the GPU: after a deformation a scene behaves exactly like a scene freshly created from desc'' (the creation
description with each deformed mesh's positions replaced by the latest ones given, then the current transforms applied) with the same
build options.

The rules are those of tests/test_gpu_scene_update.py: with the host builders (sah, reference) bit for bit, the tree dump included; with
the device builders (lbvh, ploc) hits equal ray for ray and a frame within 3 floats.  Every comparison is between the deformed handle and
a fresh scene (or a float64 restatement, for the motion pass); nothing is compared with a recorded number."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deform_cases import (DEVICE_BUILDERS, LIGHT, SHORT, STRIP_SIZES, TALL, GLASS_SPHERE, DeviceArray, assert_equals_fresh, assert_motion_close,  # noqa: E402
                          assert_same_frame, assert_same_hits, assert_same_info, camera_and_random_rays, cornell_rays, deformed_scene, motion_f64,
                          object_positions, positions_of, quad_scene, rotate_y, same_bits, scene_65, strips_scene, translate, wave)

pytestmark = pytest.mark.gpu

f32 = np.float32
W = H = 64


def prims_of(sd, objects):
    out = []
    for o in objects:
        out.extend(range(int(sd.objects["first_tri"][o]), int(sd.objects["first_tri"][o] + sd.objects["n_tri"][o])))
    return np.array(out, np.int64)


# ---------------------------------------------------------------- 1. equals a fresh scene
@pytest.mark.parametrize("builder,quant", [("sah", -1), ("sah", 0), ("reference", 0), ("reference", 1), ("lbvh", -1), ("lbvh", 0), ("ploc", -1), ("ploc", 0)])
def test_deform_equals_a_fresh_scene(pkg, hip, builder, quant):
    """The short box's vertices displaced by a smooth function of position (shared corners stay shared), by host pointer."""
    sd = pkg.scenes.cornell_demo(W, H, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder, quantise=quant)
    before, _ = hs.render(spp=4, seed=5)
    P = wave(object_positions(sd, SHORT))
    info = hs.deform([(SHORT, P)])
    assert info["path"] == (1 if dev else 0) and info["n_moved_tris"] == int(sd.objects["n_tri"][SHORT])
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, {SHORT: P}), builder=builder, quantise=quant)
    o, d = cornell_rays(hs, W, H, 4)
    prim = assert_equals_fresh(hs, fresh, o, d, dev, what=builder)
    assert (prim >= 0).mean() > 0.5 and np.isin(prim, prims_of(sd, [SHORT])).sum() > 500
    assert (~same_bits(hs.render(spp=4, seed=5)[0], before)).sum() > 100  # the box did change
    assert_same_frame(hs.render_aovs(aov_spp=2, seed=5, specular_depth=2), fresh.render_aovs(aov_spp=2, seed=5, specular_depth=2), dev, "aovs")
    assert hs.deform([])["n_moved_tris"] == 0  # n == 0: a valid no-op
    assert_same_hits(hs, fresh, o, d)


# ---------------------------------------------------------------- 2. segment and block edges
@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
def test_segment_and_block_edges(pkg, hip, builder):
    """Strips of 1, 63, 64, 65 and 257 triangles deformed in one call (segment borders inside a wave, on a wave's edge, beyond a 256-lane
    block), then only the 1-triangle and the 257-triangle strips.  Objects not listed keep their records: hits on them are bit-identical."""
    sd = strips_scene(pkg, W, H)
    assert [int(n) for n in sd.objects["n_tri"][:5]] == list(STRIP_SIZES)
    hs = hip.HipScene(sd, builder=builder)
    o, d = camera_and_random_rays(hs, W, H, 4, [-450, -55, -100], [450, 115, 300])
    t0, p0 = hs.intersect(o, d)
    assert np.isin(p0, prims_of(sd, range(5))).sum() > 300

    def untouched_hits_kept(t_before, p_before, objects):
        t1, p1 = hs.intersect(o, d)
        sel = (p1 >= 0) & (p1 == p_before) & np.isin(p1, prims_of(sd, objects))
        assert sel.sum() > 2000 and np.array_equal(t_before[sel].view(np.uint64), t1[sel].view(np.uint64))
        return t1, p1

    bases = {k: wave(object_positions(sd, k), amp=3.0, freq=0.11, phase=0.3 * k) for k in range(5)}
    info = hs.deform(list(bases.items()))
    assert info["path"] == 1 and info["n_moved_tris"] == sum(STRIP_SIZES)
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, bases), builder=builder)
    assert_equals_fresh(hs, fresh, o, d, True, what="five strips")
    t1, p1 = untouched_hits_kept(t0, p0, [5, 6])
    for k in (4, 0):  # the listed order is the caller's: the 257-lane segment first
        bases[k] = wave(object_positions(sd, k), amp=5.0, freq=0.07, phase=1.0 + k)
    info = hs.deform([(4, bases[4]), (0, bases[0])])
    assert info["path"] == 1 and info["n_moved_tris"] == 258
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, bases), builder=builder)
    assert_equals_fresh(hs, fresh, o, d, True, what="two strips")
    untouched_hits_kept(t1, p1, [1, 2, 3, 5, 6])


# ---------------------------------------------------------------- 3. device pointer equals host pointer
def test_device_pointer_equals_host_pointer():
    """The same deformation as a numpy array and as a torch tensor on the scene's device, PLOC and LBVH: the same t and primitive ids on all
    rays, frames within the device-builder rule.  It runs in a child process because torch must be imported before the library
    (tests/deform_torch_child.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "deform_torch_child.py")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [x["builder"] for x in rows] == ["ploc", "lbvh"]
    n = None
    for x in rows:
        assert x["path_host"] == 1 and x["path_device"] == 1 and x["n_moved_tris"][0] == x["n_moved_tris"][1] > 0
        assert x["prim_differ"] == 0 and x["t_differ"] == 0 and x["hit_fraction"] > 0.5
        assert x["frame_differ"] <= 3 and x["non_contiguous_refused"]
        n = x["n_moved_tris"][0]
    assert n is not None


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_device_buffer_equals_host_pointer_in_process(pkg, hip, builder):
    """The same as above with a buffer allocated through the library's own HIP runtime (__cuda_array_interface__), several objects in one
    call, host and device items mixed."""
    sd = strips_scene(pkg, W, H)
    a, b = hip.HipScene(sd, builder=builder), hip.HipScene(sd, builder=builder)
    bases = {k: wave(object_positions(sd, k), amp=4.0, freq=0.09, phase=k) for k in (3, 4, 1)}
    assert a.deform(list(bases.items()))["path"] == 1
    bufs = {k: DeviceArray(bases[k]) for k in (3, 4)}
    info = b.deform([(3, bufs[3]), (4, hip.DevicePositions(bufs[4].ptr, STRIP_SIZES[4])), (1, bases[1])])
    assert info["path"] == 1 and info["n_moved_tris"] == 65 + 257 + 63
    o, d = camera_and_random_rays(a, W, H, 4, [-450, -55, -100], [450, 115, 300])
    assert_equals_fresh(b, a, o, d, True, what=builder)


# ---------------------------------------------------------------- 4. composition with transforms
@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_composition_with_transforms(pkg, hip, builder):
    """deform, update (a rotation), deform again, update (another matrix): after each step the scene is the fresh scene of (current matrix o
    latest base).  The tall box is deformed and never transformed: it stores the given floats, -0.0 included, as a fresh scene does."""
    sd = pkg.scenes.cornell_demo(W, H, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder)
    o, d = cornell_rays(hs, W, H, 4)
    P1, P2 = wave(object_positions(sd, SHORT)), wave(object_positions(sd, SHORT), amp=20.0, phase=2.0)
    Q = wave(object_positions(sd, TALL), amp=6.0, phase=0.5)
    Q[object_positions(sd, TALL) == 0] = -0.0  # the vertices on the floor keep their zero, with the sign bit set
    assert np.signbit(Q[Q == 0]).any()
    R1, M2 = rotate_y(0.35, (185, 82, 169), shift=(25, 0, -30)), np.array([[0.8, 0, 0.1, 40], [0, 1.2, 0, 0], [-0.1, 0, 0.9, 10]], f32)
    steps = [("deform", [(SHORT, P1), (TALL, Q)], {SHORT: P1, TALL: Q}, {}),
             ("update", [(SHORT, R1)], {SHORT: P1, TALL: Q}, {SHORT: R1}),
             ("deform", [(SHORT, P2)], {SHORT: P2, TALL: Q}, {SHORT: R1}),
             ("update", [(SHORT, M2)], {SHORT: P2, TALL: Q}, {SHORT: M2})]
    for k, (call, items, bases, xf) in enumerate(steps):
        info = getattr(hs, call)(items)
        assert info["path"] == (1 if dev else 0)
        fresh = hip.HipScene(deformed_scene(pkg, hip, sd, bases, xf), builder=builder)
        assert_equals_fresh(hs, fresh, o, d, dev, what="%s step %d" % (builder, k))
        fresh.close()


# ---------------------------------------------------------------- 5. emitter
@pytest.mark.parametrize("builder", ["sah", "reference", "lbvh", "ploc"])
def test_deforming_the_light_takes_the_host_path(pkg, hip, builder):
    """The light tables are host-built: an emissive mesh deforms on path 0 under every builder, and the tables equal a fresh scene's.  With
    a device pointer the positions are downloaded first."""
    sd = pkg.scenes.cornell_demo(W, H, 4)
    dev = builder in DEVICE_BUILDERS
    P = wave(object_positions(sd, LIGHT), amp=25.0, freq=0.013)
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, {LIGHT: P}), builder=builder)
    u = np.random.default_rng(2).uniform(0, 1, (2000, 4)).astype(f32)
    want = fresh.sample_light(u)
    assert not same_bits(want, hip.HipScene(sd, builder=builder).sample_light(u)).all()
    o, d = cornell_rays(fresh, W, H, 1, n_random=3000)
    for how in ("host", "device"):
        hs = hip.HipScene(sd, builder=builder)
        buf = DeviceArray(P) if how == "device" else P
        info = hs.deform([(LIGHT, buf)])
        assert info["path"] == 0 and info["n_moved_tris"] == int(sd.objects["n_tri"][LIGHT])
        assert same_bits(hs.sample_light(u), want).all(), how
        assert_equals_fresh(hs, fresh, o, d, dev, seed=8, what="%s %s" % (builder, how))
        hs.close()


# ---------------------------------------------------------------- 6. the host copy is not stale
def test_host_copy_follows_a_device_pointer_deformation(pkg, hip):
    """PLOC: a box deformed by device pointer (path 1), then the light moved (path 0, which flattens the host copy of the base): the result
    is the fresh scene with both changes."""
    sd = pkg.scenes.cornell_demo(W, H, 4)
    hs = hip.HipScene(sd, builder="ploc")
    P = wave(object_positions(sd, SHORT))
    buf = DeviceArray(P)
    assert hs.deform([(SHORT, buf)])["path"] == 1
    buf.free()  # the scene keeps nothing of the caller's buffer
    T = translate(-40, -30, 20)
    assert hs.update([(LIGHT, T)])["path"] == 0
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, {SHORT: P}, {LIGHT: T}), builder="ploc")
    o, d = cornell_rays(hs, W, H, 4)
    prim = assert_equals_fresh(hs, fresh, o, d, True)
    assert np.isin(prim, prims_of(sd, [SHORT])).sum() > 500
    u = np.random.default_rng(2).uniform(0, 1, (500, 4)).astype(f32)
    assert same_bits(hs.sample_light(u), fresh.sample_light(u)).all()


# ---------------------------------------------------------------- 7. refused calls
def assert_refused(hip, hs, items, frame, spp, text=None):
    with pytest.raises(hip.McptError) as e:
        hs.deform(items)
    assert e.value.code == 1 and (text is None or text in str(e.value)), str(e.value)
    assert same_bits(frame, hs.render(spp=spp, seed=2)[0]).all(), items


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_refused_calls_leave_the_scene_as_it_was(pkg, hip, builder):
    sd = pkg.scenes.cornell_demo(W, H, 4)
    dev = builder in DEVICE_BUILDERS
    hs = hip.HipScene(sd, builder=builder)
    R = rotate_y(0.35, (185, 82, 169), shift=(25, 0, -30))
    hs.update([(SHORT, R)])
    frame, _ = hs.render(spp=4, seed=2)
    P, Q = wave(object_positions(sd, SHORT)), wave(object_positions(sd, TALL))
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = P.copy()
        bad[-1, 2, 1] = bad_value
        assert_refused(hip, hs, [(TALL, Q), (SHORT, bad)], frame, 4, "not finite")  # the valid item before it changes nothing either
        buf = DeviceArray(bad)
        assert_refused(hip, hs, [(TALL, Q), (SHORT, buf)], frame, 4, "not finite")
        buf.free()
    assert_refused(hip, hs, [(GLASS_SPHERE, np.zeros((1, 3, 3), f32))], frame, 4, "sphere")
    assert_refused(hip, hs, [(SHORT, P), (SHORT, P)], frame, 4, "listed twice")
    assert_refused(hip, hs, [(len(sd.objects), np.zeros((1, 3, 3), f32))], frame, 4, "out of range")
    assert_refused(hip, hs, [(-1, np.zeros((1, 3, 3), f32))], frame, 4, "out of range")
    # a following update still transforms the OLD base
    M = translate(40, 0, 60)
    hs.update([(SHORT, M), (TALL, M)])
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, {}, {SHORT: M, TALL: M}), builder=builder)
    o, d = cornell_rays(hs, W, H, 4)
    assert_equals_fresh(hs, fresh, o, d, dev, what=builder)


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
def test_non_finite_device_positions_at_the_segment_edges(pkg, hip, builder):
    """A non-finite value inside a device buffer, at lane 0 and at the last lane of the 65-triangle segment (the only live lane of its
    wave), alone and behind the 257-triangle segment: the kernel's flag word refuses the call and nothing is swapped."""
    sd = strips_scene(pkg, W, H)
    hs = hip.HipScene(sd, builder=builder)
    first = {k: wave(object_positions(sd, k), amp=3.0, freq=0.11) for k in (3, 4)}
    hs.deform(list(first.items()))
    frame, _ = hs.render(spp=4, seed=2)
    good4 = wave(object_positions(sd, 4), amp=6.0, freq=0.05)
    for flat_index, value in ((0, np.nan), (64 * 9 + 8, np.inf), (64 * 9, -np.inf)):
        bad = wave(object_positions(sd, 3), amp=6.0, freq=0.05).reshape(-1)
        bad[flat_index] = value
        buf = DeviceArray(bad)
        assert_refused(hip, hs, [(3, buf)], frame, 4, "not finite")
        assert_refused(hip, hs, [(4, good4), (3, buf)], frame, 4, "not finite")
        buf.free()
    # the base is still the first deformation: a transform applies to it, not to what the refused calls carried
    M = translate(5, 3, -2)
    hs.update([(3, M), (4, M)])
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, first, {3: M, 4: M}), builder=builder)
    o, d = camera_and_random_rays(hs, W, H, 4, [-450, -55, -100], [450, 115, 300])
    assert_equals_fresh(hs, fresh, o, d, True, what=builder)


def test_instanced_scene_is_refused(pkg, hip):
    chess = pkg.scenes.chess_scene(width=64, height=36, spp=1)
    inst = hip.HipScene(chess, builder="sah", instancing=True)
    assert inst.info()["n_instances"] == 14
    frame, _ = inst.render(spp=1, seed=2)
    assert_refused(hip, inst, [(16, object_positions(chess, 16))], frame, 1, "instancing")


# ---------------------------------------------------------------- 8. the LDS-resident flavour
@pytest.mark.parametrize("small", [True, False])
def test_lds_resident_flavour_survives_a_deformation(pkg, hip, monkeypatch, small):
    if small:
        monkeypatch.delenv("MCPT_SMALL_SCENE", raising=False)
    else:
        monkeypatch.setenv("MCPT_SMALL_SCENE", "0")
    sd = pkg.scenes.cornell_demo(W, H, 4)
    P = wave(object_positions(sd, SHORT))
    for builder in ("sah", "lbvh"):  # (the PLOC tree of this scene has more levels than the LDS-resident kernels' stack holds)
        hs = hip.HipScene(sd, builder=builder)
        assert hs.info()["lds_resident"] == (1 if small else 0)
        hs.deform([(SHORT, P)])
        if builder == "sah" or not small:  # (the height of a rebuilt LBVH is the builder's: the comparison with the fresh scene decides)
            assert hs.info()["lds_resident"] == (1 if small else 0)
        fresh = hip.HipScene(deformed_scene(pkg, hip, sd, {SHORT: P}), builder=builder)
        o, d = cornell_rays(hs, W, H, 1, n_random=4000)
        assert_equals_fresh(hs, fresh, o, d, builder in DEVICE_BUILDERS, seed=3, what=builder)


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_deforming_the_scene_one_triangle_beyond_the_lds_limit(pkg, hip, monkeypatch, builder):
    monkeypatch.delenv("MCPT_SMALL_SCENE", raising=False)
    sd = scene_65(pkg)
    P = wave(object_positions(sd, 0), amp=2.0, freq=0.2)
    hs = hip.HipScene(sd, builder=builder)
    assert hs.info()["lds_resident"] == 0
    assert hs.deform([(0, P)])["path"] == (1 if builder == "lbvh" else 0)
    assert hs.info()["lds_resident"] == 0
    fresh = hip.HipScene(deformed_scene(pkg, hip, sd, {0: P}), builder=builder)
    rng = np.random.default_rng(4)
    o = rng.uniform(-60, 60, (6000, 3)).astype(f32)
    d = (rng.uniform(-20, 20, (6000, 3)) - o).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    prim = assert_equals_fresh(hs, fresh, o, d, builder == "lbvh", spp=2, seed=1)
    assert (prim >= 0).sum() > 200


# ---------------------------------------------------------------- 9. motion and sequence
@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_motion_of_a_deformed_quad(pkg, hip, builder):
    """Every vertex of the grid moves on its own: the motion pass evaluates a hit's barycentrics on the live triangle and on the snapshot's,
    which the float64 restatement does from the library's own rays and hits and the old and new vertices."""
    sd = quad_scene(pkg, W, H)
    hs = hip.HipScene(sd, builder=builder)
    hs.snapshot()
    old = object_positions(sd, 0)
    new = wave(old, amp=9.0, freq=0.03)
    assert hs.deform([(0, new)])["path"] == (1 if builder == "ploc" else 0)
    got = hs.render_motion(seed=1, aov_spp=4)
    V_prev = positions_of(sd.triangles)
    V_cur = positions_of(deformed_scene(pkg, hip, sd, {0: new}).triangles)
    want, prim = motion_f64(hs, sd, V_cur, V_prev)
    assert_motion_close(got, want, builder)
    on_quad = np.isin(prim, prims_of(sd, [0]))
    touched = on_quad.any(-1)
    assert touched.sum() > 300 and (np.abs(got[..., 0:2][on_quad.all(-1)]).max(-1) > 0.05).mean() > 0.9
    static = ~touched & (got[..., 3] > 0)
    assert static.sum() > 300 and (got[..., 0:2][~touched] == 0).all()  # the floor, the light, the sphere: exactly zero


def test_sequence_with_deformations_is_the_composition_of_the_calls(pkg, hip):
    """Three frames of a sequence, the grid deformed before each, on the host builder: every output equals the separate calls on a second
    handle bit for bit (the loop of tests/test_gpu_sequence.py with deform in the place of update)."""
    sd = quad_scene(pkg, W, H)
    a, b = hip.HipScene(sd, builder="sah"), hip.HipScene(sd, builder="sah")
    seq = a.sequence(filter=True, aov_spp=4)
    hist, length = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    hist_var, prev_depth = np.zeros((H, W), f32), np.zeros((H, W), f32)
    want = ("fb", "accumulated", "denoised", "variance", "len", "aov", "motion")
    for k in range(3):
        P = wave(object_positions(sd, 0), amp=4.0 * (k + 1), freq=0.03, phase=0.4 * k)
        b.snapshot()
        assert b.deform([(0, P)])["path"] == 0
        a.deform([(0, P)])
        rd = b.render_denoised(spp=4, seed=k + 1, aov_spp=4)
        c, _ = b.render(spp=4, seed=k + 1)
        aov = b.render_aovs(aov_spp=4, seed=k + 1)
        motion = b.render_motion(seed=k + 1, aov_spp=4)
        acc, acc_var, acc_len = b.temporal_accumulate(c, rd["variance"], motion, hist, hist_var, prev_depth, length)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=want, spp=4, seed=k + 1)
        assert r["info"]["frame_index"] == k
        for name, ref in (("fb", c), ("aov", aov), ("motion", motion), ("accumulated", acc), ("len", acc_len), ("variance", acc_var), ("denoised", den)):
            assert same_bits(r[name], ref).all(), (k, name)
        if k > 0:
            assert (motion[..., 0:2] != 0).any() and (acc_len > 1).any(), k
        hist, length, hist_var, prev_depth = acc, acc_len, acc_var, aov[..., 6].copy()
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 10. group
def test_group_deform(pkg, hip):
    """Two replicas on one device: mcpt_group_deform, then mcpt_group_render, equals a fresh group's frame and the deformed single scene's."""
    sd = pkg.scenes.cornell_demo(64, 48, 4)
    bases = {SHORT: wave(object_positions(sd, SHORT)), LIGHT: wave(object_positions(sd, LIGHT), amp=25.0, freq=0.013)}
    g = hip.HipGroup(sd, [0, 0])
    g.deform(list(bases.items()))
    a, _ = g.render(spp=4, seed=6)
    fresh = hip.HipGroup(deformed_scene(pkg, hip, sd, bases), [0, 0])
    assert same_bits(a, fresh.render(spp=4, seed=6)[0]).all()
    fresh.close()
    hs = hip.HipScene(sd)
    hs.deform(list(bases.items()))
    assert same_bits(a, hs.render(spp=4, seed=6)[0]).all()
    buf = DeviceArray(bases[SHORT])
    for bad in ([(SHORT, buf)], [(TALL, wave(object_positions(sd, TALL))), (SHORT, hip.DevicePositions(buf.ptr, len(bases[SHORT])))], [(99, np.zeros((1, 3, 3), f32))]):
        with pytest.raises(hip.McptError) as e:
            g.deform(bad)
        assert e.value.code == 1
        assert same_bits(a, g.render(spp=4, seed=6)[0]).all()
    g.close()
