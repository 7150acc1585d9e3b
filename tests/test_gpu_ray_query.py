"""mcpt_query_closest / mcpt_query_occluded on the GPU: rays and results in device memory, on a stream.

The reference for closest hits is mcpt_intersect on the same scene (t bit for bit, prim equal); the reference for occlusion is the rule
of include/mcpt.h evaluated in float64 from those distances, without a tolerance; the reference for a live scene is a freshly created
scene of the edited description.  Device buffers are made without torch (tests/ray_query_cases.py); every output buffer is followed by 64
guard elements that must survive.  torch and a non-default stream: tests/ray_query_torch_child.py, a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from add_cases import addition_of, extend_numpy  # noqa: E402
from chain_scene import chain_scene  # noqa: E402
from deform_cases import SHORT, TALL, PLASTIC_SPHERE, DeviceArray, cornell_rays, deformed_scene, object_positions, translate, wave  # noqa: E402
from ray_query_cases import (ALL, DBL_MAX, DevBuf, Rays, check_attributes, closest, expected_occluded, object_of, occluded, out_buffer,  # noqa: E402
                             tmax_cycle)
from visibility_cases import live_ids, mask_hiding, translate_ids  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
W = H = 64
SPP = 4
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_answer(a, b, names, what=""):
    for k in names:
        differ = int((bits(a[k]) != bits(b[k])).sum())
        assert differ == 0, "%s: %s differs on %d values" % (what, k, differ)


def scene_rays(hs, sd, n, seed):
    """The _scene_rays recipe of tests/test_gpu_parity.py: camera rays plus rays started at their hit points."""
    rng = np.random.default_rng(seed)
    Wd, Hd = int(sd.camera["width"]), int(sd.camera["height"])
    pix = rng.integers(0, Wd * Hd, size=n).astype(np.uint32)
    smp = rng.integers(0, 64, size=n).astype(np.uint32)
    o, d = hs.camera_rays(pix, smp, seed=7)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    p = (o + d * np.where(hit, t, 0.0)[:, None].astype(f32)).astype(f32)
    d2 = rng.normal(size=(n, 3)).astype(f32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    o2 = np.where(hit[:, None], p, o).astype(f32)
    return np.concatenate([o, o2]), np.concatenate([d, d2.astype(f32)])


class Case:
    """A scene, rays on the device, and mcpt_intersect's answer for them: computed once, shared, never changed."""

    def __init__(self, hs, sd, o, d):
        self.hs, self.sd = hs, sd
        self.o, self.d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
        self.rays = Rays(self.o, self.d)
        self.t, self.prim = hs.intersect(self.o, self.d)
        self.tmax = tmax_cycle(self.t, self.prim)
        self.rays_tmax = Rays(self.o, self.d, self.tmax)


@pytest.fixture(scope="module")
def cornell(pkg):
    return pkg.scenes.cornell_demo(W, H, SPP)


@pytest.fixture(scope="module")
def cases(pkg, hip, cornell):
    made = {}

    def get(name):
        if name not in made:
            if name == "chess":  # 160 x 90, sah, quantised: the refill kernel
                sd = pkg.scenes.chess_scene(width=160, height=90, spp=4)
                hs = hip.HipScene(sd, builder="sah", quantise=1)
                assert hs.info()["quantised"] == 1
                made[name] = Case(hs, sd, *scene_rays(hs, sd, 20000, 11))
            else:
                hs = hip.HipScene(cornell, builder=name)
                made[name] = Case(hs, cornell, *cornell_rays(hs, W, H, SPP))
        return made[name]

    yield get
    for c in made.values():
        c.hs.close()


CASES = ["sah", "reference", "lbvh", "ploc", "chess"]


# ---------------------------------------------------------------- 1. parity with mcpt_intersect
@pytest.mark.parametrize("name", CASES)
def test_closest_equals_intersect(cases, name):
    c = cases(name)
    assert (c.prim >= 0).mean() > 0.3
    res, info = closest(c.hs, c.rays)
    assert np.array_equal(res["prim"], c.prim), "primitive ids differ on %d rays" % int((res["prim"] != c.prim).sum())
    assert np.array_equal(bits(res["t"]), bits(c.t))
    assert info["launches"] == 1 and info["staged_bytes"] >= 48 * c.rays.n


@pytest.mark.parametrize("builder", ["sah", "reference"])
def test_degenerate_directions(hip, cornell, builder):
    """The directions of tests/test_gpu_parity.py::test_intersect_degenerate_directions: zero components and an all-zero direction."""
    hs = hip.HipScene(cornell, builder=builder)
    rng = np.random.default_rng(5)
    n = 6000
    o = rng.uniform(-50, 600, size=(n, 3)).astype(f32)
    o[::7, 0] = 0.0
    o[1::7, 1] = 548.8
    o[2::7, 2] = 559.2
    d = rng.normal(size=(n, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.eye(3, dtype=f32)
    d[0::5] = axes[rng.integers(0, 3, size=len(d[0::5]))] * rng.choice([-1, 1], size=(len(d[0::5]), 1)).astype(f32)
    d[1::5, 0] = 0.0
    d[2::25] = 0.0
    d[3::25, 1] = -0.0
    t, prim = hs.intersect(o, d)
    assert (prim >= 0).mean() > 0.2
    res, _ = closest(hs, Rays(o, d))
    assert np.array_equal(res["prim"], prim) and np.array_equal(bits(res["t"]), bits(t))
    tm = tmax_cycle(t, prim)
    occ, _ = occluded(hs, Rays(o, d, tm))
    assert np.array_equal(occ, expected_occluded(t, prim, tm))
    hs.close()


# ---------------------------------------------------------------- 2. edges of the launch shape
def test_launch_edges(hip, cornell, cases, monkeypatch):
    """MCPT_QUERY_CHUNK = 256: n on both sides of a wave, of a workgroup (= the chunk) and of two chunks.  Every n gives the first n rays of
    the full answer, the guard elements behind every output survive (checked by DevBuf.get), and the call runs ceil(n / 256) chunks."""
    full = cases("sah")
    want_all, _ = closest(full.hs, full.rays, ALL)
    want_occ = expected_occluded(full.t, full.prim, full.tmax)
    monkeypatch.setenv("MCPT_QUERY_CHUNK", "256")
    hs = hip.HipScene(cornell, builder="sah")
    monkeypatch.delenv("MCPT_QUERY_CHUNK")
    assert np.array_equal(want_all["prim"], full.prim)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        r = Rays(full.o[:n], full.d[:n], full.tmax[:n])
        res, info = closest(hs, Rays(full.o[:n], full.d[:n]), ALL)
        assert info["launches"] == -(-n // 256), (n, info)
        assert_same_answer(res, {k: v[:n] for k, v in want_all.items()}, ALL, "n = %d" % n)
        occ, info = occluded(hs, r)
        assert info["launches"] == -(-n // 256), (n, info)
        assert np.array_equal(occ, want_occ[:n]), n
    res, info = closest(hs, full.rays)  # many chunks, the last one partial
    assert info["launches"] == -(-full.rays.n // 256) and np.array_equal(res["prim"], full.prim) and np.array_equal(bits(res["t"]), bits(full.t))
    hs.close()


# ---------------------------------------------------------------- 3. deep trees
def test_deep_tree(pkg, hip):
    """chain_scene(30) with the linear builder: a tree deeper than the plain LDS stacks, so the retry flavour and both retrace kernels run."""
    sd = chain_scene(pkg, 30)
    hs = hip.HipScene(sd, builder="lbvh")
    assert hs.info()["bvh_height"] > 24
    rng = np.random.default_rng(9)
    n = 3000
    o1 = np.concatenate([rng.uniform(-1, 0, (n, 2)), np.full((n, 1), -5.0)], axis=1).astype(f32)
    d1 = np.tile(np.array([0, 0, 1], f32), (n, 1))
    o2 = rng.uniform([-2, -2, -6], [8, 8, 40], (n, 3)).astype(f32)
    d2 = rng.normal(size=(n, 3)).astype(f32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2.astype(f32)])
    t, prim = hs.intersect(o, d)
    assert (prim[:n] >= 0).all() and (prim >= 0).mean() > 0.5
    res, _ = closest(hs, Rays(o, d), ALL)
    assert np.array_equal(res["prim"], prim) and np.array_equal(bits(res["t"]), bits(t))
    assert np.array_equal(res["object"], np.where(prim >= 0, 0, -1))
    tm = tmax_cycle(t, prim)
    want = expected_occluded(t, prim, tm)
    assert 0.1 < want.mean() < 0.9
    occ, _ = occluded(hs, Rays(o, d, tm))
    assert np.array_equal(occ, want), "occlusion differs on %d rays" % int((occ != want).sum())
    occ, _ = occluded(hs, Rays(o, d, np.full(len(o), np.inf, f32)))
    assert np.array_equal(occ, (prim >= 0).astype(np.uint8))
    hs.close()


# ---------------------------------------------------------------- 4. the occlusion rule, exact
@pytest.mark.parametrize("name", CASES)
def test_occlusion_rule_exact(cases, name):
    """The cycle of tmax values (tests/ray_query_cases.py: tmax_cycle) around every known hit distance, the expected value from the rule in
    float64, no tolerance.  Both answers must be well represented: of the rays that hit, at least a quarter are expected occluded (three
    of the cycle's twelve entries, float32(t + 3e-4), 2 t and inf, always are) and at least a quarter not; that holds by construction.
    Counted over ALL rays, misses included, the occluded share is the hit fraction times that: 0.267 on the Cornell rays (78 % hit), which
    is asserted too, but 0.085 on the chess rays (31 % hit), where no answer of the code under test could raise it to a quarter."""
    c = cases(name)
    want = expected_occluded(c.t, c.prim, c.tmax)
    hit = c.prim >= 0
    print("%s: %d rays, %.3f hit; expected occluded: %.3f of the hits, %.3f of all rays" % (name, c.rays.n, hit.mean(), want[hit].mean(), want.mean()))
    assert hit.mean() > 0.3 and want[hit].mean() >= 0.25 and (1 - want[hit]).mean() >= 0.25
    assert (1 - want).mean() >= 0.25 and (name == "chess" or want.mean() >= 0.25)
    occ, _ = occluded(c.hs, c.rays_tmax)
    assert set(np.unique(occ)) <= {0, 1}
    assert np.array_equal(occ, want), "occlusion differs on %d rays" % int((occ != want).sum())
    res, _ = closest(c.hs, c.rays_tmax, ("t", "prim", "object"))
    assert np.array_equal(res["prim"] >= 0, want == 1)
    keep = want == 1
    assert np.array_equal(res["prim"][keep], c.prim[keep]) and np.array_equal(bits(res["t"][keep]), bits(c.t[keep]))
    assert (res["prim"][~keep] == -1).all() and (res["t"][~keep] == DBL_MAX).all() and (res["object"][~keep] == -1).all()
    occ, _ = occluded(c.hs, Rays(c.o, c.d, np.full(c.rays.n, np.inf, f32)))  # "is anything hit"
    assert np.array_equal(occ, (c.prim >= 0).astype(np.uint8))


# ---------------------------------------------------------------- 5. attributes
def test_attributes_cornell(cases):
    c = cases("sah")
    res, _ = closest(c.hs, c.rays, ALL)
    assert np.array_equal(res["prim"], c.prim) and np.array_equal(bits(res["t"]), bits(c.t))
    n_tri, n_sph = check_attributes(c.sd, c.o, c.d, res, "cornell_demo")
    assert n_tri > 5000 and n_sph > 500
    for w in ALL:  # one output at a time: the same values
        one, _ = closest(c.hs, c.rays, (w,))
        assert_same_answer(one, res, (w,), "alone")


def test_attributes_chess_with_a_sphere(pkg, hip, cases):
    """The chess scene has no sphere: one is appended with extend_scene, above the middle of the board, and rays are aimed at it."""
    base = cases("chess")
    sd = base.sd
    v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]])
    lo, hi = v.min(0), v.max(0)
    centre = ((lo + hi) / 2).astype(f32)
    centre[1] = hi[1] + f32(0.2) * (hi - lo).max()
    radius = f32(0.05) * (hi - lo).max()
    ball = np.zeros(1, sd.objects.dtype)
    ball["kind"], ball["material"], ball["center"], ball["radius"] = 1, 0, centre, radius
    ext = hip.extend_scene(sd, ball, None)
    hs = hip.HipScene(ext, builder="sah", quantise=1)
    rng = np.random.default_rng(4)
    eye = np.asarray(sd.camera["position"], f32).reshape(3)
    aim = centre + rng.normal(0, 0.5 * radius, (2000, 3)).astype(f32) - eye
    aim = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(f32)
    o, d = np.concatenate([base.o, np.tile(eye, (2000, 1))]), np.concatenate([base.d, aim])
    t, prim = hs.intersect(o, d)
    res, _ = closest(hs, Rays(o, d), ALL)
    assert np.array_equal(res["prim"], prim) and np.array_equal(bits(res["t"]), bits(t))
    n_tri, n_sph = check_attributes(ext, o, d, res, "chess + sphere")
    assert n_tri > 10000 and n_sph > 500
    assert (res["object"][prim >= len(ext.triangles)] == len(ext.objects) - 1).all()
    hs.close()


# ---------------------------------------------------------------- 6. live scene
def answers(hs, rays, rays_tmax, names):
    res, _ = closest(hs, rays, names)
    res["occluded"], _ = occluded(hs, rays_tmax)
    return res


@pytest.mark.parametrize("builder", ["ploc", "sah"])
def test_live_scene(pkg, hip, cornell, builder):
    """After every edit a query on the edited scene equals a query on a freshly created scene of the edited description: with sah every
    output bit for bit, with ploc prim ids and t bits (the rule of assert_same_hits).  Before every edit a query is enqueued and NOT
    synchronised; the edit follows at once, and the query's results must be those of the scene before the edit (the event rule)."""
    sd = cornell
    names = ALL if builder == "sah" else ("t", "prim", "object")
    hs = hip.HipScene(sd, builder=builder)
    o, d = cornell_rays(hs, W, H, SPP)
    # what will be added in the last step, and rays aimed at it
    objs, tris = addition_of(sd, [SHORT, PLASTIC_SPHERE])
    for k in ("v0", "v1", "v2"):
        tris[k] = tris[k] + np.array([0, 250, -60], f32)
    objs["center"][1], objs["radius"][1] = (150, 120, 60), 40
    eye = np.asarray(sd.camera["position"], f32).reshape(3)
    rng = np.random.default_rng(8)
    targets = np.concatenate([(tris["v0"] + tris["v1"] + tris["v2"]) / f32(3), np.tile(objs["center"][1], (200, 1)) + rng.normal(0, 15, (200, 3)).astype(f32)])
    aim = (targets - eye).astype(np.float64)
    aim = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(f32)
    o, d = np.concatenate([o, np.tile(eye, (len(aim), 1))]), np.concatenate([d, aim])
    rays = Rays(o, d)
    tm, rays_tm = None, None

    def set_tmax():
        """tmax just behind the current first hit: occluded now, and no longer once the blocker is gone and nothing else lies within one unit."""
        nonlocal tm, rays_tm
        t0, p0 = hs.intersect(o, d)
        tm = np.where(p0 >= 0, t0 + 1.0, np.inf).astype(f32)
        rays_tm = Rays(o, d, tm)

    set_tmax()

    def check(fresh_sd, what, prim_map=None, obj_map=None):
        fresh = hip.HipScene(fresh_sd, builder=builder)
        a, b = answers(hs, rays, rays_tm, names), answers(fresh, rays, rays_tm, names)
        tb, pb = fresh.intersect(o, d)
        assert np.array_equal(b["prim"], pb) and np.array_equal(bits(b["t"]), bits(tb))
        assert np.array_equal(b["occluded"], expected_occluded(tb, pb, tm))
        if prim_map is not None:  # ids of the live scene -> ids of the compacted description
            a = dict(a)
            a["prim"] = translate_ids(a["prim"], prim_map)
            assert (a["prim"] != -2).all(), "%d rays report a hidden primitive" % int((a["prim"] == -2).sum())
            a["object"] = np.where(a["object"] >= 0, obj_map[np.maximum(a["object"], 0)], -1).astype(np.int32)
        assert_same_answer(a, b, names + ("occluded",), "%s, %s" % (builder, what))
        fresh.close()
        return a

    def edit_behind_a_query(edit):
        """Enqueue both queries, edit at once, then read: the answers are those of the scene before the edit."""
        before = answers(hs, rays, rays_tm, names)
        out, _ = closest(hs, rays, names, enqueue_only=True)
        occ, _ = occluded(hs, rays_tm, enqueue_only=True)
        edit()
        got = {k: out[k].get() for k in names}
        got["occluded"] = occ.get()
        assert_same_answer(got, before, names + ("occluded",), "%s: a query enqueued before the edit" % builder)
        return before

    m = translate(40, 0, -30)
    edit_behind_a_query(lambda: hs.update([(SHORT, m)]))
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    check(now, "update")

    P = wave(object_positions(sd, TALL))
    dev_P = DeviceArray(P)
    edit_behind_a_query(lambda: hs.deform([(TALL, dev_P)]))
    now = deformed_scene(pkg, hip, sd, {TALL: P}, {SHORT: m})
    check(now, "deform")

    set_tmax()
    before = edit_behind_a_query(lambda: hs.set_visibility([(SHORT, False)]))
    mask = mask_hiding(now, [SHORT])
    csd, prim_map = hip.compact_scene(now, mask)
    obj_map = (np.cumsum(mask) - 1).astype(np.int32)
    after = check(csd, "set_visibility", prim_map, obj_map)
    live = answers(hs, rays, rays_tm, names)
    assert not np.isin(live["prim"], live_ids(now, SHORT)).any()
    blocked = np.isin(before["prim"], live_ids(now, SHORT))
    assert blocked.sum() > 200 and (before["occluded"][blocked] == 1).all()
    flipped = blocked & (live["occluded"] == 0)
    assert flipped.sum() > 100, flipped.sum()  # what only the short box blocked within tmax is visible now
    assert after is not None

    edit_behind_a_query(lambda: hs.set_visibility([(SHORT, True)]))
    check(now, "shown again")

    first = []
    edit_behind_a_query(lambda: first.append(hs.add_objects(objs, tris)[0]))
    want = extend_numpy(now, objs, tris)
    assert first[0] == len(now.objects)
    got = check(want, "add_objects")
    assert np.array_equal(got["object"], object_of(want, got["prim"]))
    assert (got["object"] == first[0]).sum() > 10 and (got["object"] == first[0] + 1).sum() > 50
    old_sphere = got["object"] == PLASTIC_SPHERE  # sphere ids moved up by the number of added triangles
    assert old_sphere.sum() > 50 and (got["prim"][old_sphere] == len(want.triangles) + PLASTIC_SPHERE).all()
    assert len(want.triangles) == len(now.triangles) + len(tris)
    hs.close()


# ---------------------------------------------------------------- 7. no allocation in the steady state
def test_no_allocation_in_the_steady_state(hip, cornell, cases):
    c = cases("sah")
    hs = hip.HipScene(cornell, builder="sah")
    small, large = Rays(c.o[:5000], c.d[:5000], c.tmax[:5000]), c.rays_tmax
    grew = [closest(hs, small)[1]["grew"], closest(hs, small)[1]["grew"], occluded(hs, small)[1]["grew"], closest(hs, large)[1]["grew"],
            closest(hs, large)[1]["grew"], occluded(hs, large)[1]["grew"], closest(hs, small, ALL)[1]["grew"]]
    assert grew == [1, 0, 0, 1, 0, 0, 0], grew
    hs.close()


# ---------------------------------------------------------------- 8. errors
def test_errors_leave_the_scene_usable(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    n = 256
    r = Rays(c.o[:n], c.d[:n], c.tmax[:n])
    t_out, occ_out = out_buffer("t", n), out_buffer("occluded", n)
    host = np.zeros((n, 3), f32)
    info = hip.QueryInfo()

    def rays(origins=r.o.ptr, dirs=r.d.ptr, tmax=r.tmax.ptr):
        return hip.RayBuffers(origins, dirs, tmax)

    def refused(rc, word):
        assert rc == 1 and word in L.mcpt_last_error(), (rc, L.mcpt_last_error())

    hits = hip.HitBuffers(t=t_out.ptr)
    refused(L.mcpt_query_closest(hs.h, n, C.byref(rays(origins=host.ctypes.data)), C.byref(hits), None, C.byref(info)), b"device")
    refused(L.mcpt_query_occluded(hs.h, n, C.byref(rays(dirs=host.ctypes.data)), occ_out.ptr, None, None), b"device")
    refused(L.mcpt_query_closest(hs.h, n, C.byref(rays()), C.byref(hip.HitBuffers()), None, None), b"every hit pointer is null")
    refused(L.mcpt_query_occluded(hs.h, n, C.byref(rays(tmax=None)), occ_out.ptr, None, None), b"tmax")
    refused(L.mcpt_query_occluded(hs.h, n, C.byref(rays()), None, None, None), b"occluded")
    refused(L.mcpt_query_closest(hs.h, -1, C.byref(rays()), C.byref(hits), None, None), b"n must be")
    refused(L.mcpt_query_closest(hs.h, 2 ** 31, C.byref(rays()), C.byref(hits), None, None), b"n must be")
    refused(L.mcpt_query_closest(hs.h, n, None, C.byref(hits), None, None), b"null rays")
    refused(L.mcpt_query_closest(hs.h, n, C.byref(rays(origins=None)), C.byref(hits), None, None), b"null rays")
    refused(L.mcpt_query_closest(hs.h, n, C.byref(rays()), C.byref(hip.HitBuffers(t=host.ctypes.data)), None, None), b"device")
    assert L.mcpt_query_closest(hs.h, 0, None, None, None, C.byref(info)) == 0 and info.launches == 0  # a valid no-op
    assert L.mcpt_query_occluded(hs.h, 0, None, None, None, None) == 0
    assert (t_out.get() == -7.25).all() and (occ_out.get() == 0xAB).all()  # nothing was written
    res, _ = closest(hs, c.rays)  # and the scene still answers
    assert np.array_equal(res["prim"], c.prim) and np.array_equal(bits(res["t"]), bits(c.t))


# ---------------------------------------------------------------- 9. torch and streams
def test_torch_tensors_on_a_side_stream():
    """tests/ray_query_torch_child.py (torch imported first): rays produced by a torch kernel on a non-default stream, both queries enqueued
    on that stream without a host synchronisation in between, outputs allocated by the call."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "ray_query_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in rec, rec
    assert rec["n"] > 20000 and rec["hit_fraction"] > 0.3
    assert rec["prim_differ"] == 0 and rec["t_differ"] == 0 and rec["occluded_differ"] == 0 and rec["filtered_differ"] == 0
    assert rec["outputs_are_torch"] and rec["on_side_stream"] and rec["non_contiguous_refused"]
    assert rec["grew"] == [1, 0]
