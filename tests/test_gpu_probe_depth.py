"""mcpt_query_probe_depth / mcpt_probe_shade_visible / mcpt_bake_probe_volume on the GPU.

Expected values are compositions of calls that exist without the feature: the directions come from hs.probe_rays, the distances from
hs.intersect, the normals from hs.query_closest (tests/probe_depth_cases.py: samples), folded by mcpt_probe_depth_fold_host; device bits
are compared with them.  Device buffers are made without torch, every output sits between two runs of 64 guard elements that must
survive.  torch and a non-default stream: tests/probe_depth_torch_child.py, a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_cases as pc  # noqa: E402
import probe_depth_cases as pdc  # noqa: E402
from add_cases import extend_numpy, split  # noqa: E402
from chain_scene import chain_scene  # noqa: E402
from deform_cases import PLASTIC_SPHERE, SHORT, deformed_scene, object_positions, translate, wave  # noqa: E402
from ray_query_cases import DevBuf, scene_extent  # noqa: E402
from sensor_query_cases import SENTINEL, same_bits  # noqa: E402
from test_probes_cpu import GRIDS, lookup_points, unit  # noqa: E402
from test_probe_depth_cpu import volume  # noqa: E402
from visibility_cases import mask_hiding  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
N_MAX, SPP_MAX = 65, 130
SHAPES = [(n, spp) for n in (1, 3, 65) for spp in (5, 64, 70, 130)]
SEED = 21


def assert_equal(got, want, what=""):
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


def make_scene(pkg, hip, name):
    """(description, creation keywords, probe points, max_distance) of a named case."""
    if name == "chess":
        sd = pkg.scenes.chess_scene(width=160, height=90, spp=4)
        kw = dict(builder="sah", quantise=1)
    elif name == "chain":
        sd = chain_scene(pkg, 40)
        kw = dict(builder="lbvh")
    else:
        sd = pkg.scenes.cornell_demo(64, 64, 4)
        kw = dict(builder=name)
    if name == "chain":
        p, md = np.random.default_rng(6).uniform(-2, 2, (N_MAX, 3)).astype(f32), 3.0
    else:
        p, md = pc.probe_points(sd, N_MAX), 0.3 * scene_extent(sd)
    return sd, kw, p, float(f32(md))


class Case:
    def __init__(self, pkg, hip, name):
        self.sd, self.kw, self.p, self.md = make_scene(pkg, hip, name)
        self.hs = hip.HipScene(self.sd, **self.kw)
        self._s = None

    def samples(self):
        """(d, r, backfacing) of the N_MAX x SPP_MAX samples, made once: d(i, k) depends on (seed, i, k) alone, so the samples of a
        smaller call are the leading block."""
        if self._s is None:
            self._s = pdc.samples(self.hs, self.p, SPP_MAX, SEED, self.md)
        return self._s

    def want(self, hip, n, spp):
        d, r, bf = self.samples()
        return hip.probe_depth_fold(d[:n, :spp], r[:n, :spp], bf[:n, :spp])


@pytest.fixture(scope="module")
def cases(pkg, hip):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(pkg, hip, name)
        return made[name]

    yield get
    for c in made.values():
        c.hs.close()


# ---------------------------------------------------------------- 1. parity of the fold
@pytest.mark.parametrize("name", ["sah", "lbvh", "ploc", "chess", "chain"])
def test_device_fold_equals_host_fold(pkg, hip, cases, monkeypatch, name):
    c = cases(name)
    if name in ("sah", "lbvh", "ploc"):
        assert c.hs.info()["lds_resident"] == 1
    if name == "chain":
        assert c.hs.info()["bvh_height"] > 24  # deeper than every LDS stack: the retry flavour and its retrace list
    monkeypatch.setenv("MCPT_QUERY_CHUNK", "64")
    small = hip.HipScene(c.sd, **c.kw)
    monkeypatch.delenv("MCPT_QUERY_CHUNK")
    d, r, bf = c.samples()
    hit_share, back_share, clamp_share = float((r < f32(c.md)).mean()), float(bf.mean()), float((r == f32(c.md)).mean())
    print("\n[probe depth] %s: %.0f %% of the samples are closer than max_distance %.3g, %.0f %% at it, %.0f %% back-facing"
          % (name, 100 * hit_share, c.md, 100 * clamp_share, 100 * back_share))
    if name != "chain":  # both branches of r occur in numbers: hits closer than max_distance, and misses or farther hits clamped to it
        assert hit_share > 0.1 and clamp_share > 0.1
    launches = {}
    for n, spp in SHAPES:
        wm, wc = c.want(hip, n, spp)
        for tag, hs in (("default chunk", c.hs), ("chunk 64", small)):
            m, cn, info = pdc.depth(hs, c.p[:n], spp, c.md, seed=SEED)  # (get() insists on the guard elements)
            what = "%s, n %d, spp %d, %s" % (name, n, spp, tag)
            assert_equal(m, wm, what + ", moments")
            assert np.array_equal(cn, wc), what + ", counts"
            launches[(n, spp, tag)] = info["launches"]
    # the chunking took place: whole probes per launch below 64 samples, 64-sample blocks of one probe above
    assert launches[(65, 5, "default chunk")] == 1 and launches[(65, 130, "default chunk")] == 1
    assert launches[(65, 5, "chunk 64")] == 6 and launches[(65, 64, "chunk 64")] == 65 and launches[(65, 70, "chunk 64")] == 130
    assert launches[(3, 130, "chunk 64")] == 9
    small.close()


def test_back_faces_are_counted(hip, cases):
    """The Cornell boxes and walls face the room, the spheres outward: probes in free space see few back faces, but not none (probe
    points inside a box or a sphere see only back faces)."""
    c = cases("sah")
    _, cn = c.want(hip, N_MAX, SPP_MAX)
    assert (cn[:, 0] == SPP_MAX).all() and (cn[:, 1] >= 0).all() and (cn[:, 1] <= SPP_MAX).all()
    assert cn[:, 1].sum() > 0 and (cn[:, 1] == 0).any()


# ---------------------------------------------------------------- 2. progressive calls, steady state
def test_progressive_calls(hip, cases):
    c = cases("chess")
    for total, first in ((130, 70), (130, 64), (5, 3)):
        one_m, one_c, _ = pdc.depth(c.hs, c.p, total, c.md, seed=SEED)
        out = pdc.depth_outputs(N_MAX)
        pdc.depth(c.hs, c.p, first, c.md, out=out, seed=SEED)
        two_m, two_c, _ = pdc.depth(c.hs, c.p, total - first, c.md, out=out, seed=SEED, sample_offset=first, accumulate=1)
        assert_equal(two_m, one_m, "%d + %d samples, moments" % (first, total - first))
        assert np.array_equal(two_c, one_c)
        wm, wc = c.want(hip, N_MAX, total)
        assert_equal(one_m, wm, "spp %d" % total)
        assert np.array_equal(one_c, wc)


def test_steady_state(hip, cases):
    c = cases("sah")
    hs = hip.HipScene(c.sd, **c.kw)
    _, _, first = pdc.depth(hs, c.p, 70, c.md, seed=SEED)
    m2, c2, second = pdc.depth(hs, c.p, 70, c.md, seed=SEED)
    _, _, smaller = pdc.depth(hs, c.p[:3], 5, c.md, seed=SEED)
    assert first["grew"] == 1 and second["grew"] == 0 and smaller["grew"] == 0
    assert second["staged_bytes"] == first["staged_bytes"] >= 65 * 70 * 48
    wm, wc = c.want(hip, N_MAX, 70)
    assert_equal(m2, wm, "second call")
    assert np.array_equal(c2, wc)
    # the staging is the ray queries': a closest-hit query of the same size allocates nothing either
    o = np.repeat(c.p, 70, axis=0)
    _, info = hs.query_closest(DevBuf(o), DevBuf(o), want=("t",), out={"t": DevBuf(shape=(len(o),), dtype=f64)})
    assert info["grew"] == 0
    hs.close()


# ---------------------------------------------------------------- 3. live scene, ordering
def test_live_scene_and_ordering(pkg, hip, cases):
    """After one update, one deform, one set_visibility and one add_objects the live handle answers like a fresh scene of the edited
    description; and an edit issued right behind an enqueued call leaves that call's result what it was before the edit."""
    c = cases("sah")
    p, md = c.p, c.md
    sd, (objs, tris) = split(hip, c.sd, [PLASTIC_SPHERE])
    hs = hip.HipScene(sd, builder="sah")
    spp = 70

    def check(fresh_sd, what):
        fresh = hip.HipScene(fresh_sd, builder="sah")
        lm, lc, _ = pdc.depth(hs, p, spp, md, seed=SEED)
        wm, wc, _ = pdc.depth(fresh, p, spp, md, seed=SEED)
        assert_equal(lm, wm, what + ", moments")
        assert np.array_equal(lc, wc), what
        fresh.close()
        return lm, lc

    before_m, before_c, _ = pdc.depth(hs, p, spp, md, seed=SEED)
    # ordering: enqueue, edit at once, only then read back
    out = pdc.depth_outputs(N_MAX)
    hs.query_probe_depth(DevBuf(p), spp, md, seed=SEED, out=out)
    m = translate(40, 0, -30)
    hs.update([(SHORT, m)])
    assert_equal(out["moments"].get(), before_m, "an update right behind the call, moments")
    assert np.array_equal(out["counts"].get(), before_c)
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    after_m, _ = check(now, "update")
    assert (after_m != before_m).any()  # the box moved: the maps saw it
    pos = wave(object_positions(sd, SHORT))
    hs.deform([(SHORT, pos)])
    now = deformed_scene(pkg, hip, sd, {SHORT: pos}, {SHORT: m})
    check(now, "deform")
    hs.set_visibility([(SHORT, False)])
    csd, _ = hip.compact_scene(now, mask_hiding(now, [SHORT]))
    check(csd, "set_visibility")
    hs.set_visibility([(SHORT, True)])
    wm, wc, _ = pdc.depth(hs, p, spp, md, seed=SEED)
    out = pdc.depth_outputs(N_MAX)
    hs.query_probe_depth(DevBuf(p), spp, md, seed=SEED, out=out)
    hs.add_objects(objs, tris if len(tris) else None)  # right behind an enqueued call
    assert_equal(out["moments"].get(), wm, "add_objects right behind the call")
    assert np.array_equal(out["counts"].get(), wc)
    check(extend_numpy(now, objs, tris, []), "add_objects")
    hs.close()


# ---------------------------------------------------------------- 4. the lookup
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_device_lookup_equals_host_lookup(hip, cases, name):
    hs = cases("sah").hs
    origin, spacing, dims = GRIDS[name]
    rng = np.random.default_rng(17)
    sh, mom, cnt = volume(rng, origin, spacing, dims)
    cnt[::3] = (24, 20)  # dead at backface_max 0.25
    p = lookup_points(rng, origin, spacing, dims, 150)
    n = unit(rng, len(p))
    dsh, dmom, dcnt, dp, dn = DevBuf(sh), DevBuf(mom), DevBuf(cnt, dtype=np.int32), DevBuf(p), DevBuf(n)
    for nb, bm in ((0.0, 0.25), (0.15, 0.25), (0.05, 1.0), (0.0, 0.0)):
        out = pdc.Guarded((len(p), 3))
        wt = pdc.Guarded((len(p),))
        hs.probe_shade_visible(origin, spacing, dims, dsh, dmom, dcnt, dp, dn, normal_bias=nb, backface_max=bm, weight=wt, out=out)
        want, wa = hip.probe_shade_visible(origin, spacing, dims, sh, mom, cnt, p, n, normal_bias=nb, backface_max=bm, weight=True)
        assert_equal(out.get(), want, "%s, bias %g, backface_max %g" % (name, nb, bm))
        assert_equal(wt.get(), wa, "%s, weights" % name)
    # without a weight buffer, and with every probe dead (the plain lookup, equal bits)
    out = pdc.Guarded((len(p), 3))
    hs.probe_shade_visible(origin, spacing, dims, dsh, dmom, dcnt, dp, dn, out=out)
    assert_equal(out.get(), hip.probe_shade_visible(origin, spacing, dims, sh, mom, cnt, p, n), name + ", no weights")
    cnt[:] = (8, 8)
    plain = pdc.Guarded((len(p), 3))
    hs.probe_shade(origin, spacing, dims, dsh, dp, dn, out=plain)
    out = pdc.Guarded((len(p), 3))
    hs.probe_shade_visible(origin, spacing, dims, dsh, dmom, DevBuf(cnt, dtype=np.int32), dp, dn, out=out)
    assert_equal(out.get(), plain.get(), name + ", all dead")


# ---------------------------------------------------------------- 5. the composite
def test_bake_probe_volume_equals_its_pieces(hip, cases):
    c = cases("sah")
    hs = hip.HipScene(c.sd, builder="sah")
    origin, spacing, dims = (60.0, 60.0, 60.0), (110.0, 140.0, 90.0), (5, 4, 5)  # 100 probes inside the Cornell box
    kw = dict(spp=4, seed=11)
    out = {"sh": pdc.Guarded((100, 27)), **pdc.depth_outputs(100)}
    _, _, _, st = hs.bake_probe_volume(origin, spacing, dims, 70, 200.0, depth_seed=5, out=out, **kw)
    assert st.samples == 100 * 4
    pts = hip.probe_grid_points(origin, spacing, dims)
    want_sh, _, _, _ = pc.probes(c.hs, pts, radiance=False, **kw)
    want_m, want_c, _ = pdc.depth(c.hs, pts, 70, 200.0, seed=5)
    assert_equal(out["sh"].get(), want_sh, "sh against bake_probe_grid's pieces")
    assert_equal(out["moments"].get(), want_m, "moments against query_probe_depth at the grid's points")
    assert np.array_equal(out["counts"].get(), want_c)
    baked = pdc.Guarded((100, 27))
    hs.bake_probe_grid(origin, spacing, dims, out=baked, **kw)
    assert_equal(baked.get(), want_sh, "bake_probe_grid")
    hs.close()


# ---------------------------------------------------------------- 6. refusals on the device
def test_refusals_and_edges(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    n = 16
    dp = DevBuf(c.p[:n])
    out = pdc.depth_outputs(n)
    host = np.zeros((n, 192), f32)

    def params(seed=1, spp=4, sample_offset=0, accumulate=0, max_distance=2.0, reserved=(0, 0, 0)):
        return hip.ProbeDepthParams(seed, spp, sample_offset, accumulate, max_distance, (C.c_int32 * 3)(*reserved))

    def call(p=None, n=n, origins=dp.ptr, moments=out["moments"].ptr, counts=out["counts"].ptr):
        return L.mcpt_query_probe_depth(hs.h, C.byref(p or params()), n, origins, moments, counts, None, None)

    for kw, word in ((dict(origins=host.ctypes.data), b"device"), (dict(moments=host.ctypes.data), b"device"), (dict(counts=host.ctypes.data), b"device"),
                     (dict(n=-1), b"n must"), (dict(n=(2 ** 31 - 1) // 192 + 1), b"n must"), (dict(p=params(spp=0)), b"spp"),
                     (dict(p=params(sample_offset=-1)), b"sample_offset"), (dict(p=params(spp=2 ** 30, sample_offset=2 ** 30)), b"2^31"),
                     (dict(p=params(accumulate=2)), b"accumulate"), (dict(p=params(max_distance=0.0)), b"max_distance"),
                     (dict(p=params(max_distance=-1.0)), b"max_distance"), (dict(p=params(max_distance=float("inf"))), b"max_distance"),
                     (dict(p=params(max_distance=float("nan"))), b"max_distance"), (dict(p=params(reserved=(0, 0, 1))), b"reserved"),
                     (dict(origins=None), b"null"), (dict(moments=None), b"null"), (dict(counts=None), b"null")):
        rc = call(**kw)
        assert rc == 1 and b"mcpt_query_probe_depth" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
    assert L.mcpt_query_probe_depth(hs.h, None, n, dp.ptr, out["moments"].ptr, out["counts"].ptr, None, None) == 1
    assert (out["moments"].get() == f32(SENTINEL)).all() and (out["counts"].get() == pdc.COUNT_SENTINEL).all()  # nothing was written
    assert call(n=0) == 0 and call(n=0, origins=None, moments=None, counts=None) == 0  # a valid no-op
    assert (out["moments"].get() == f32(SENTINEL)).all()
    # the lookup and the composite: pointers off the device, bad options
    g = hip.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(0, 0, 0))
    sh8, m8, c8 = DevBuf(np.zeros((8, 27), f32)), DevBuf(np.zeros((8, 192), f32)), DevBuf(np.zeros((8, 2), np.int32), dtype=np.int32)
    res = pdc.Guarded((n, 3))
    o = hip.ProbeVisibility(0.0, 0.25, (C.c_int32 * 2)(0, 0))

    def look(sh=sh8.ptr, mom=m8.ptr, cnt=c8.ptr, opts=o, pts=dp.ptr, nrm=dp.ptr, dst=res.ptr, wt=None, grid=g):
        return L.mcpt_probe_shade_visible(hs.h, C.byref(grid), sh, mom, cnt, C.byref(opts), n, pts, nrm, dst, wt, None)

    bad_grid = hip.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 0, 1), (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(0, 0, 0))
    for kw, word in ((dict(sh=host.ctypes.data), b"device"), (dict(mom=host.ctypes.data), b"device"), (dict(cnt=host.ctypes.data), b"device"),
                     (dict(pts=host.ctypes.data), b"device"), (dict(dst=host.ctypes.data), b"device"), (dict(wt=host.ctypes.data), b"device"),
                     (dict(opts=hip.ProbeVisibility(-1.0, 0.25, (C.c_int32 * 2)(0, 0))), b"normal_bias"),
                     (dict(opts=hip.ProbeVisibility(0.0, float("nan"), (C.c_int32 * 2)(0, 0))), b"backface_max"),
                     (dict(opts=hip.ProbeVisibility(0.0, 0.25, (C.c_int32 * 2)(1, 0))), b"reserved"), (dict(grid=bad_grid), b"spacing"),
                     (dict(mom=None), b"null")):
        rc = look(**kw)
        assert rc == 1 and b"mcpt_probe_shade_visible" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
    assert (res.get() == f32(SENTINEL)).all()
    prm = hs.params(spp=2, seed=1)
    assert L.mcpt_bake_probe_volume(hs.h, C.byref(g), C.byref(prm), C.byref(params()), sh8.ptr, host.ctypes.data, c8.ptr, None, None) == 1 and b"device" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_volume(hs.h, C.byref(g), C.byref(prm), C.byref(params(spp=0)), sh8.ptr, m8.ptr, c8.ptr, None, None) == 1 and b"spp" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_volume(hs.h, C.byref(g), C.byref(hs.params(spp=0)), C.byref(params()), sh8.ptr, m8.ptr, c8.ptr, None, None) == 1
    assert L.mcpt_bake_probe_volume(hs.h, C.byref(bad_grid), C.byref(prm), C.byref(params()), sh8.ptr, m8.ptr, c8.ptr, None, None) == 1 and b"spacing" in L.mcpt_last_error()
    assert not sh8.get().any() and not m8.get().any() and not c8.get().any()
    # one probe, one sample; and the scene still answers as before
    m1, c1, _ = pdc.depth(hs, c.p[:1], 1, c.md, seed=SEED)
    wm, wc = c.want(hip, 1, 1)
    assert_equal(m1, wm, "n = 1, spp = 1")
    assert np.array_equal(c1, wc)


# ---------------------------------------------------------------- 7. what it is for
def quad(a, b, c, d):
    """Two triangles (a, b, c), (a, c, d): the normal is (b - a) x (c - a)."""
    return [(a, b, c), (a, c, d)]


def box_tris(pkg, lo, hi, outward=True):
    """The twelve triangles of an axis-aligned box, every normal pointing out of it (outward) or into it."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)),  # -x
             ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),  # +x
             ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)),  # -y
             ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),  # +y
             ((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)),  # -z
             ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))]  # +z
    t = []
    for f in faces:
        t += quad(*(f if outward else f[::-1]))
    tris = np.zeros(len(t), dtype=pkg.scenes.TRI_DTYPE)
    for k, (a, b, c) in enumerate(t):
        tris["v0"][k], tris["v1"][k], tris["v2"][k] = f32(a), f32(b), f32(c)
    return tris


def test_box_helper_orientation(pkg):
    """The helper the two scenes below rest on: cross(v1 - v0, v2 - v0) points away from the centre of an outward box."""
    for outward in (True, False):
        t = box_tris(pkg, (0, 0, 0), (2, 3, 4), outward)
        nrm = np.cross(t["v1"] - t["v0"], t["v2"] - t["v0"])
        mid = (t["v0"] + t["v1"] + t["v2"]) / 3 - np.array([1, 1.5, 2])
        s = np.einsum("ij,ij->i", nrm, mid)
        assert len(t) == 12 and ((s > 0) if outward else (s < 0)).all()


def room_scene(pkg, hi, emitter, extra=()):
    """A sealed room [0, hi] whose walls face inward, a square emitter just below its ceiling facing down, background 0, and closed
    outward-facing boxes inside it."""
    S = pkg.scenes
    b = S._Builder()
    white = b.material("white", S.material_presets()["rough_white_conductor"])
    light = b.material("light", S._mat(S.ROUGH_CONDUCTOR, emission=S.light_emission(1.0)))
    b.add_mesh(box_tris(pkg, (0, 0, 0), hi, outward=False), white)
    for lo_, hi_ in extra:
        b.add_mesh(box_tris(pkg, lo_, hi_, outward=True), white)
    (x0, z0), (x1, z1), y = emitter[0], emitter[1], hi[1] - 0.01
    lt = np.zeros(2, dtype=S.TRI_DTYPE)
    for k, (a, bb, cc) in enumerate(quad((x0, y, z0), (x1, y, z0), (x1, y, z1), (x0, y, z1))):  # normal (0, -1, 0)
        lt["v0"][k], lt["v1"][k], lt["v2"][k] = f32(a), f32(bb), f32(cc)
    b.add_mesh(lt, light)
    cam = S.make_camera(32, 32, 40, (1, 1, -5), (1, 1, 0))
    return b.finish(camera=cam, rr_rate=0.7, spp=4, name="rooms", background=np.zeros(3, f32))


def bake(hs, grid, spp, depth_spp, max_distance):
    m = grid[2][0] * grid[2][1] * grid[2][2]
    out = {"sh": pdc.Guarded((m, 27)), **pdc.depth_outputs(m)}
    hs.bake_probe_volume(*grid, depth_spp, max_distance, depth_seed=3, out=out, spp=spp, seed=2)
    return out


def test_light_does_not_leak_through_a_wall(pkg, hip):
    """Two sealed rooms share a wall, a slab 0.1 thick at x = 2; the emitter is in room A (x < 2) only, the background is 0.  A 4 x 2 x 2
    grid has the wall between its probe columns 1 (x = 1.5) and 2 (x = 2.5).  Points of room B near the wall: the HEMISPHERE sensors there
    are exactly 0 (the scene is what it should be), the plain lookup is positive (it leaks), and the occlusion-aware lookup lies strictly
    between 0 and the plain value at every point and channel.  Printed and recorded in DESIGN.md, not asserted: the summed ratio visible / plain
    (0.049 on an MI355X, largest single ratio 0.52)."""
    sd = room_scene(pkg, (4.0, 2.0, 2.0), ((0.6, 0.6), (1.4, 1.4)), extra=[((1.95, 0.0, 0.0), (2.05, 2.0, 2.0))])
    hs = hip.HipScene(sd, builder="sah")
    grid = ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (4, 2, 2))
    vol = bake(hs, grid, 512, 512, 3.0)
    rng = np.random.default_rng(4)
    P = np.stack([rng.uniform(2.2, 2.45, 24), rng.uniform(0.6, 1.4, 24), rng.uniform(0.6, 1.4, 24)], axis=1).astype(f32)
    N = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]], f32)
    p, n = np.repeat(P, len(N), axis=0), np.tile(N, (len(P), 1))
    dp, dn = DevBuf(p), DevBuf(n)
    so = {"radiance": pdc.Guarded((len(p), 3))}
    hs.query_radiance(dp, dn, kind="hemisphere", out=so, spp=64, seed=5)
    truth = so["radiance"].get()
    assert (truth == 0).all(), "room B is not dark: the scene of this test is wrong"
    sh = vol["sh"].get()
    assert (sh[pc.grid_points(*grid)[:, 0] > 2].reshape(-1) == 0).all() and (sh[:, 0:3] >= 0).all()  # the probes of room B saw nothing
    plain = pdc.Guarded((len(p), 3))
    hs.probe_shade(*grid, vol["sh"], dp, dn, out=plain)
    plain = plain.get()
    assert (plain > 0).all(), "the plain lookup does not leak here: the test would show nothing"
    vis = pdc.Guarded((len(p), 3))
    hs.probe_shade_visible(*grid, vol["sh"], vol["moments"], vol["counts"], dp, dn, normal_bias=0.02, backface_max=0.25, out=vis)
    vis = vis.get()
    ratio = vis.astype(f64).sum() / plain.astype(f64).sum()
    print("\n[probe depth] leak through the wall: sum visible / sum plain = %.4g; largest single ratio %.4g" % (ratio, (vis / plain).max()))
    assert ((vis > 0) & (vis < plain)).all(), "%d of %d values are not strictly between 0 and the plain lookup" % (int((~((vis > 0) & (vis < plain))).sum()), vis.size)
    cn = vol["counts"].get()
    assert (cn[:, 0] == 512).all() and (cn[:, 1] == 0).all()  # inward rooms, an outward slab: nobody sees a back face
    hs.close()


def test_a_buried_probe_is_retired(pkg, hip):
    """Probe 1 of a 3 x 2 x 2 grid sits inside a closed, outward-oriented box: every one of its rays hits the box from inside, so all spp
    samples are back-facing; with backface_max = 0.25 a lookup in the cells around it equals the restated lookup with that probe's weight
    forced to 0 (nothing else is dead: no other probe sees a back face)."""
    sd = room_scene(pkg, (2.0, 2.0, 2.0), ((0.6, 0.6), (1.4, 1.4)), extra=[((0.85, 0.35, 0.35), (1.15, 0.65, 0.65))])
    hs = hip.HipScene(sd, builder="sah")
    grid = ((0.5, 0.5, 0.5), (0.5, 1.0, 1.0), (3, 2, 2))
    assert np.array_equal(pc.grid_points(*grid)[1], f32([1.0, 0.5, 0.5]))
    spp = 256
    vol = bake(hs, grid, 256, spp, 2.0)
    sh, mom, cn = vol["sh"].get(), vol["moments"].get(), vol["counts"].get()
    assert cn[1, 0] == spp and cn[1, 1] == spp
    assert (np.delete(cn[:, 1], 1) == 0).all() and (cn[:, 0] == spp).all()
    rng = np.random.default_rng(8)
    p = np.stack([rng.uniform(0.55, 1.45, 96), rng.uniform(0.7, 1.2, 96), rng.uniform(0.7, 1.2, 96)], axis=1).astype(f32)  # both cells beside it
    n = unit(rng, len(p))
    out = pdc.Guarded((len(p), 3))
    hs.probe_shade_visible(*grid, vol["sh"], vol["moments"], vol["counts"], DevBuf(p), DevBuf(n), normal_bias=0.0, backface_max=0.25, out=out)
    got = out.get()
    want, _ = pdc.shade_visible(*grid, sh, mom, cn * 0, p, n, 0.0, 0.25, kill=[1])
    assert_equal(got, want, "probe 1 retired")
    # With its depth map the probe hardly counts anyway (the map says "0.15 away in every direction", so Chebyshev gives it next to
    # nothing): the back-face rule is what is left when the map cannot tell, shown here with the maps zeroed (W == 0: ch = 1).
    zero = DevBuf(np.zeros_like(mom))
    res = {}
    for bm in (0.25, 1.0):
        out = pdc.Guarded((len(p), 3))
        hs.probe_shade_visible(*grid, vol["sh"], zero, vol["counts"], DevBuf(p), DevBuf(n), normal_bias=0.0, backface_max=bm, out=out)
        res[bm] = out.get()
    assert_equal(res[0.25], pdc.shade_visible(*grid, sh, mom * 0, cn * 0, p, n, 0.0, 0.25, kill=[1])[0], "no maps, probe 1 retired")
    assert_equal(res[1.0], pdc.shade_visible(*grid, sh, mom * 0, cn * 0, p, n, 0.0, 0.25)[0], "no maps, probe 1 alive")
    assert (res[0.25] != res[1.0]).any(axis=1).mean() > 0.9  # alive, the dark probe would have counted
    hs.close()


# ---------------------------------------------------------------- 8. torch and streams
def test_torch_tensors_on_a_side_stream():
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_depth_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["n"] == 65 and rec["on_side_stream"] and rec["outputs_are_torch"]
    assert rec["moments_differ"] == 0 and rec["counts_differ"] == 0 and rec["shade_differ"] == 0 and rec["volume_differ"] == 0
    assert rec["non_contiguous_refused"]
