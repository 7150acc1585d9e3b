"""mcpt_query_probes / mcpt_probe_rays / mcpt_probe_shade / mcpt_bake_probe_grid on the GPU.

Expected values are compositions of calls that exist without the feature: the first rays come from hs.probe_rays, their values from
hs.cast_rays on the same handle (tests/sensor_query_cases.py: cast_values), the projection from the numpy float32 fold of
tests/probe_cases.py weighted with the HOST basis of those directions; bits are compared where the expectation is finite, NaN-ness where
it is not.  Device buffers are made without torch, every output is followed by 64 guard elements that must survive.  torch and a
non-default stream: tests/probe_torch_child.py, a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_cases as pc  # noqa: E402
from chain_scene import chain_scene  # noqa: E402
from add_cases import extend_numpy, split  # noqa: E402
from deform_cases import PLASTIC_SPHERE, SHORT, deformed_scene, object_positions, translate, wave  # noqa: E402
from ray_query_cases import GUARD, DevBuf  # noqa: E402
from sensor_query_cases import SENTINEL, cast_values, fold, same_bits, variance_f64  # noqa: E402
from visibility_cases import mask_hiding  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
PARITY = dict(spp=5, spp_per_pass=2, pool_paths=3 * 1024, seed=9)  # three passes, two in flight, a last pass of one sample


def assert_equal(got, want, what=""):
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


def want_for(hs, p, spp, seed, sample_offset=0, spp_total=None, start=None):
    """(sh, radiance, values) expected of a call, from probe_rays, cast_rays, the host basis and the numpy folds."""
    o, d = pc.probe_pairs(hs, p, spp, seed, sample_offset)
    v = cast_values(hs, o, d, spp, sample_offset=sample_offset, seed=seed)
    return pc.sh_fold(v, d, spp_total, None if start is None else start[0]), fold(v, spp_total, None if start is None else start[1]), v, d


class Case:
    def __init__(self, hs, sd):
        self.hs, self.sd = hs, sd
        self.p = pc.probe_points(sd)


@pytest.fixture(scope="module")
def cases(pkg, hip):
    made = {}

    def get(name):
        if name not in made:
            if name == "chess":
                sd = pkg.scenes.chess_scene(width=160, height=90, spp=4)
                hs = hip.HipScene(sd, builder="sah", quantise=1)
            else:
                sd = pkg.scenes.cornell_demo(64, 64, 4)
                hs = hip.HipScene(sd, builder=name)
                assert hs.info()["lds_resident"] == 1
            made[name] = Case(hs, sd)
        return made[name]

    yield get
    for c in made.values():
        c.hs.close()


# ---------------------------------------------------------------- 1. directions
def test_probe_rays(cases, oracle, hip):
    hs = cases("sah").hs
    rng = np.random.default_rng(12)
    n_s, n = 256, 2048
    p = rng.uniform(-1, 1, (n_s, 3)).astype(f32)
    sensor = np.concatenate([np.arange(n_s), rng.integers(0, n_s, n - n_s)]).astype(np.uint32)
    sample = rng.integers(0, 1000, n).astype(np.uint32)
    o, d = hs.probe_rays(p, sensor, sample, seed=77)
    o64, d64 = pc.sphere_f64(oracle, p, sensor, sample, 77)
    e_d = np.abs(d - d64).max()
    print("\n[probes] sphere rays vs float64: |direction error| %.3g" % e_d)
    assert e_d <= 2e-6  # (the bound test_hemisphere_rays sets for the same sincos and normalisation)
    assert np.array_equal(o.view(np.uint32), p[sensor].view(np.uint32))  # no offset: the probe itself
    ln = np.linalg.norm(d.astype(f64), axis=1)
    print("[probes] max ||d| - 1| = %.3g" % np.abs(ln - 1).max())
    assert np.abs(ln - 1).max() <= 4e-7
    # uniform over the sphere: E[z] = 0 (Var 1/3), E[Y_j] = 0 and E[Y_j^2] = 1 / (4 pi) for j >= 1
    m = 4096
    _, dm = hs.probe_rays(np.zeros((1, 3), f32), np.zeros(m, np.uint32), np.arange(m, dtype=np.uint32), seed=5)
    mz = float(dm[:, 2].astype(f64).mean())
    Y = hip.sh_basis(dm).astype(f64)
    my = Y[:, 1:].mean(0)
    print("[probes] mean z %.4f, mean Y_j %s over %d samples" % (mz, np.round(my, 4), m))
    assert abs(mz) <= 5 * np.sqrt(1 / 3 / m)
    assert (np.abs(my) <= 5 * np.sqrt(1 / (4 * np.pi) / m)).all()


# ---------------------------------------------------------------- 2. parity of the fold
@pytest.mark.parametrize("name", ["sah", "lbvh", "ploc", "chess"])
def test_fold_equals_cast_rays(cases, name):
    c = cases(name)
    w_sh, w_rad, v, _ = want_for(c.hs, c.p, PARITY["spp"], PARITY["seed"])
    sh, rad, _, st = pc.probes(c.hs, c.p, **PARITY)
    assert st.samples == 805 * 5
    nonzero = (w_sh != 0).any(axis=1).mean()
    print("\n[probes] %s: %.0f %% of the probes have a non-zero sh row" % (name, 100 * nonzero))
    assert nonzero >= 0.5
    assert_equal(sh, w_sh, name + ", sh")
    assert_equal(rad, w_rad, name + ", radiance")
    # the variance: the existing sensor rule (no progressive parameters; passes as above)
    _, rad2, var, _ = pc.probes(c.hs, c.p, variance=True, **PARITY)
    assert_equal(rad2, w_rad, name + ", radiance beside a variance")
    want = variance_f64(v)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(var.astype(f64) - want) <= np.spacing(np.abs(want.astype(f32)))) | (np.isnan(var) & np.isnan(want))
    assert ok.all(), name + ", variance"


def test_dc_term(cases):
    """sh[27i + c] * Y0 against radiance[3i + c]: the same non-negative sum scaled by 4 pi Y0 per term; (spp + 3) roundings apart."""
    c = cases("sah")
    spp = 8
    sh, rad, _, _ = pc.probes(c.hs, c.p, spp=spp, seed=3)
    dc = sh[:, 0:3].astype(f64) * f64(pc.K0)
    fin = np.isfinite(rad) & (rad > 0)
    rel = np.abs(dc[fin] - rad[fin].astype(f64)) / rad[fin].astype(f64)
    print("\n[probes] DC term: largest relative difference %.3g (bound %.3g)" % (rel.max(), (spp + 3) * 2.0 ** -23))
    assert fin.mean() > 0.5 and rel.max() <= (spp + 3) * 2.0 ** -23
    assert (dc[np.isfinite(rad) & (rad == 0)] == 0).all()


def test_two_pools(hip, cases, monkeypatch):
    """MCPT_POOLS=2 with every pass large enough for both: the launch site in the two-pool tail of render_list."""
    c = cases("chess")
    monkeypatch.setenv("MCPT_POOLS", "2")
    monkeypatch.setenv("MCPT_POOL_MIN_WORK", "1")
    hs = hip.HipScene(c.sd, builder="sah", quantise=1)
    monkeypatch.delenv("MCPT_POOLS")
    monkeypatch.delenv("MCPT_POOL_MIN_WORK")
    w_sh, w_rad, _, _ = want_for(c.hs, c.p, 5, 9)
    sh, rad, _, _ = pc.probes(hs, c.p, spp=5, spp_per_pass=2, pool_paths=6 * 1024, seed=9)
    assert_equal(sh, w_sh, "two pools, sh")
    assert_equal(rad, w_rad, "two pools, radiance")
    hs.close()


def test_retry_flavour(pkg, hip):
    """A tree deeper than every LDS stack: first rays that lose an entry go through k_sensor_primary_retrace."""
    sd = chain_scene(pkg, 40)
    hs = hip.HipScene(sd, builder="lbvh")
    assert hs.info()["bvh_height"] > 24
    p = np.random.default_rng(6).uniform(-2, 2, (300, 3)).astype(f32)
    w_sh, w_rad, _, _ = want_for(hs, p, 3, 4)
    sh, rad, _, _ = pc.probes(hs, p, spp=3, seed=4)
    assert_equal(sh, w_sh, "chain scene, sh")
    assert_equal(rad, w_rad, "chain scene, radiance")
    hs.close()


# ---------------------------------------------------------------- 3. progressive calls
def test_progressive_calls(cases):
    c = cases("chess")
    one_sh, one_rad, _, _ = pc.probes(c.hs, c.p, spp=5, seed=9)
    out = pc.probe_outputs(805)
    pc.probes(c.hs, c.p, out=out, spp=3, spp_total=5, seed=9)
    two_sh, two_rad, _, _ = pc.probes(c.hs, c.p, out=out, spp=2, sample_offset=3, spp_total=5, accumulate=1, seed=9)
    assert_equal(two_sh, one_sh, "3 + 2 samples, sh")
    assert_equal(two_rad, one_rad, "3 + 2 samples, radiance")
    assert_equal(one_sh, want_for(c.hs, c.p, 5, 9)[0], "spp 5")


# ---------------------------------------------------------------- 4. live scene
def test_live_scene(pkg, hip, cases):
    """After one update, one deform, one set_visibility and one add_objects the live handle answers like a fresh scene of the edited
    description (builder sah: the host tree of a fresh scene is the tree the live scene rebuilt)."""
    p = cases("sah").p
    sd, (objs, tris) = split(hip, cases("sah").sd, [PLASTIC_SPHERE])  # (the sphere comes back through add_objects; SHORT keeps its index)
    hs = hip.HipScene(sd, builder="sah")
    kw = dict(spp=4, seed=6)

    def check(fresh_sd, what):
        fresh = hip.HipScene(fresh_sd, builder="sah")
        live, lrad, _, _ = pc.probes(hs, p, **kw)
        want, wrad, _, _ = pc.probes(fresh, p, **kw)
        assert_equal(live, want, what + ", sh")
        assert_equal(lrad, wrad, what + ", radiance")
        fresh.close()

    m = translate(40, 0, -30)
    hs.update([(SHORT, m)])
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    check(now, "update")
    pos = wave(object_positions(sd, SHORT))  # base positions: the transform above still applies to them
    hs.deform([(SHORT, pos)])
    now = deformed_scene(pkg, hip, sd, {SHORT: pos}, {SHORT: m})
    check(now, "deform")
    hs.set_visibility([(SHORT, False)])
    csd, _ = hip.compact_scene(now, mask_hiding(now, [SHORT]))
    check(csd, "set_visibility")
    hs.set_visibility([(SHORT, True)])
    hs.add_objects(objs, tris if len(tris) else None)
    check(extend_numpy(now, objs, tris, []), "add_objects")
    hs.close()


# ---------------------------------------------------------------- 5. the lookup
def test_probe_shade_equals_the_host(hip, cases):
    hs = cases("sah").hs
    origin, spacing, dims = (-1.0, 0.5, 2.0), (0.75, 1.5, 0.4), (3, 2, 4)
    rng = np.random.default_rng(8)
    sh = rng.normal(size=(24, 27)).astype(f32)
    ext = np.asarray(spacing) * (np.asarray(dims) - 1)
    p = (np.asarray(origin) + rng.uniform(-0.6, 1.6, (805, 3)) * ext).astype(f32)  # inside and clamped
    p[:24] = hip.probe_grid_points(origin, spacing, dims)                         # on the probes
    n = rng.normal(size=(805, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    out = DevBuf(shape=(805, 3), dtype=f32, fill=SENTINEL, guard=GUARD)
    hs.probe_shade(origin, spacing, dims, DevBuf(sh), DevBuf(p), DevBuf(n), out=out)
    assert_equal(out.get(), hip.probe_shade(origin, spacing, dims, sh, p, n), "device against host")
    for g in (((0, 0, 0), (1, 1, 1), (1, 1, 1)), ((10.0, -3.0, 0.0), (2.0, 1.0, 0.25), (4, 1, 3))):
        m = g[2][0] * g[2][1] * g[2][2]
        out = DevBuf(shape=(37, 3), dtype=f32, fill=SENTINEL, guard=GUARD)
        hs.probe_shade(*g, DevBuf(sh[:m]), DevBuf(p[:37]), DevBuf(n[:37]), out=out)
        assert_equal(out.get(), hip.probe_shade(*g, sh[:m], p[:37], n[:37]), "dims %s" % (g[2],))


# ---------------------------------------------------------------- 6. the composite
def test_bake_probe_grid(hip, cases):
    c = cases("sah")
    hs = hip.HipScene(c.sd, builder="sah")
    origin, spacing, dims = (60.0, 60.0, 60.0), (110.0, 140.0, 90.0), (5, 4, 5)  # 100 probes inside the Cornell box
    kw = dict(spp=4, seed=11)
    out = DevBuf(shape=(100, 27), dtype=f32, fill=SENTINEL, guard=GUARD)
    _, st = hs.bake_probe_grid(origin, spacing, dims, out=out, **kw)
    assert st.samples == 100 * 4
    pts = hip.probe_grid_points(origin, spacing, dims)
    want, _, _, _ = pc.probes(c.hs, pts, radiance=False, **kw)
    got = out.get()
    assert_equal(got, want, "bake against grid points + query_probes")
    assert (got != 0).any(axis=1).mean() >= 0.5
    floats, allocs = hs.probe_buffers()
    assert floats >= 100 * 6 and allocs >= 2  # the points and the stand-in radiance
    again = DevBuf(shape=(100, 27), dtype=f32, fill=SENTINEL, guard=GUARD)
    hs.bake_probe_grid(origin, spacing, dims, out=again, **kw)
    assert hs.probe_buffers() == (floats, allocs), "a second bake of the same size allocated"
    assert_equal(again.get(), got, "second bake")
    hs.close()


# ---------------------------------------------------------------- 7. guards, refusals and edges
def test_refusals_and_edges(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    n = 256
    dp = DevBuf(c.p[:n])
    out = pc.probe_outputs(n, variance=True)
    host = np.zeros((n, 27), f32)
    p = hs.params(spp=2, seed=1)

    def call(n=n, origins=dp.ptr, sh=out["sh"].ptr, rad=out["radiance"].ptr, var=None, reserved=None, params=p):
        return L.mcpt_query_probes(hs.h, C.byref(params), n, origins, C.byref(hip.ProbeOutputs(sh, rad, var, reserved)), None, None)

    def refused(rc, word):
        assert rc == 1 and b"mcpt_query_probes" in L.mcpt_last_error() and word in L.mcpt_last_error(), (rc, L.mcpt_last_error())

    refused(call(origins=host.ctypes.data), b"device")
    refused(call(sh=host.ctypes.data), b"device")
    refused(call(rad=host.ctypes.data), b"device")
    refused(call(var=host.ctypes.data), b"device")
    refused(call(n=(2 ** 31 - 1) // 27 + 1), b"n must be")
    refused(call(n=-1), b"n must be")
    refused(call(params=hs.params(spp=2, nranks=2)), b"nranks")
    refused(call(params=hs.params(spp=2, rank=1)), b"nranks")
    refused(call(reserved=8), b"reserved")
    refused(call(params=hs.params(spp=0)), b"spp")
    refused(call(params=hs.params(spp=2, n_dir_sample=0)), b"n_dir_sample")
    refused(call(var=out["variance"].ptr, params=hs.params(spp=1)), b"variance")
    refused(call(var=out["variance"].ptr, params=hs.params(spp=4, accumulate=1)), b"variance")
    refused(call(origins=None), b"null")
    refused(call(sh=None), b"null")
    assert L.mcpt_query_probes(hs.h, None, n, None, None, None, None) == 1
    # the lookup and the bake: pointers off the device, bad grids
    g = hip.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(0, 0, 0))
    sh8 = DevBuf(np.zeros((8, 27), f32))
    assert L.mcpt_probe_shade(hs.h, C.byref(g), host.ctypes.data, n, dp.ptr, dp.ptr, out["radiance"].ptr, None) == 1 and b"device" in L.mcpt_last_error()
    assert L.mcpt_probe_shade(hs.h, C.byref(g), sh8.ptr, n, dp.ptr, dp.ptr, host.ctypes.data, None) == 1 and b"device" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_grid(hs.h, C.byref(g), C.byref(p), host.ctypes.data, None, None) == 1 and b"device" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_grid(hs.h, C.byref(g), C.byref(hs.params(spp=0)), sh8.ptr, None, None) == 1 and b"spp" in L.mcpt_last_error()
    bad = hip.ProbeGrid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 0, 1), (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(0, 0, 0))
    assert L.mcpt_probe_shade(hs.h, C.byref(bad), sh8.ptr, n, dp.ptr, dp.ptr, out["radiance"].ptr, None) == 1 and b"spacing" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_grid(hs.h, C.byref(bad), C.byref(p), sh8.ptr, None, None) == 1 and b"spacing" in L.mcpt_last_error()
    for w in ("sh", "radiance", "variance"):
        assert (out[w].get() == f32(SENTINEL)).all(), w  # nothing was written
    assert not sh8.get().any()
    assert call(n=0) == 0 and call(n=0, origins=None, sh=None, rad=None) == 0  # a valid no-op
    assert (out["sh"].get() == f32(SENTINEL)).all()
    # one probe, one sample; sh alone (the scene's buffer stands in for the radiance)
    sh1, none, _, st = pc.probes(hs, c.p[:1], radiance=False, spp=1, seed=8)
    assert st.samples == 1 and none is None
    assert_equal(sh1, want_for(hs, c.p[:1], 1, 8)[0], "n = 1, spp = 1")
    # and the scene still answers as before
    assert_equal(pc.probes(hs, c.p, **PARITY)[0], want_for(hs, c.p, PARITY["spp"], PARITY["seed"])[0], "after the refusals")


# ---------------------------------------------------------------- 8. torch and streams
def test_torch_tensors_on_a_side_stream():
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["n"] == 805 and rec["on_side_stream"] and rec["outputs_are_torch"]
    assert rec["sh_differ"] == 0 and rec["radiance_differ"] == 0 and rec["shade_differ"] == 0 and rec["bake_differ"] == 0
    assert rec["non_contiguous_refused"]
