"""mcpt_query_radiance / mcpt_sensor_rays on the GPU: radiance at sensors that sit in device memory.

The expected value everywhere is the numpy float32 fold of hs.cast_rays on the same handle, in sample order, divided by
np.float32(spp_total) (tests/sensor_query_cases.py): bits are compared where the expectation is finite, NaN-ness where it is not.  The
reference for a live scene is a freshly created scene of the edited description.  Device buffers are made without torch
(tests/ray_query_cases.py), every output is followed by 64 guard elements that must survive.  torch and a non-default stream:
tests/sensor_query_torch_child.py, a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chain_scene import chain_scene  # noqa: E402
from deform_cases import SHORT, deformed_scene, translate  # noqa: E402
from material_edit_cases import edited_scene, with_fields  # noqa: E402
from mirror_scene import mirror_scene  # noqa: E402
from ray_query_cases import DevBuf  # noqa: E402
from sensor_query_cases import (K_EPS, SENTINEL, cast_values, fold, hemisphere_f64, hemisphere_pairs, outputs, radiance, rays_805, same_bits,  # noqa: E402
                                surface_sensors, variance_f64)
from visibility_cases import mask_hiding  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
PARITY = dict(spp=5, spp_per_pass=2, pool_paths=3 * 1024, seed=9)  # three passes, two in flight, a last pass of one sample; both paths of split_sample
CAST = ("seed", "n_dir_sample", "max_depth")  # the members of params both calls read


def cast_kw(kw):
    return {k: v for k, v in kw.items() if k in CAST}


def assert_equal(got, want, what=""):
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


class Case:
    """A scene with 805 rays and 805 surface sensors: made once, shared, never changed."""

    def __init__(self, hs, sd):
        self.hs, self.sd = hs, sd
        self.o, self.d = rays_805(hs, sd)
        self.hit = hs.intersect(self.o, self.d)[1] >= 0
        self._surface = None

    def surface(self):
        if self._surface is None:
            self._surface = surface_sensors(self.hs, self.sd)
        return self._surface


@pytest.fixture(scope="module")
def cases(pkg, hip):
    made = {}

    def get(name):
        if name not in made:
            if name == "chess":  # sah, quantised; smooth conductors: the short path of primary_sample
                sd = pkg.scenes.chess_scene(width=160, height=90, spp=4)
                hs = hip.HipScene(sd, builder="sah", quantise=1)
                assert hs.info()["quantised"] == 1
            elif name == "mirrors":
                sd = mirror_scene(pkg)
                hs = hip.HipScene(sd, builder="sah")
            else:  # the LDS-resident flavour under every builder
                sd = pkg.scenes.cornell_demo(64, 64, 4)
                hs = hip.HipScene(sd, builder=name)
                assert hs.info()["lds_resident"] == 1
            made[name] = Case(hs, sd)
        return made[name]

    yield get
    for c in made.values():
        c.hs.close()


# ---------------------------------------------------------------- 1. parity, kind RAY
@pytest.mark.parametrize("name", ["sah", "reference", "lbvh", "ploc", "chess", "mirrors"])
def test_ray_sensors_equal_cast_rays(cases, name):
    c = cases(name)
    assert c.hit.mean() >= 0.3, c.hit.mean()
    want = fold(cast_values(c.hs, c.o, c.d, PARITY["spp"], **cast_kw(PARITY)))
    got, _, st = radiance(c.hs, c.o, c.d, **PARITY)
    assert st.samples == 805 * 5
    assert_equal(got, want, name)


def test_two_pools(hip, cases, monkeypatch):
    """MCPT_POOLS=2 with every pass large enough for both: the second branch of render_list, each pool on half of every pass."""
    c = cases("chess")
    monkeypatch.setenv("MCPT_POOLS", "2")
    monkeypatch.setenv("MCPT_POOL_MIN_WORK", "1")
    hs = hip.HipScene(c.sd, builder="sah", quantise=1)
    monkeypatch.delenv("MCPT_POOLS")
    monkeypatch.delenv("MCPT_POOL_MIN_WORK")
    kw = dict(spp=5, spp_per_pass=2, pool_paths=6 * 1024, seed=9)
    got, var, _ = radiance(hs, c.o, c.d, variance=True, **kw)
    v = cast_values(c.hs, c.o, c.d, 5, seed=9)
    assert_equal(got, fold(v), "two pools")
    assert_equal(var, radiance(c.hs, c.o, c.d, variance=True, **kw)[1], "two pools, variance")  # (one pool: the same sums in the same order)
    p, nrm = c.surface()
    o2, d2 = hemisphere_pairs(c.hs, p, nrm, 5, seed=9)
    assert_equal(radiance(hs, p, nrm, kind="hemisphere", **kw)[0], fold(cast_values(c.hs, o2, d2, 5, seed=9)), "two pools, hemisphere")
    hs.close()


# ---------------------------------------------------------------- 2. the retry flavour
def test_retry_flavour(pkg, hip):
    """A tree deeper than every LDS stack: the first rays that lose an entry go through k_sensor_primary_retrace."""
    sd = chain_scene(pkg, 40)
    hs = hip.HipScene(sd, builder="lbvh")
    assert hs.info()["bvh_height"] > 24
    rng = np.random.default_rng(6)
    m = 300
    o = np.concatenate([rng.uniform(-0.9, -0.1, (m, 2)), np.full((m, 1), -5.0)], axis=1).astype(f32)
    d = np.tile(np.array([0, 0, 1], f32), (m, 1))
    o2 = rng.uniform(-2, 2, (m, 3)).astype(f32)
    d2 = rng.normal(size=(m, 3))
    d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(f32)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    assert (hs.intersect(o, d)[1] >= 0).sum() >= m
    want = fold(cast_values(hs, o, d, 3, seed=4))
    got, _, _ = radiance(hs, o, d, spp=3, seed=4)
    assert_equal(got, want, "chain scene")
    hs.close()


# ---------------------------------------------------------------- 3. hemisphere rays
def unit_normals(rng, n):
    """Random unit normals with the axis-aligned ones among them, and pairs on both sides of |n.x| > |n.y| (the branches of toWorld)."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v.astype(f32)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(f32)
    v[:6] = axes
    v[6] = (f32(np.sqrt(0.5)), f32(np.sqrt(0.5)), 0)  # |n.x| == |n.y|: the else branch
    return v


def test_hemisphere_rays(cases, oracle):
    hs = cases("sah").hs
    rng = np.random.default_rng(12)
    n_s, n = 512, 4096
    nrm = unit_normals(rng, n_s)
    p = rng.uniform(-1, 1, (n_s, 3)).astype(f32)
    sensor = np.concatenate([np.arange(n_s), rng.integers(0, n_s, n - n_s)]).astype(np.uint32)
    sample = rng.integers(0, 1000, n).astype(np.uint32)
    o, d = hs.sensor_rays("hemisphere", p, nrm, sensor, sample, seed=77)
    assert (np.abs(nrm[sensor, 0]) > np.abs(nrm[sensor, 1])).sum() > 1000 and (np.abs(nrm[sensor, 0]) <= np.abs(nrm[sensor, 1])).sum() > 1000
    # (i) the rule in float64
    o64, d64 = hemisphere_f64(oracle, p, nrm, sensor, sample, 77)
    e_o, e_d = np.abs(o - o64).max(), np.abs(d - d64).max()
    print("\n[sensor] hemisphere rays vs float64: |origin error| %.3g, |direction error| %.3g" % (e_o, e_d))
    assert e_o <= 2e-6 and e_d <= 2e-6
    # (ii) unit length, the upper hemisphere, the offset origin in float32
    ln = np.linalg.norm(d.astype(f64), axis=1)
    dn = (d.astype(f64) * nrm[sensor].astype(f64)).sum(1)
    print("[sensor] max |d| - 1 = %.3g, min d.n = %.3g" % ((ln - 1).max(), dn.min()))
    assert (ln - 1).max() <= 4e-7 and dn.min() >= -4e-7
    want_o = (p[sensor] + (nrm[sensor] * K_EPS).astype(f32)).astype(f32)
    assert np.array_equal(o.view(np.uint32), want_o.view(np.uint32))
    # kind RAY returns the inputs of the named sensors
    ro, rd = hs.sensor_rays("ray", p, nrm, sensor, sample, seed=77)
    assert np.array_equal(ro.view(np.uint32), p[sensor].view(np.uint32)) and np.array_equal(rd.view(np.uint32), nrm[sensor].view(np.uint32))
    # (iii) cosine weighting: E[cos] = 2/3, Var[cos] = 1/2 - 4/9 = 1/18
    m = 65536
    n1 = unit_normals(np.random.default_rng(13), 8)[7:8]
    _, dm = hs.sensor_rays("hemisphere", np.zeros((1, 3), f32), n1, np.zeros(m, np.uint32), np.arange(m, dtype=np.uint32), seed=5)
    mean = float((dm.astype(f64) * n1.astype(f64)).sum(1).mean())
    print("[sensor] mean d.n over %d samples: %.5f (2/3 = %.5f)" % (m, mean, 2 / 3))
    assert abs(mean - 2 / 3) <= 5 * np.sqrt(1 / 18 / m)


# ---------------------------------------------------------------- 4. parity, kind HEMISPHERE
@pytest.mark.parametrize("name", ["sah", "chess"])
def test_hemisphere_sensors_equal_cast_rays(cases, name):
    c = cases(name)
    p, nrm = c.surface()
    o, d = hemisphere_pairs(c.hs, p, nrm, 4, seed=3)
    want = fold(cast_values(c.hs, o, d, 4, seed=3))
    got, _, st = radiance(c.hs, p, nrm, kind="hemisphere", spp=4, seed=3)
    assert st.samples == 805 * 4 and st.paths == 3 * st.samples
    assert_equal(got, want, name)
    assert (want > 0).mean() > 0.3  # light does arrive at the surfaces


# ---------------------------------------------------------------- 5. progressive calls and the variance
def test_progressive_calls(cases):
    c = cases("chess")
    one, _, _ = radiance(c.hs, c.o, c.d, spp=5, seed=9)
    out = outputs(805)
    radiance(c.hs, c.o, c.d, out=out, spp=3, spp_total=5, seed=9)
    two, _, _ = radiance(c.hs, c.o, c.d, out=out, spp=2, sample_offset=3, spp_total=5, accumulate=1, seed=9)
    assert_equal(two, one, "3 + 2 samples")
    v = np.concatenate([cast_values(c.hs, c.o, c.d, 3, seed=9), cast_values(c.hs, c.o, c.d, 2, sample_offset=3, seed=9)], axis=1)
    assert_equal(one, fold(v), "spp 5")


def test_variance(cases):
    c = cases("sah")
    # rays that leave the scene into the constant background: eight equal values, variance exactly 0
    o = np.concatenate([c.o, np.tile(np.array([278, 273, -900], f32), (40, 1))])
    d = np.concatenate([c.d, np.tile(np.array([0, 0, -1], f32), (40, 1))])
    v = cast_values(c.hs, o, d, 8, seed=2)
    got, var, _ = radiance(c.hs, o, d, variance=True, spp=8, seed=2)
    assert_equal(got, fold(v), "radiance beside a variance")
    want = variance_f64(v)
    w32 = want.astype(f32)
    with np.errstate(invalid="ignore"):
        ulp = np.spacing(np.abs(w32))
        ok = (np.abs(var.astype(f64) - want) <= ulp) | (np.isnan(var) & np.isnan(want))
    print("\n[sensor] variance: %d of %d values differ from the float64 evaluation by more than 1 ulp; %d are exactly 0"
          % (int((~ok).sum()), ok.size, int((var == 0).sum())))
    assert ok.all()
    equal = (v == v[:, :1, :]).all(axis=1)
    assert equal[-40:].all() and (var[equal] == 0).all() and (var[~equal] > 0).mean() > 0.9
    # the refusals: nothing is written
    L = c.hs.L
    out = outputs(len(o), True)
    for kw in (dict(spp=1), dict(spp=8, accumulate=1), dict(spp=8, sample_offset=1), dict(spp=8, spp_total=8)):
        with pytest.raises(Exception) as e:
            radiance(c.hs, o, d, variance=True, out=out, seed=2, **kw)
        assert getattr(e.value, "code", None) == 1 and b"variance" in L.mcpt_last_error(), kw
    assert (out["radiance"].get() == f32(SENTINEL)).all() and (out["variance"].get() == f32(SENTINEL)).all()


# ---------------------------------------------------------------- 6. live scene
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_live_scene(pkg, hip, cases, builder):
    """After update, set_visibility and set_materials the live handle answers like a scene freshly created from the edited description;
    a render after the queries equals one before them."""
    sd = cases("sah").sd
    o, d = cases("sah").o, cases("sah").d
    p, nrm = cases("sah").surface()
    device_built = builder == "lbvh"
    allowed = max(3, 805 // 10000) if device_built else 0  # (sensors; a grazing ray may take another side of a box face in a device-built tree)
    hs = hip.HipScene(sd, builder=builder)
    kw = dict(spp=4, seed=6)

    def check(fresh_sd, what):
        fresh = hip.HipScene(fresh_sd, builder=builder)
        before = hs.render(spp=2, seed=3)[0]
        for kind, a, b in (("ray", o, d), ("hemisphere", p, nrm)):
            live, _, _ = radiance(hs, a, b, kind=kind, **kw)
            want, _, _ = radiance(fresh, a, b, kind=kind, **kw)
            differ = int((~same_bits(live, want)).any(axis=1).sum())
            assert differ <= allowed, "%s, %s, %s: %d sensors differ" % (builder, what, kind, differ)
        after = hs.render(spp=2, seed=3)[0]
        assert same_bits(before, after).all(), "%s: the queries changed a render" % what
        fresh.close()

    m = translate(40, 0, -30)
    hs.update([(SHORT, m)])
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    check(now, "update")
    hs.set_visibility([(SHORT, False)])
    csd, _ = hip.compact_scene(now, mask_hiding(now, [SHORT]))
    check(csd, "set_visibility")
    hs.set_visibility([(SHORT, True)])
    mat = int(now.objects["material"][SHORT])
    edit = [(mat, with_fields(now.materials[mat], base_reflectance=(0.1, 0.7, 0.2), roughness=0.3))]
    hs.set_materials(edits=edit)
    check(edited_scene(now, edits=edit), "set_materials")
    hs.close()


# ---------------------------------------------------------------- 7. refusals and edges
def test_refusals_and_edges(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    n = 256
    do, dd = DevBuf(c.o[:n]), DevBuf(c.d[:n])
    out = outputs(n, True)
    host = np.zeros((n, 3), f32)
    p = hs.params(spp=2, seed=1)

    def call(n=n, origins=do.ptr, dirs=dd.ptr, kind=0, reserved=(0, 0, 0), rad=out["radiance"].ptr, var=None, params=p):
        s = hip.SensorBuffers(origins, dirs, kind, (C.c_int32 * 3)(*reserved))
        return L.mcpt_query_radiance(hs.h, C.byref(params), n, C.byref(s), C.byref(hip.SensorOutputs(rad, var)), None, None)

    def refused(rc, word):
        assert rc == 1 and b"mcpt_query_radiance" in L.mcpt_last_error() and word in L.mcpt_last_error(), (rc, L.mcpt_last_error())

    refused(call(origins=host.ctypes.data), b"device")
    refused(call(rad=host.ctypes.data), b"device")
    refused(call(var=host.ctypes.data, params=hs.params(spp=2)), b"device")
    refused(call(n=(2 ** 31 - 1) // 3 + 1), b"n must be")
    refused(call(n=-1), b"n must be")
    refused(call(params=hs.params(spp=2, nranks=2)), b"nranks")
    refused(call(params=hs.params(spp=2, rank=1)), b"nranks")
    refused(call(kind=2), b"kind")
    refused(call(reserved=(0, 0, 5)), b"reserved")
    refused(call(params=hs.params(spp=0)), b"spp")
    refused(call(params=hs.params(spp=2, n_dir_sample=0)), b"n_dir_sample")
    refused(call(origins=None), b"null")
    refused(call(rad=None), b"null")
    assert L.mcpt_query_radiance(hs.h, None, n, None, None, None, None) == 1
    assert (out["radiance"].get() == f32(SENTINEL)).all() and (out["variance"].get() == f32(SENTINEL)).all()  # nothing was written
    assert call(n=0) == 0 and call(n=0, origins=None, dirs=None, rad=None) == 0  # a valid no-op
    assert (out["radiance"].get() == f32(SENTINEL)).all()
    # one sensor, one sample
    got, _, st = radiance(hs, c.o[:1], c.d[:1], spp=1, seed=8)
    assert st.samples == 1
    assert_equal(got, fold(cast_values(hs, c.o[:1], c.d[:1], 1, seed=8)), "n = 1, spp = 1")
    # and the scene still answers as before
    assert_equal(radiance(hs, c.o, c.d, **PARITY)[0], fold(cast_values(hs, c.o, c.d, PARITY["spp"], **cast_kw(PARITY))), "after the refusals")


# ---------------------------------------------------------------- 8. statistics
def test_stats(pkg, hip, cases, monkeypatch):
    c = cases("chess")
    n, spp = 805, 4
    got, _, st = radiance(c.hs, c.o, c.d, spp=spp, seed=5)
    traced, shared = c.hs.ray_counts()
    pc = c.hs.primary_conductor_counts()
    assert st.samples == n * spp and st.paths == 3 * st.samples
    # every resolved ray beyond the first rays is a continuation ray: one that was traced, or one that rode on a sibling's
    assert st.closest_rays - n * spp == traced + shared and traced > 0
    assert pc[0] > 0 and pc[1] > 0, pc
    monkeypatch.setenv("MCPT_PRIMARY_CONDUCTOR", "0")
    off = hip.HipScene(c.sd, builder="sah", quantise=1)
    monkeypatch.delenv("MCPT_PRIMARY_CONDUCTOR")
    got_off, _, st_off = radiance(off, c.o, c.d, spp=spp, seed=5)
    assert off.primary_conductor_counts() == (0, 0)
    assert_equal(got_off, got, "MCPT_PRIMARY_CONDUCTOR=0")
    assert (st_off.samples, st_off.paths, st_off.closest_rays, st_off.shadow_rays) == (st.samples, st.paths, st.closest_rays, st.shadow_rays)
    off.close()
    # with the ray sharing off no record rides on a sibling's ray: the continuation rays are the traced ones, and the radiance is the same
    monkeypatch.setenv("MCPT_SHARE_RAYS", "0")
    own = hip.HipScene(c.sd, builder="sah", quantise=1)
    monkeypatch.delenv("MCPT_SHARE_RAYS")
    got_own, _, st2 = radiance(own, c.o, c.d, spp=spp, seed=5)
    assert own.ray_counts()[1] == 0 and st2.closest_rays - n * spp == own.ray_counts()[0] == traced + shared
    assert_equal(got_own, got, "MCPT_SHARE_RAYS=0")
    own.close()


# ---------------------------------------------------------------- 9. torch and streams
def test_torch_tensors_on_a_side_stream():
    """tests/sensor_query_torch_child.py (torch imported first): sensors produced by a torch kernel on a non-default stream, outputs
    allocated by the call, against the numpy path in the same process."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "sensor_query_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["n"] == 805 and rec["on_side_stream"] and rec["outputs_are_torch"]
    assert rec["ray_differ"] == 0 and rec["hemisphere_differ"] == 0 and rec["variance_differ"] == 0
    assert rec["non_contiguous_refused"]
