"""The sampled direct term on the GPU: mcpt_query_direct, the indirect-only probes (mcpt_query_probes_ex and the two bakes) and
mcpt_render_probe_lit_direct.

Every expectation of the direct term is the host composition of tests/direct_cases.py -- rng_uniforms, then sample_light, then
direct_samples, then intersect, then direct_fold -- and device bits are compared with it.  The indirect-only probes are compared with
the numpy fold of cast_rays at probe_rays with the masked samples zeroed (the mask from intersect and the description's emitting
objects); the lit frames with a * (max(E, 0) + D) composed from the parts of tests/probe_lit_cases.py.  Device buffers are made without
torch and every output sits between two runs of 64 guard elements that must survive.  torch and a non-default stream:
tests/direct_torch_child.py, a child process."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_cases as dc  # noqa: E402
import mirror_scene as ms  # noqa: E402,F401
import probe_cases as pc  # noqa: E402
import probe_depth_cases as pdc  # noqa: E402
import probe_lit_cases as plc  # noqa: E402
import test_gpu_probe_lit as plit  # noqa: E402  (its scenes and cases; none of its tests run from here)
from add_cases import extend_numpy, split  # noqa: E402
from deform_cases import PLASTIC_SPHERE, SHORT, deformed_scene, object_positions, translate, wave  # noqa: E402
from material_edit_cases import LIGHT, edited_scene, emits, with_fields  # noqa: E402
from ray_query_cases import DevBuf, Rays, closest, scene_extent  # noqa: E402
from sensor_query_cases import SENTINEL, cast_values, fold, same_bits, variance_f64  # noqa: E402
from test_gpu_material import _many_lights  # noqa: E402
from visibility_cases import mask_hiding  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
W, H, WJ, HJ, SPPJ = plit.W, plit.H, plit.WJ, plit.HJ, plit.SPPJ
assert_equal = plit.assert_equal
# (N, seed, key_sample): every sample count of the issue, two seeds, both sample words
COMBOS = ((1, 1, 0), (3, 2, 7), (4, 1, 7), (32, 2, 0))


def upload(a):
    return DevBuf(np.ascontiguousarray(a, f32))


def query(hs, p, nf, N, seed=1, key_sample=0):
    """query_direct on the null stream for points uploaded here, into a guarded buffer -> (D (n, 3), info)."""
    out = pdc.Guarded((len(p), 3))
    _, info = hs.query_direct(upload(p), upload(nf), N, seed=seed, key_sample=key_sample, out=out)
    return out.get(), info


def frame_points(hs, cam):
    """position and facing normal of the centre frame of `cam`: p = o + d * (float)t in float32 (0 on a miss), the AOV record's normal."""
    n_px = int(cam["width"]) * int(cam["height"])
    o, d = hs.centre_rays(np.arange(n_px, dtype=np.uint32), camera=cam)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(hit[:, None], o + d * t.astype(f32)[:, None], f32(0)).astype(f32)
    nf = hs.render_aovs(centre=True, camera=cam).reshape(n_px, 8)[:, 3:6].astype(f32)
    return p, np.ascontiguousarray(nf), hit


def without_emitters(sd):
    mats = sd.materials.copy()
    for i in np.flatnonzero(emits(mats)):
        mats[i] = with_fields(mats[i], emission=(0.0, 0.0, 0.0))
    return dataclasses.replace(sd, materials=mats)


def point_scene(pkg, name):
    if name == "three":
        return _many_lights(pkg), dict(builder="sah")
    if name == "dark":
        return without_emitters(plit.make_scene(pkg, "sah")[0]), dict(builder="sah")
    return plit.make_scene(pkg, name)[:2]


# ---------------------------------------------------------------- 1. points
@pytest.mark.parametrize("name", ["sah", "lbvh", "ploc", "chess", "three", "dark"])
def test_points_equal_the_host_composition(pkg, hip, name):
    sd, kw = point_scene(pkg, name)
    hs = hip.HipScene(sd, **kw)
    if name in ("sah", "lbvh", "ploc"):
        assert hs.info()["lds_resident"] == 1
    if name == "chess":
        assert hs.info()["quantised"] == 1 and int(sd.camera["width"]) == 48 and int(sd.camera["height"]) == 27
    p, nf, hit = frame_points(hs, sd.camera)
    # 64 points below the scene whose normals face away from everything in it, and a point on an emitter itself
    v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]]).astype(f64)
    rng = np.random.default_rng(5)
    away = rng.uniform(v.min(0), v.max(0), (64, 3))
    away[:, 1] = v[:, 1].min() - 1.0
    row = hs.sample_light(np.full((1, 4), 0.5, f32))[0]
    P = np.concatenate([p, away.astype(f32), row[None, 0:3]]).astype(f32)
    NF = np.concatenate([nf, np.tile(f32([0, -1, 0]), (64, 1)), row[None, 3:6]]).astype(f32)
    n_frame = len(p)
    got = {}
    for N, seed, ks in COMBOS:
        D, info = query(hs, P, NF, N, seed=seed, key_sample=ks)
        want, parts = dc.host_direct(hip, hs, P, NF, N, seed=seed, key_sample=ks)
        live, vis = parts["live"] != 0, parts["visible"] != 0
        print("\n[direct] %s, N %d, seed %d, key_sample %d: %d points (%d hit pixels), %.1f %% of the light samples live, %.1f %% visible; "
              "%d launch(es), staged %d KiB" % (name, N, seed, ks, len(P), int(hit.sum()), 100 * live.mean(), 100 * vis.mean(), info["launches"],
                                              info["staged_bytes"] >> 10))
        assert_equal(D, want, "%s, N %d" % (name, N))
        assert not live[n_frame:n_frame + 64].any(), "a point that faces away has a live sample"
        if name == "dark":
            assert hs.info()["n_lights"] == 0 and not D.view(np.uint32).any(), "no emitter: exact +0"
        else:
            assert (D[:n_frame][hit] > 0).any(axis=1).mean() > (0.05 if N >= 4 else 0.0)
            assert (D >= 0).all() and np.isfinite(D).all()
        got[(N, seed, ks)] = D
    if name in ("sah", "lbvh", "ploc"):  # the boxes and spheres cast shadows: live samples that are not visible
        assert (live & ~vis).sum() > 50
    if name != "dark":  # the seed and the sample word are read
        other, _ = query(hs, P, NF, 4, seed=2, key_sample=7)
        assert (other != got[(4, 1, 7)]).any()
        other, _ = query(hs, P, NF, 4, seed=1, key_sample=0)
        assert (other != got[(4, 1, 7)]).any()
    hs.close()


# ---------------------------------------------------------------- 2. chunking, the steady state, torch
def test_chunking_does_not_change_a_bit(pkg, hip, monkeypatch):
    sd, kw = point_scene(pkg, "sah")
    hs = hip.HipScene(sd, **kw)
    p, nf, _ = frame_points(hs, sd.camera)
    p, nf = np.roll(p, len(p) // 2, axis=0), np.roll(nf, len(p) // 2, axis=0)  # (the short runs below start in the middle of the frame)
    monkeypatch.setenv("MCPT_QUERY_CHUNK", "64")
    small = hip.HipScene(sd, **kw)
    monkeypatch.delenv("MCPT_QUERY_CHUNK")
    # whole points per chunk (21 of 3 samples, 2 of 32) and runs of one point's samples (100 > 64: two launches per point)
    for N, n, launches in ((3, len(p), -(-len(p) // 21)), (32, len(p), len(p) // 2), (100, 101, 202), (64, 37, 37), (65, 37, 74)):
        want, i0 = query(hs, p[:n], nf[:n], N, seed=3)
        got, i1 = query(small, p[:n], nf[:n], N, seed=3)
        assert_equal(got, want, "N %d in chunks of 64" % N)
        assert i0["launches"] == 1 and i1["launches"] == launches, (N, i0, i1)
        assert n < len(p) or (want > 0).any()
    # the steady state: a second call of the same size allocates nothing; neither does a smaller one
    _, a = query(hs, p, nf, 32, seed=3)
    _, b = query(hs, p, nf, 32, seed=3)
    _, c = query(hs, p[:100], nf[:100], 4, seed=3)
    assert b["grew"] == 0 and c["grew"] == 0 and b["staged_bytes"] == a["staged_bytes"] == c["staged_bytes"]
    fresh = hip.HipScene(sd, **kw)
    _, first = query(fresh, p, nf, 4)
    _, second = query(fresh, p, nf, 4)
    _, bigger = query(fresh, p, nf, 32)
    assert first["grew"] == 1 and second["grew"] == 0 and bigger["grew"] == 1 and bigger["staged_bytes"] > second["staged_bytes"]
    # n == 0 is a no-op; the ray queries still work on the shared staging
    z = pdc.Guarded((0, 3))
    _, info = hs.query_direct(DevBuf(shape=(0, 3)), DevBuf(shape=(0, 3)), 4, out=z)
    assert info["launches"] == 0
    o, d = hs.centre_rays(np.arange(64, dtype=np.uint32), camera=sd.camera)
    t, prim = hs.intersect(o, d)
    q = closest(hs, Rays(o, d), want=("t", "prim"))[0]
    assert np.array_equal(q["t"][prim >= 0], t[prim >= 0]) and np.array_equal(q["prim"], prim)
    for s in (hs, small, fresh):
        s.close()


def test_torch_tensors_on_a_side_stream():
    r = subprocess.run([sys.executable, os.path.join(HERE, "direct_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["on_side_stream"] and rec["outputs_are_torch"] and rec["nonzero"] > 20
    assert rec["differ"] == 0 and rec["again_differ"] == 0 and rec["grew_again"] == 0 and rec["non_contiguous_refused"]


# ---------------------------------------------------------------- 3. occlusion is exact
def test_occlusion_is_exact(pkg, hip):
    """The dark room of the two-room scene: light samples are live (the points face the lit room) and every one of them is stopped by the
    wall, so D is exactly 0.  Under a blocker D is 0 while the neighbour outside its shadow is lit."""
    sd = plit.two_rooms(pkg)
    hs = hip.HipScene(sd, builder="sah")
    rng = np.random.default_rng(9)
    P = np.stack([rng.uniform(2.1, 3.9, 200), rng.uniform(0.1, 1.9, 200), rng.uniform(0.1, 1.9, 200)], axis=1).astype(f32)
    NF = np.tile(np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0], [0, -1, 0]], f32), (40, 1))
    for N, seed, ks in COMBOS:
        D, _ = query(hs, P, NF, N, seed=seed, key_sample=ks)
        want, parts = dc.host_direct(hip, hs, P, NF, N, seed=seed, key_sample=ks)
        assert (parts["live"] != 0).mean() > 0.2 and not parts["visible"].any()
        assert_equal(D, want, "dark room")
        assert not D.view(np.uint32).any(), "light leaks into the dark room"
    # ... and in the lit room the same call sees the light
    lit, _ = query(hs, P - f32([2.05, 0, 0]), NF, 32)
    assert (lit > 0).any(axis=1).mean() > 0.15
    hs.close()
    sd = dc.one_triangle_scene(pkg, blocker=True)
    hs = hip.HipScene(sd, builder="sah")
    P, NF = np.array([dc.BLOCKED, dc.OPEN], f32), np.tile(f32([0, 1, 0]), (2, 1))
    for N in (4, 32):
        D, _ = query(hs, P, NF, N, seed=5)
        want, parts = dc.host_direct(hip, hs, P, NF, N, seed=5)
        assert parts["live"].all() and not parts["visible"][0].any() and parts["visible"][1].all()
        assert_equal(D, want, "blocker")
        assert not D[0].view(np.uint32).any() and (D[1] > 0).all()
    hs.close()


# ---------------------------------------------------------------- 4. against the closed form
def test_against_lamberts_formula(pkg, hip):
    """ONE emitting triangle above a floor, nothing between, 16 floor points, N = 4096: D against Lambert's polygon form-factor formula
    in float64, within 6 standard errors of each point's own mean (the errors from the host composition's per-sample contributions).
    tests/test_direct_cpu.py checks the same margin for the host composition with the oracle's sampleLight, without a GPU."""
    sd = dc.one_triangle_scene(pkg)
    hs = hip.HipScene(sd, builder="sah")
    p, nf = dc.floor_points()
    N = 4096
    D, info = query(hs, p, nf, N, seed=3)
    want, parts = dc.host_direct(hip, hs, p, nf, N, seed=3)
    assert_equal(D, want, "N 4096")
    assert parts["live"].all() and parts["visible"].all()  # nothing between
    dev, formula, se = dc.closed_form_check(D, parts, p, nf, N)
    print("\n[direct] device against Lambert's formula, 16 points x 4096 samples: largest deviation %.3g standard errors (relative standard "
          "error at most %.3g)" % (dev.max(), (se / formula).max()))
    assert (dev <= 6).all(), dev.max()
    hs.close()


# ---------------------------------------------------------------- 5. indirect-only probes
def masked_want(hs, sd, p, spp, seed, sample_offset=0, spp_total=None, start=None):
    """(sh, radiance, values, mask) expected of an indirect-only call: the fold of tests/test_gpu_probes.py with the value of every sample
    whose first ray has its closest hit on an emitting primitive replaced by 0."""
    o, d = pc.probe_pairs(hs, p, spp, seed, sample_offset)
    v = cast_values(hs, o, d, spp, sample_offset=sample_offset, seed=seed)
    t, prim = hs.intersect(o.reshape(-1, 3), d.reshape(-1, 3))
    em = emits(sd.materials)[plc.prim_materials(sd)[np.where(prim >= 0, prim, 0)]] & (prim >= 0)
    mask = em.reshape(len(p), spp)
    v = np.where(mask[..., None], f32(0), v).astype(f32)
    return (pc.sh_fold(v, d, spp_total, None if start is None else start[0]), fold(v, spp_total, None if start is None else start[1]), v, mask,
            (prim >= 0).reshape(len(p), spp))


def probe_points(hs, sd):
    """The 18 points of a 3 x 2 x 3 grid and 5 loose points, one of them 0.05 below the light."""
    grid = plc.scene_grid(sd)
    row = hs.sample_light(np.full((1, 4), 0.5, f32))[0]
    under = row[0:3] + row[3:6] * f32(0.05)
    loose = np.concatenate([pc.probe_points(sd, 4, seed=7), under[None]]).astype(f32)
    return grid, np.concatenate([pc.grid_points(*grid), loose]).astype(f32)


@pytest.mark.parametrize("kw", [dict(spp=64, seed=9), dict(spp=5, spp_per_pass=2, pool_paths=3 * 1024, seed=9)], ids=["spp64", "two_passes"])
def test_indirect_only_probes_equal_the_masked_fold(pkg, hip, kw):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah")
    grid, p = probe_points(hs, sd)
    w_sh, w_rad, v, mask, hits = masked_want(hs, sd, p, kw["spp"], kw["seed"])
    print("\n[direct] indirect-only probes, spp %d: %d of %d samples masked, %d probes with masked samples, the probe under the light %d of %d"
          % (kw["spp"], int(mask.sum()), mask.size, int(mask.any(axis=1).sum()), int(mask[-1].sum()), kw["spp"]))
    assert mask.any(axis=1).any() and (hits & ~mask).any(axis=1).any() and mask[-1].any()  # the condition: both kinds of sample are there
    sh, rad, var, _ = pc.probes(hs, p, variance=True, indirect_only=True, **kw)
    assert_equal(sh, w_sh, "sh")
    assert_equal(rad, w_rad, "radiance")
    want_var = variance_f64(v)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(var.astype(f64) - want_var) <= np.spacing(np.abs(want_var.astype(f32)))) | (np.isnan(var) & np.isnan(want_var))
    assert ok.all(), "variance"
    # the plain call differs exactly where a sample was masked, and opts null / zeroed is the plain call
    full_sh, full_rad, _, _ = pc.probes(hs, p, **kw)
    assert ((full_sh != sh).any(axis=1) == mask.any(axis=1)).all() and (full_rad[mask.any(axis=1)] > rad[mask.any(axis=1)]).any()
    off_sh, off_rad, _, _ = pc.probes(hs, p, indirect_only=False, **kw)
    assert_equal(off_sh, full_sh, "indirect_only False")
    assert_equal(off_rad, full_rad, "indirect_only False")
    out = pc.probe_outputs(len(p))
    outs = hip.ProbeOutputs(out["sh"].ptr, out["radiance"].ptr, None, None)
    prm, st, dp = hs.params(**kw), hip.Stats(), upload(p)
    for o in (None, C.byref(hip.ProbeOpts())):
        assert hip.lib().mcpt_query_probes_ex(hs.h, C.byref(prm), len(p), dp.ptr, C.byref(outs), None, C.byref(st), o) == 0
        assert_equal(out["sh"].get(), full_sh, "opts null or zeroed")
        assert_equal(out["radiance"].get(), full_rad, "opts null or zeroed")
    hs.close()


def test_indirect_only_composes_bakes_and_keeps_the_sky(pkg, hip):
    sd = pkg.scenes.cornell_demo(64, 64, 4)
    hs = hip.HipScene(sd, builder="sah")
    grid, p = probe_points(hs, sd)
    n = len(p)
    # a + b == a then b
    one_sh, one_rad, _, _ = pc.probes(hs, p, spp=5, seed=9, indirect_only=True)
    out = pc.probe_outputs(n)
    pc.probes(hs, p, out=out, spp=3, spp_total=5, seed=9, indirect_only=True)
    two_sh, two_rad, _, _ = pc.probes(hs, p, out=out, spp=2, sample_offset=3, spp_total=5, accumulate=1, seed=9, indirect_only=True)
    assert_equal(two_sh, one_sh, "3 + 2 samples, sh")
    assert_equal(two_rad, one_rad, "3 + 2 samples, radiance")
    assert_equal(one_sh, masked_want(hs, sd, p, 5, 9)[0], "spp 5")
    # the bakes equal their pieces
    m = 18
    kw = dict(spp=8, seed=11)
    pieces, _, _, _ = pc.probes(hs, pc.grid_points(*grid), radiance=False, indirect_only=True, **kw)
    full, _, _, _ = pc.probes(hs, pc.grid_points(*grid), radiance=False, **kw)
    assert (pieces != full).any()
    g = pdc.Guarded((m, 27))
    _, st = hs.bake_probe_grid(*grid, out=g, indirect_only=True, **kw)
    assert st.samples == m * 8
    assert_equal(g.get(), pieces, "bake_probe_grid_ex")
    md = float(f32(0.3 * scene_extent(sd)))
    vol = {"sh": pdc.Guarded((m, 27)), **pdc.depth_outputs(m)}
    hs.bake_probe_volume(*grid, 64, md, depth_seed=3, out=vol, indirect_only=True, **kw)
    assert_equal(vol["sh"].get(), pieces, "bake_probe_volume_ex, sh")
    w_m, w_c, _ = pdc.depth(hs, pc.grid_points(*grid), 64, md, seed=3)
    assert_equal(vol["moments"].get(), w_m, "bake_probe_volume_ex, moments (unchanged)")
    assert np.array_equal(vol["counts"].get(), w_c)
    plain = {"sh": pdc.Guarded((m, 27)), **pdc.depth_outputs(m)}
    hs.bake_probe_volume(*grid, 64, md, depth_seed=3, out=plain, **kw)
    assert_equal(plain["sh"].get(), full, "bake_probe_volume, sh")
    hs.close()
    # an environment map: a miss keeps the sky
    esd = plit.make_scene(pkg, "env")[0]
    hs = hip.HipScene(esd, builder="sah")
    _, p = probe_points(hs, esd)
    w_sh, w_rad, v, mask, hits = masked_want(hs, esd, p, 16, 4)
    assert (~hits).any() and (v[~hits] > 0).any() and mask.any()
    sh, rad, _, _ = pc.probes(hs, p, spp=16, seed=4, indirect_only=True)
    assert_equal(sh, w_sh, "environment map, sh")
    assert_equal(rad, w_rad, "environment map, radiance")
    hs.close()


# ---------------------------------------------------------------- 6. lit frames
@pytest.fixture(scope="module")
def cases(pkg, hip):
    made = {}

    def get(name):
        if name not in made:
            made[name] = plit.Case(pkg, hip, name)
        return made[name]

    yield get
    for c in made.values():
        c.hs.close()


def restate_direct(hs, hip, sd, vol, visible, cam, N, dseed, centre=True, spp=1, seed=1, aov=None):
    """plc.restate_depth0 with the direct term: the surface samples get a * (max(E, 0) + D), D = query_direct at the samples' own points
    and facing normals with key_sample k (point i of call k is sample k of pixel i).  Also returns the surface samples' count."""
    Wc, Hc = int(cam["width"]), int(cam["height"])
    n_px = Wc * Hc
    o, d = plc.frame_rays(hs, cam, centre, spp, seed)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(hit[:, None], o + d * t.astype(f32)[:, None], f32(0)).astype(f32)
    mi = plc.prim_materials(sd)[np.where(hit, prim, 0)]
    emitter = hit & emits(sd.materials)[mi]
    kind = np.where(hit, np.where(emitter, plc.EMITTER, plc.SURFACE), plc.MISS)
    if aov is not None:
        a = aov.reshape(n_px, 8)
        alb, nf = a[:, 0:3].astype(f32), a[:, 3:6].astype(f32)
    else:
        M = sd.materials[mi]
        assert not M["textured"][kind == plc.SURFACE].any()
        conductor = (M["type"] == 0) | (M["type"] == 1)
        alb = np.where(conductor[:, None], M["base_reflectance"], f32(1)).astype(f32)
        ng = closest(hs, Rays(o, d), want=("normal",))[0]["normal"]
        nf = np.where((plc.dot3(ng, d) > 0)[:, None], -ng, ng).astype(f32)
    D = np.zeros((n_px, spp, 3), f32)
    pk, nk = p.reshape(n_px, spp, 3), nf.reshape(n_px, spp, 3)
    for k in range(spp):
        D[:, k], _ = query(hs, pk[:, k], nk[:, k], N, seed=dseed, key_sample=k)
    D = D.reshape(-1, 3)
    v = np.zeros((len(o), 3), f32)
    s = kind == plc.SURFACE
    E = vol.lookup(hip, p[s], nf[s], visible)
    v[s] = alb[s] * (np.fmax(E, f32(0)) + D[s])
    other = np.flatnonzero(~s)
    if len(other):
        v[other] = cast_values(hs, o[other], d[other], 1, seed=1)[:, 0, :]
    lit, pos = plc.fold(v, p, kind, n_px, spp)
    return dict(lit=lit.reshape(Hc, Wc, 3), position=pos.reshape(Hc, Wc, 3), lookups=int(s.sum()), kind=kind.reshape(Hc, Wc, spp), D=D, s=s, p=p, nf=nf)


def live_samples(hip, hs, w, N, dseed, spp):
    """The live light samples of a restated frame, from the host composition with the frame's keys (m, k)."""
    idx = np.flatnonzero(w["s"])
    _, parts = dc.host_direct(hip, hs, w["p"][idx], w["nf"][idx], N, seed=dseed, pixels=idx // spp, key_samples=idx % spp)
    return int((parts["live"] != 0).sum())


def test_null_or_zero_direct_is_the_plain_frame(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    cam = np.ascontiguousarray(c.cam)
    g = hip.ProbeGrid((C.c_float * 3)(*c.grid[0]), (C.c_float * 3)(*c.grid[1]), (C.c_int32 * 3)(*c.grid[2]), (C.c_int32 * 3)(0, 0, 0))
    v = hip.ProbeVisibility(c.vol.nb, c.vol.bm, (C.c_int32 * 2)(0, 0))
    Dv = c.vol.dev
    pv = hip.ProbeVolume(C.pointer(g), Dv["sh"].ptr, Dv["moments"].ptr, Dv["counts"].ptr, C.pointer(v))
    for o in (hip.LitOpts(1, 0, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0)), hip.LitOpts(SPPJ, 2, 0, 7, (C.c_int32 * 4)(0, 0, 0, 0))):
        frames, infos = [], []
        for d in ("plain", None, hip.LitDirectOpts(0, 99, (C.c_int32 * 6)(0, 0, 0, 0, 0, 0))):
            lit, pos = pdc.Guarded((H, W, 3)), pdc.Guarded((H, W, 3))
            po = hip.LitOutputs(lit.ptr, pos.ptr, (C.c_void_p * 2)(None, None))
            info, di = hip.LitInfo(), hip.LitDirectInfo(7, 7, 7)
            if d == "plain":
                rc = L.mcpt_render_probe_lit(hs.h, cam.ctypes.data_as(C.c_void_p), C.byref(o), C.byref(pv), C.byref(po), None, C.byref(info))
            else:
                rc = L.mcpt_render_probe_lit_direct(hs.h, cam.ctypes.data_as(C.c_void_p), C.byref(o), None if d is None else C.byref(d), C.byref(pv),
                                                    C.byref(po), None, C.byref(info), C.byref(di))
                assert (di.light_samples, di.shadow_rays, di.pieces) == (0, 0, 0)
            assert rc == 0
            frames.append((lit.get(), pos.get()))
            infos.append((info.chunks, info.in_workspace, info.samples, info.lookups))
        for f, i in zip(frames[1:], infos[1:]):
            assert_equal(f[0], frames[0][0], "lit")
            assert_equal(f[1], frames[0][1], "position")
            assert i == infos[0]


@pytest.mark.parametrize("visible", [True, False], ids=["visible", "plain"])
@pytest.mark.parametrize("name", ["sah", "lbvh", "ploc", "chess", "chain"])
def test_centre_frame_with_direct_light(hip, cases, name, visible):
    c = cases(name)
    N, dseed = 4, 11
    aov = c.want(hip, visible)["aov"]
    w = restate_direct(c.hs, hip, c.sd, c.vol, visible, c.cam, N, dseed, aov=aov)
    lit, pos, info = plc.lit_frame(c.hs, c.vol, visible, centre=True, camera=c.cam, direct_samples=N, direct_seed=dseed)
    plain = c.want(hip, visible)
    assert_equal(lit, w["lit"], "%s: lit" % name)
    assert_equal(pos, plain["position"], "%s: position" % name)
    s = w["s"].reshape(lit.shape[:2])
    assert_equal(lit[~s], plain["lit"][~s], "%s: sky and emitter pixels" % name)
    gained = (lit[s] > plain["lit"][s]).any(axis=1).mean()
    print("\n[direct lit] %s, %s: %d surface pixels, %.0f %% of them gained direct light; %d light samples, %d shadow rays, %d piece(s), %.3g ms"
          % (name, "visible" if visible else "plain", int(s.sum()), 100 * gained, info["light_samples"], info["shadow_rays"], info["pieces"], info["ms_total"]))
    lights = c.hs.info()["n_lights"]
    assert (gained > 0.1 if lights else gained == 0) and (lit[s] >= plain["lit"][s]).all()  # (the chain scene has no emitter: D == 0 there)
    assert (info["shadow_rays"] > 0) == (lights > 0)
    assert info["samples"] == lit.shape[0] * lit.shape[1] and info["lookups"] == plain["lookups"] == int(s.sum())
    assert info["light_samples"] == info["lookups"] * N and (info["pieces"] >= 1 if lights else info["pieces"] == 0)
    assert info["shadow_rays"] == live_samples(hip, c.hs, w, N, dseed, 1)
    if name == "sah" and visible:  # the direct seed is read, also with centre rays; the frame's seed is not
        other, _, _ = plc.lit_frame(c.hs, c.vol, visible, centre=True, camera=c.cam, direct_samples=N, direct_seed=dseed + 1, position=False)
        assert (other != lit).any()
        same, _, _ = plc.lit_frame(c.hs, c.vol, visible, centre=True, camera=c.cam, direct_samples=N, direct_seed=dseed, seed=5, position=False)
        assert_equal(same, lit, "centre: the frame's seed is ignored")


@pytest.mark.parametrize("visible", [True, False], ids=["visible", "plain"])
def test_jittered_frame_with_direct_light(hip, cases, visible):
    c = cases("rc")
    N, dseed = 3, 6
    w = restate_direct(c.hs, hip, c.sd, c.vol, visible, c.cam, N, dseed, centre=False, spp=SPPJ, seed=7)
    lit, pos, info = plc.lit_frame(c.hs, c.vol, visible, aov_spp=SPPJ, seed=7, camera=c.cam, direct_samples=N, direct_seed=dseed)
    assert_equal(lit, w["lit"], "jittered lit")
    assert_equal(pos, w["position"], "jittered position")
    assert info["samples"] == WJ * HJ * SPPJ and info["lookups"] == w["lookups"] and info["light_samples"] == w["lookups"] * N
    assert info["shadow_rays"] == live_samples(hip, c.hs, w, N, dseed, SPPJ)
    plain, _, _ = plc.lit_frame(c.hs, c.vol, visible, aov_spp=SPPJ, seed=7, camera=c.cam, position=False)
    assert (lit != plain).any(axis=2).mean() > 0.1


@pytest.mark.parametrize("depth", [1, 2])
def test_chains_with_direct_light(hip, cases, depth):
    """At the end of a mirror chain the term is applied like the lookup: terminal surfaces are albedo x (max(E, 0) + D) of the frame's own
    position output with the chain AOV's albedo (throughput inside) and normal; misses and emitters are the plain frame's."""
    c = cases("mirrors")
    N, dseed, vis = 4, 3, True
    aov = c.hs.render_aovs(centre=True, camera=c.cam, specular_depth=depth).reshape(-1, 8)
    plain, ppos, pinfo = plc.lit_frame(c.hs, c.vol, vis, centre=True, camera=c.cam, specular_depth=depth)
    lit, pos, info = plc.lit_frame(c.hs, c.vol, vis, centre=True, camera=c.cam, specular_depth=depth, direct_samples=N, direct_seed=dseed)
    assert_equal(pos, ppos, "position")
    lit, pos, plain = lit.reshape(-1, 3), pos.reshape(-1, 3), plain.reshape(-1, 3)
    alb, nf = aov[:, 0:3].astype(f32), np.ascontiguousarray(aov[:, 3:6], f32)
    E = c.vol.lookup(hip, pos, nf, vis)
    D, _ = query(c.hs, pos, nf, N, seed=dseed, key_sample=0)
    want = alb * (np.fmax(E, f32(0)) + D)
    s = ~same_bits(lit, plain).all(axis=1)  # the pixels the direct term changed: terminal surfaces all of them
    deep0 = plc.lit_frame(c.hs, c.vol, vis, centre=True, camera=c.cam, specular_depth=0, direct_samples=N, direct_seed=dseed, position=False)[0].reshape(-1, 3)
    print("\n[direct lit] chains depth %d: %d pixels changed by the direct term, %d lookups, %d pixels differ from depth 0" % (
        depth, int(s.sum()), info["lookups"], int((~same_bits(lit, deep0).all(axis=1)).sum())))
    assert s.sum() > 0.3 * info["lookups"] and info["lookups"] == pinfo["lookups"]
    assert_equal(lit[s], want[s], "terminal surfaces")
    assert (~same_bits(lit, deep0).all(axis=1)).sum() > 20  # the mirrors are in view: the term was applied behind them
    assert info["light_samples"] == info["lookups"] * N


def test_own_buffers_pieces_and_the_steady_state(pkg, hip, cases):
    c, j = cases("sah"), cases("rc")
    N, dseed = 4, 11
    wc = restate_direct(c.hs, hip, c.sd, c.vol, True, c.cam, N, dseed, aov=c.want(hip, True)["aov"])
    wj = restate_direct(j.hs, hip, j.sd, j.vol, True, j.cam, N, dseed, centre=False, spp=SPPJ, seed=7)
    for case, w, kw, spp in ((c, wc, dict(centre=True), 1), (j, wj, dict(aov_spp=SPPJ, seed=7), SPPJ)):
        hs = hip.HipScene(case.sd, **case.kw)  # nothing has run on it: buffers of the call's own
        lit, pos, info = plc.lit_frame(hs, case.vol, True, camera=case.cam, direct_samples=N, direct_seed=dseed, **kw)
        assert info["in_workspace"] == 0
        assert_equal(lit, w["lit"], "a scene that has never rendered")
        assert_equal(pos, w["position"], "a scene that has never rendered, position")
        n_live = live_samples(hip, hs, w, N, dseed, spp)
        assert info["chunks"] == 1 and info["pieces"] >= N and info["shadow_rays"] == n_live  # one chunk of n rays stages n * N light samples n at a time
        hs.render(camera=case.cam, spp=1, seed=1, pool_paths=768)
        lit, pos, info = plc.lit_frame(hs, case.vol, True, camera=case.cam, direct_samples=N, direct_seed=dseed, **kw)
        assert info["in_workspace"] == 1 and info["pieces"] > info["chunks"] >= 1, info
        assert_equal(lit, w["lit"], "in the 768-path pool: %d chunks, %d pieces" % (info["chunks"], info["pieces"]))
        assert_equal(pos, w["position"], "in the 768-path pool, position")
        assert info["light_samples"] == w["lookups"] * N and info["shadow_rays"] == n_live
        before = hs.probe_buffers()
        o, d = hs.centre_rays(np.arange(64, dtype=np.uint32), camera=case.cam)
        closest(hs, Rays(o, d))
        lit2, _, info2 = plc.lit_frame(hs, case.vol, True, camera=case.cam, direct_samples=N, direct_seed=dseed, **kw)
        assert hs.probe_buffers() == before and closest(hs, Rays(o, d))[1]["grew"] == 0
        assert (info2["chunks"], info2["pieces"], info2["shadow_rays"]) == (info["chunks"], info["pieces"], info["shadow_rays"])
        assert_equal(lit2, lit, "second call")
        print("\n[direct lit] %s: %d chunk(s) and %d piece(s) in the 768-path pool, %d of %d light samples live" % (
            case.name, info["chunks"], info["pieces"], n_live, info["light_samples"]))
        hs.close()
    # no emitter: exact zeros, no shadow ray, the frame of the plain call
    dsd = without_emitters(c.sd)
    hs = hip.HipScene(dsd, **c.kw)
    lit, _, info = plc.lit_frame(hs, c.vol, True, camera=c.cam, centre=True, direct_samples=N, position=False)
    plain, _, _ = plc.lit_frame(hs, c.vol, True, camera=c.cam, centre=True, position=False)
    assert info["shadow_rays"] == 0 and info["light_samples"] == info["lookups"] * N and np.array_equal(lit, plain)
    hs.close()


def test_live_scene_with_direct_light(pkg, hip, cases):
    """After every kind of edit the frame of the live handle equals the frame of a fresh scene of the edited description, and the restated
    one; a dimmed light scales D, a light that no longer emits leaves none."""
    c = cases("sah")
    N, dseed = 4, 11
    sd, (objs, tris) = split(hip, c.sd, [PLASTIC_SPHERE])
    hs = hip.HipScene(sd, builder="sah")
    frames = []

    def check(fresh_sd, what, restate=True):
        fresh = hip.HipScene(fresh_sd, builder="sah")
        want, wpos, winfo = plc.lit_frame(fresh, c.vol, True, centre=True, camera=c.cam, direct_samples=N, direct_seed=dseed)
        lit, pos, info = plc.lit_frame(hs, c.vol, True, centre=True, camera=c.cam, direct_samples=N, direct_seed=dseed)
        assert_equal(lit, want, what)
        assert_equal(pos, wpos, what + ", position")
        assert (info["lookups"], info["shadow_rays"]) == (winfo["lookups"], winfo["shadow_rays"])
        if restate:
            w = restate_direct(fresh, hip, fresh_sd, c.vol, True, c.cam, N, dseed, aov=fresh.render_aovs(centre=True, camera=c.cam))
            assert_equal(lit, w["lit"], what + ", restated")
        fresh.close()
        frames.append((lit, info))
        if len(frames) > 1:
            assert (frames[-1][0] != frames[-2][0]).any(), what + ": the edit is not in the frame"

    check(sd, "as created")
    m = translate(40, 0, -30)
    hs.update([(SHORT, m)])
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    check(now, "update")
    P = wave(object_positions(sd, SHORT))
    hs.deform([(SHORT, P)])
    now = deformed_scene(pkg, hip, sd, {SHORT: P}, {SHORT: m})
    check(now, "deform", restate=False)
    with_box = frames[-1][0]
    hs.set_visibility([(SHORT, False)])
    csd, _ = hip.compact_scene(now, mask_hiding(now, [SHORT]))
    check(csd, "set_visibility")
    # the blocker is hidden: its shadow goes.  Seen from the demo camera, which looks down at the floor: the pixels that show the same point
    # in both frames only gain light.
    cam2 = pkg.scenes.cornell_demo(W, H, 4).camera
    hid, pos_a, _ = plc.lit_frame(hs, c.vol, True, centre=True, camera=cam2, direct_samples=N, direct_seed=dseed)
    hs.set_visibility([(SHORT, True)])
    shown, pos_b, _ = plc.lit_frame(hs, c.vol, True, centre=True, camera=cam2, direct_samples=N, direct_seed=dseed)
    both = same_bits(pos_a, pos_b).all(axis=2) & (pos_a != 0).any(axis=2)
    gone = (hid[both] > shown[both]).any(axis=1)
    print("\n[direct lit] hiding the short box: %d pixels show the same point in both frames, %d of them brighter without it" % (int(both.sum()), int(gone.sum())))
    assert both.sum() > 100 and gone.sum() > 3 and (hid[both] >= shown[both]).all()
    hs.add_objects(objs, tris if len(tris) else None)
    now = extend_numpy(now, objs, tris, [])
    check(now, "add_objects", restate=False)
    # the light dimmed to a quarter (a power of two: D scales exactly), then made non-emitting
    full, _ = frames[-1]
    li = int(now.objects["material"][LIGHT])
    e = np.asarray(now.materials[li]["emission"], f32)
    for scale, what in ((0.25, "dimmed"), (0.0, "dark")):
        edits = [(li, with_fields(now.materials[li], emission=tuple(float(x) for x in e * f32(scale))))]
        hs.set_materials(edits)
        check(edited_scene(now, edits), "set_materials, " + what, restate=(scale == 0.25))
    plain, _, _ = plc.lit_frame(hs, c.vol, True, centre=True, camera=c.cam, position=False)
    assert np.array_equal(frames[-1][0], plain) and frames[-1][1]["shadow_rays"] == 0  # no emitter: D == 0
    assert frames[-2][1]["shadow_rays"] == frames[-3][1]["shadow_rays"] > 0           # dimmed: the same rays
    hs.close()


def test_dimmed_light_scales_the_term(pkg, hip):
    sd = plit.make_scene(pkg, "sah")[0]
    hs = hip.HipScene(sd, builder="sah")
    p, nf, _ = frame_points(hs, sd.camera)
    full, _ = query(hs, p, nf, 4, seed=2)
    li = int(sd.objects["material"][LIGHT])
    e = np.asarray(sd.materials[li]["emission"], f32)
    hs.set_materials([(li, with_fields(sd.materials[li], emission=tuple(float(x) for x in e * f32(0.25))))])
    dim, _ = query(hs, p, nf, 4, seed=2)
    assert_equal(dim, full * f32(0.25), "a quarter of the emission: a quarter of D, exactly")
    assert (full > 0).any()
    hs.set_materials([(li, with_fields(sd.materials[li], emission=(0.0, 0.0, 0.0)))])
    dark, _ = query(hs, p, nf, 4, seed=2)
    assert hs.info()["n_lights"] == 0 and not dark.view(np.uint32).any()
    hs.close()


def test_a_direct_lit_call_leaves_the_scene_as_it_was(hip, cases):
    c = cases("sah")
    hs = hip.HipScene(c.sd, **c.kw)
    o, d = hs.centre_rays(np.arange(W * H, dtype=np.uint32), camera=c.cam)
    p, nf, _ = frame_points(hs, c.cam)

    def state():
        fb, _ = hs.render(camera=c.cam, spp=2, seed=5)
        aov = hs.render_aovs(aov_spp=2, seed=3, camera=c.cam, specular_depth=1)
        q = closest(hs, Rays(o, d), want=("t", "prim", "normal"))[0]
        return fb, aov, q

    fb0, aov0, q0 = state()
    for kw in (dict(centre=True), dict(aov_spp=SPPJ, seed=2, specular_depth=2)):
        plc.lit_frame(hs, c.vol, True, camera=c.cam, direct_samples=4, **kw)
        plc.lit_frame(hs, c.vol, False, camera=c.cam, direct_samples=32, **kw)
    query(hs, p, nf, 4)
    fb1, aov1, q1 = state()
    assert_equal(fb1, fb0, "render")
    assert_equal(aov1, aov0, "render_aovs")
    assert np.array_equal(q1["t"], q0["t"]) and np.array_equal(q1["prim"], q0["prim"])
    assert_equal(q1["normal"], q0["normal"], "query_closest")
    hs.close()


class IndirectVolume(plc.Volume):
    """plc.Volume baked with indirect_only."""

    def __init__(self, hs, grid, spp, depth_spp, max_distance, normal_bias=0.0, backface_max=0.25):
        self.grid, self.nb, self.bm = grid, normal_bias, backface_max
        m = grid[2][0] * grid[2][1] * grid[2][2]
        self.dev = {"sh": pdc.Guarded((m, 27)), **pdc.depth_outputs(m)}
        hs.bake_probe_volume(*grid, depth_spp, max_distance, depth_seed=3, out=self.dev, spp=spp, seed=2, indirect_only=True)
        self.sh, self.mom, self.cnt = self.dev["sh"].get(), self.dev["moments"].get(), self.dev["counts"].get()


def test_the_dark_room_gets_no_direct_light(pkg, hip):
    """The two rooms with an indirect-only volume: in the dark room D == 0 at every pixel, so the frame with N = 4 is the N = 0 frame of
    the same volume bit for bit; light samples were live and every shadow ray was stopped by the wall."""
    sd = plit.two_rooms(pkg)
    hs = hip.HipScene(sd, builder="sah")
    grid = ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (4, 2, 2))
    vol = IndirectVolume(hs, grid, 512, 512, 3.0, normal_bias=0.02)
    full = plc.Volume(hs, grid, 512, 512, 3.0, normal_bias=0.02)
    assert (vol.sh != full.sh).any() and np.array_equal(vol.mom, full.mom)  # the probes of the lit room saw the emitter
    for visible in (True, False):
        off, _, _ = plc.lit_frame(hs, vol, visible, centre=True)
        on, pos, info = plc.lit_frame(hs, vol, visible, centre=True, direct_samples=4, direct_seed=8)
        assert info["lookups"] == W * H and info["shadow_rays"] > 0.1 * info["light_samples"]
        assert_equal(on, off, "the dark room, %s" % ("visible" if visible else "plain"))
    # ... while a camera in the lit room gets the term
    cam = pkg.scenes.make_camera(W, H, 40, (1.5, 1.0, 1.0), (1.0, 0.0, 1.0))
    off, _, _ = plc.lit_frame(hs, vol, True, centre=True, camera=cam)
    on, _, _ = plc.lit_frame(hs, vol, True, centre=True, camera=cam, direct_samples=4, direct_seed=8)
    assert (on > off).any(axis=2).mean() > 0.5
    hs.close()


def test_refusals_on_a_live_handle(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    cam = np.ascontiguousarray(c.cam)
    pcam = cam.ctypes.data_as(C.c_void_p)
    host = np.zeros((H * W * 3 + 18 * 192,), f32)
    lit, pos = pdc.Guarded((H, W, 3)), pdc.Guarded((H, W, 3))
    g = hip.ProbeGrid((C.c_float * 3)(*c.grid[0]), (C.c_float * 3)(*c.grid[1]), (C.c_int32 * 3)(*c.grid[2]), (C.c_int32 * 3)(0, 0, 0))
    v = hip.ProbeVisibility(c.vol.nb, c.vol.bm, (C.c_int32 * 2)(0, 0))
    Dv = c.vol.dev
    info, di = hip.LitInfo(7, 7, 7, 7, 7.0), hip.LitDirectInfo(7, 7, 7)

    def call(d=None, sh=Dv["sh"].ptr, out_lit=lit.ptr, out_pos=pos.ptr):
        d = d or hip.LitDirectOpts(4, 1, (C.c_int32 * 6)(0, 0, 0, 0, 0, 0))
        o = hip.LitOpts(1, 0, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0))
        pv = hip.ProbeVolume(C.pointer(g), sh, Dv["moments"].ptr, Dv["counts"].ptr, C.pointer(v))
        po = hip.LitOutputs(out_lit, out_pos, (C.c_void_p * 2)(None, None))
        return L.mcpt_render_probe_lit_direct(hs.h, pcam, C.byref(o), C.byref(d), C.byref(pv), C.byref(po), None, C.byref(info), C.byref(di))

    for kw, word in ((dict(d=hip.LitDirectOpts(-1, 1, (C.c_int32 * 6)(0, 0, 0, 0, 0, 0))), b"n_samples"),
                     (dict(d=hip.LitDirectOpts(4097, 1, (C.c_int32 * 6)(0, 0, 0, 0, 0, 0))), b"n_samples"),
                     (dict(d=hip.LitDirectOpts(4, 1, (C.c_int32 * 6)(0, 0, 0, 0, 0, 1))), b"reserved"), (dict(sh=host.ctypes.data), b"device"),
                     (dict(out_lit=host.ctypes.data), b"device"), (dict(out_pos=host.ctypes.data), b"device"), (dict(out_lit=None), b"null")):
        rc = call(**kw)
        assert rc == 1 and b"mcpt_render_probe_lit_direct" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert info.samples == 7 and di.pieces == 7
    assert (lit.get() == f32(SENTINEL)).all() and (pos.get() == f32(SENTINEL)).all()  # nothing was written
    assert call() == 0 and info.samples == W * H and di.light_samples == info.lookups * 4
    # mcpt_query_direct: host memory, and the refusals that need no device, on a live handle
    p, nf, _ = frame_points(hs, c.cam)
    dp, dn, out = upload(p), upload(nf), pdc.Guarded((len(p), 3))
    qi = hip.QueryInfo(7, 7, 7)

    def q(o=None, n=len(p), pp=dp.ptr, pn=dn.ptr, po=out.ptr):
        o = o or hip.DirectOpts(1, 4, 0, (C.c_int32 * 5)(0, 0, 0, 0, 0))
        return L.mcpt_query_direct(hs.h, C.byref(o), n, pp, pn, po, None, C.byref(qi))

    hp = np.zeros((len(p), 3), f32)
    for kw, word in ((dict(pp=hp.ctypes.data), b"device"), (dict(pn=hp.ctypes.data), b"device"), (dict(po=hp.ctypes.data), b"device"),
                     (dict(o=hip.DirectOpts(1, 0, 0, (C.c_int32 * 5)(0, 0, 0, 0, 0))), b"n_samples"),
                     (dict(o=hip.DirectOpts(1, 4, 0, (C.c_int32 * 5)(0, 0, 3, 0, 0))), b"reserved"), (dict(n=-1), b"n must"), (dict(po=None), b"null")):
        assert q(**kw) == 1 and b"mcpt_query_direct" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, L.mcpt_last_error())
        assert (qi.launches, qi.grew) == (7, 7)
    assert (out.get() == f32(SENTINEL)).all() and not hp.any()
    assert q() == 0 and qi.launches == 1
    assert (out.get() != f32(SENTINEL)).all()
    # the probe options on a live handle
    prm, outs = hs.params(spp=4, seed=1), hip.ProbeOutputs(Dv["sh"].ptr, None, None, None)
    bad = hip.ProbeOpts(2, (C.c_int32 * 7)(0, 0, 0, 0, 0, 0, 0))
    pts = upload(pc.grid_points(*c.grid))
    assert L.mcpt_query_probes_ex(hs.h, C.byref(prm), 18, pts.ptr, C.byref(outs), None, None, C.byref(bad)) == 1 and b"indirect_only" in L.mcpt_last_error()
    assert np.array_equal(Dv["sh"].get(), c.vol.sh)  # untouched
