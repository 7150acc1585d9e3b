"""mcpt_probe_volume_relight on the GPU: one update of a probe volume from itself.

Expected volumes are the restatement of tests/probe_relight_cases.py, a composition of calls that exist without the feature (probe_rays,
intersect, the material table with query_closest's normal, the host forms of the two grid lookups, the host composition of the direct
term, cast_rays for the sky and the emitters, the fold and the blend in numpy float32).  Device bits are compared with it.  Scenes are the
Cornell box with a 3 x 2 x 3 grid; the previous volume is baked at 64 spp with 64 depth samples.  Device buffers are made without torch
and every output sits between two runs of 64 guard elements that must survive.  torch and a non-default stream:
tests/probe_relight_torch_child.py, a child process."""
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
import probe_lit_cases as plc  # noqa: E402
import probe_relight_cases as prc  # noqa: E402
from add_cases import extend_numpy, split  # noqa: E402
from deform_cases import PLASTIC_SPHERE, SHORT, deformed_scene, translate  # noqa: E402
from material_edit_cases import LEFT, edited_scene, with_fields  # noqa: E402
from ray_query_cases import DevBuf  # noqa: E402
from sensor_query_cases import SENTINEL, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
PROBES = 18


def assert_equal(got, want, what=""):
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: got %r, want %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], np.asarray(got)[bad][0], np.asarray(want)[bad][0])


class Case:
    def __init__(self, pkg, hip, name):
        self.name = name
        self.sd, self.kw, self.grid, self.md = prc.make_scene(pkg, name)
        self.hs = hip.HipScene(self.sd, **self.kw)
        self.vol = plc.Volume(self.hs, self.grid, 64, 64, self.md, normal_bias=float(f32(0.01 * self.md)))


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


# ---------------------------------------------------------------- 1. one update equals the restatement
# (scene, occlusion-aware lookup, spp, direct_samples, indirect_only, hysteresis, sample_offset)
UPDATES = [("sah", True, 64, 0, 0, 0.0, 0), ("sah", False, 64, 0, 0, 0.0, 0), ("lbvh", True, 64, 0, 0, 0.0, 0), ("lbvh", False, 64, 3, 1, 0.75, 0),
           ("ploc", True, 64, 3, 1, 0.75, 0), ("ploc", False, 64, 0, 0, 0.0, 0), ("env", True, 64, 0, 0, 0.0, 0), ("env", False, 64, 3, 1, 0.75, 5),
           ("dim", True, 64, 0, 0, 0.0, 0), ("dim", False, 65, 3, 0, 0.75, 5), ("sah", True, 1, 0, 0, 0.75, 0), ("sah", False, 1, 3, 1, 0.0, 7),
           ("sah", True, 65, 3, 1, 0.75, 7), ("sah", False, 65, 0, 1, 0.0, 0), ("sah", True, 64, 3, 0, 0.0, 0), ("sah", False, 64, 0, 0, 0.75, 3)]


@pytest.mark.parametrize("name,visible,spp,direct,indirect_only,h,offset", UPDATES,
                         ids=["%s-%s-spp%d-d%d-io%d-h%g-o%d" % (u[0], "visible" if u[1] else "plain", *u[2:]) for u in UPDATES])
def test_one_update_equals_the_restatement(hip, cases, name, visible, spp, direct, indirect_only, h, offset):
    c = cases(name)
    kw = dict(spp=spp, seed=5, sample_offset=offset, indirect_only=bool(indirect_only), direct_samples=direct, direct_seed=9)
    want, smp = prc.restate(c.hs, hip, c.sd, c.vol, visible, hysteresis=h, **kw)
    sh, mom, cnt, info = prc.relight(c.hs, c.vol, visible, hysteresis=h, **kw)
    kind = smp["kind"]
    n_s, n_e, n_m = (int((kind == k).sum()) for k in (plc.SURFACE, plc.EMITTER, plc.MISS))
    print("\n[probe relight] %s, %s, spp %d, direct %d, indirect_only %d, h %g: %d surface, %d emitter, %d sky samples; %d launch(es), staged %d KiB"
          % (name, "visible" if visible else "plain", spp, direct, indirect_only, h, n_s, n_e, n_m, info["launches"], info["staged_bytes"] >> 10))
    assert mom is None and cnt is None and sh.shape == (PROBES, 27)
    assert n_s + n_e + n_m == PROBES * spp and n_s > 0.5 * kind.size
    if name == "env":
        assert n_m > 0  # the sky through the opening
    assert np.isfinite(want).all() and (want != 0).any()
    assert_equal(sh, want, "%s: sh" % name)
    if name == "dim" and not indirect_only:  # below the clamp: emission x |cos| is in the samples
        em = smp["v"][kind == plc.EMITTER]
        assert len(em) == 0 or ((em > 0).all() and (em < f32(prc.DIM)).all())


def test_the_switches_are_read(hip, cases):
    """The premise of the parametrisation: on the Cornell scene the lookup, the direct term, the emitter switch, the hysteresis, the seed
    and the sample offset each change the result."""
    c = cases("sah")
    base = dict(spp=64, seed=5)
    ref = prc.relight(c.hs, c.vol, True, **base)[0]
    for what, vis, kw in (("the lookup", False, {}), ("direct_samples", True, dict(direct_samples=3)), ("hysteresis", True, dict(hysteresis=0.75)),
                          ("seed", True, dict(seed=6)), ("sample_offset", True, dict(sample_offset=1)), ("indirect_only", True, dict(indirect_only=True))):
        other = prc.relight(c.hs, c.vol, vis, **dict(base, **kw))[0]
        assert (other != ref).any(), what
    a = prc.relight(c.hs, c.vol, True, spp=64, seed=5, direct_samples=3, direct_seed=1)[0]
    b = prc.relight(c.hs, c.vol, True, spp=64, seed=5, direct_samples=3, direct_seed=2)[0]
    assert (a != b).any(), "direct_seed"


# ---------------------------------------------------------------- 2. depth outputs
@pytest.mark.parametrize("spp", [64, 70])
def test_depth_outputs_equal_the_depth_query(hip, cases, spp):
    c = cases("sah")
    kw = dict(spp=spp, seed=11, sample_offset=2, direct_samples=3, hysteresis=0.75)
    sh0 = prc.relight(c.hs, c.vol, True, **kw)[0]
    sh, mom, cnt, info = prc.relight(c.hs, c.vol, True, depth=True, max_distance=c.md, **kw)
    want_m, want_c, _ = pdc.depth(c.hs, pc.grid_points(*c.grid), spp, c.md, seed=11, sample_offset=2)
    assert_equal(mom, want_m, "moments")
    assert np.array_equal(cnt, want_c) and (cnt[:, 0] == spp).all()
    assert_equal(sh, sh0, "sh with depth outputs")


# ---------------------------------------------------------------- 3. the cut
def test_the_result_does_not_depend_on_the_cut(hip, cases, monkeypatch):
    """A staging of 64: a probe's 130 samples take three pieces (64, 64, 2), whose partial sums pass through the output, and the 3 light
    samples of a piece's 64 records take four."""
    c = cases("sah")
    kw = dict(spp=130, seed=3, direct_samples=3, direct_seed=4, hysteresis=0.75, indirect_only=True, depth=True, max_distance=c.md)
    sh, mom, cnt, info = prc.relight(c.hs, c.vol, True, **kw)
    monkeypatch.setenv("MCPT_QUERY_CHUNK", "64")
    hs = hip.HipScene(c.sd, **c.kw)
    monkeypatch.delenv("MCPT_QUERY_CHUNK")
    for visible in (True, False):
        want = (sh, mom, cnt) if visible else prc.relight(c.hs, c.vol, False, **kw)[:3]
        sh2, mom2, cnt2, info2 = prc.relight(hs, c.vol, visible, **kw)
        assert_equal(sh2, want[0], "sh at a staging of 64")
        assert_equal(mom2, want[1], "moments at a staging of 64")
        assert np.array_equal(cnt2, want[2])
    print("\n[probe relight] spp 130 x 3 light samples: %d launch(es) by default, %d at a staging of 64" % (info["launches"], info2["launches"]))
    assert info2["launches"] >= PROBES * 3 * 2 and info2["launches"] > info["launches"]
    hs.close()


# ---------------------------------------------------------------- 4. the inputs, the steady state, determinism
def test_inputs_unchanged_steady_state_and_determinism(hip, cases):
    c = cases("sah")
    hs = hip.HipScene(c.sd, **c.kw)
    kw = dict(spp=65, seed=2, direct_samples=3, hysteresis=0.5, depth=True, max_distance=c.md)
    sh, mom, cnt, info = prc.relight(hs, c.vol, True, **kw)
    assert info["grew"] == 1  # the scene's first such call
    before = hs.probe_buffers()
    assert before[0] > 0
    sh2, mom2, cnt2, info2 = prc.relight(hs, c.vol, True, **kw)
    assert info2["grew"] == 0 and hs.probe_buffers() == before and info2["launches"] == info["launches"]
    assert_equal(sh2, sh, "second call: sh")
    assert_equal(mom2, mom, "second call: moments")
    assert np.array_equal(cnt2, cnt)
    # a smaller call fits what the scene owns
    assert prc.relight(hs, c.vol, False, spp=8, direct_samples=2)[3]["grew"] == 0 and hs.probe_buffers() == before
    # the previous volume was read only
    assert_equal(c.vol.dev["sh"].get(), c.vol.sh, "volume->sh")
    assert_equal(c.vol.dev["moments"].get(), c.vol.mom, "volume->moments")
    assert np.array_equal(c.vol.dev["counts"].get(), c.vol.cnt)
    # ... and the other scene, which has its own buffers, gives the same bits
    assert_equal(prc.relight(c.hs, c.vol, True, **kw)[0], sh, "another scene of the same description")
    hs.close()


# ---------------------------------------------------------------- 5. the live scene
def test_live_scene(pkg, hip, cases):
    """Baked once; after an update (the short box moves), a material edit (a wall is recoloured) and an addition, an update from the OLD
    volume equals the restatement made on a scene freshly created from the edited description."""
    c = cases("sah")
    sd, (objs, tris) = split(hip, c.sd, [PLASTIC_SPHERE])
    hs = hip.HipScene(sd, builder="sah")
    kw = dict(spp=64, seed=4, direct_samples=3, direct_seed=2, hysteresis=0.75, indirect_only=True)
    results = []

    def check(fresh_sd, what):
        fresh = hip.HipScene(fresh_sd, builder="sah")
        for visible in (True, False):
            want, _ = prc.restate(fresh, hip, fresh_sd, c.vol, visible, **kw)
            got = prc.relight(hs, c.vol, visible, **kw)[0]
            assert_equal(got, want, "%s, %s" % (what, "visible" if visible else "plain"))
        fresh.close()
        results.append(got)
        if len(results) > 1:
            assert (results[-1] != results[-2]).any(), what + ": the edit is not in the volume"

    check(sd, "as created")
    m = translate(40, 0, -30)
    hs.update([(SHORT, m)])
    now = deformed_scene(pkg, hip, sd, {}, {SHORT: m})
    check(now, "update")
    left = int(now.objects["material"][LEFT])
    edits = [(left, with_fields(now.materials[left], base_reflectance=(0.2, 0.3, 0.9)))]
    hs.set_materials(edits)
    now = edited_scene(now, edits)
    check(now, "set_materials")
    hs.add_objects(objs, tris if len(tris) else None)
    now = extend_numpy(now, objs, tris, [])
    check(now, "add_objects")
    hs.close()


# ---------------------------------------------------------------- 6. the link to the path tracer
def test_no_light_gives_exactly_zero(hip, cases):
    """No emitter and a black background: the path tracer's frame is 0, an update from a zero volume is exactly 0 (with the direct term
    asked for as well), and so is a frame lit by it on every surface pixel."""
    c = cases("dark")
    assert c.hs.info()["n_lights"] == 0
    fb, _ = c.hs.render(spp=2, seed=3)
    assert (fb == 0).all(), "the scene of this test is not dark"
    zero = prc.HostVolume(c.grid, np.zeros((PROBES, 27), f32), c.vol.mom, c.vol.cnt, c.vol.nb, c.vol.bm)
    for visible in (True, False):
        for kw in (dict(), dict(direct_samples=3), dict(hysteresis=0.75, direct_samples=3, indirect_only=True)):
            sh = prc.relight(c.hs, zero, visible, spp=64, seed=2, **kw)[0]
            assert not sh.view(np.uint32).any(), "not exactly +0"
        relit = prc.HostVolume(c.grid, sh, c.vol.mom, c.vol.cnt, c.vol.nb, c.vol.bm)
        lit, _, info = plc.lit_frame(c.hs, relit, visible, position=False, centre=True)
        assert info["lookups"] > 0.5 * lit.shape[0] * lit.shape[1] and not lit.view(np.uint32).any()


# ---------------------------------------------------------------- 7. the output is a volume every consumer accepts
@pytest.mark.parametrize("visible", [True, False], ids=["visible", "plain"])
def test_a_frame_lit_from_the_relit_volume(hip, cases, visible):
    """Two updates chained on the device (the second reads the first's output buffer), then frames from the relit buffers: the plain
    frame equals restate_depth0 fed the relit host copy; the frame with sampled direct light equals the one from an upload of that copy."""
    c = cases("sah")
    kw = dict(spp=64, direct_samples=2, indirect_only=True, hysteresis=0.5, depth=True, max_distance=c.md)
    out1, out2 = prc.outputs(PROBES, True), prc.outputs(PROBES, True)
    sh1, mom1, cnt1, _ = prc.relight(c.hs, c.vol, visible, out=out1, seed=21, **kw)
    first = prc.HostVolume(c.grid, sh1, mom1, cnt1, c.vol.nb, c.vol.bm)
    first.dev = out1  # the device buffers the first update wrote
    sh2, mom2, cnt2, _ = prc.relight(c.hs, first, visible, out=out2, seed=22, **kw)
    want2, _ = prc.restate(c.hs, hip, c.sd, first, visible, spp=64, seed=22, direct_samples=2, indirect_only=True, hysteresis=0.5)
    assert_equal(sh2, want2, "the second update")
    relit = prc.HostVolume(c.grid, sh2, mom2, cnt2, c.vol.nb, c.vol.bm)
    uploaded_dev = relit.dev
    cam = c.sd.camera
    aov = c.hs.render_aovs(centre=True, camera=cam)
    want = plc.restate_depth0(c.hs, hip, c.sd, relit, visible, cam, aov=aov)
    relit.dev = out2
    lit, pos, info = plc.lit_frame(c.hs, relit, visible, centre=True, camera=cam)
    assert_equal(lit, want["lit"], "lit from the relit volume")
    assert_equal(pos, want["position"], "position")
    assert info["lookups"] == want["lookups"] and (lit > 0).any()
    direct, _, _ = plc.lit_frame(c.hs, relit, visible, centre=True, camera=cam, position=False, direct_samples=3, direct_seed=5)
    relit.dev = uploaded_dev
    direct_up, _, _ = plc.lit_frame(c.hs, relit, visible, centre=True, camera=cam, position=False, direct_samples=3, direct_seed=5)
    assert_equal(direct, direct_up, "lit with direct light")
    assert (direct != lit).any()


# ---------------------------------------------------------------- 8. refusals on a live handle; torch
def test_refusals_on_a_live_handle(hip, cases):
    c = cases("sah")
    hs, L = c.hs, hip.lib()
    host = np.zeros((PROBES * 192,), f32)
    out = prc.outputs(PROBES, True)
    g = hip.ProbeGrid((C.c_float * 3)(*c.grid[0]), (C.c_float * 3)(*c.grid[1]), (C.c_int32 * 3)(*c.grid[2]), (C.c_int32 * 3)(0, 0, 0))
    v = hip.ProbeVisibility(c.vol.nb, c.vol.bm, (C.c_int32 * 2)(0, 0))
    D = c.vol.dev
    info = hip.QueryInfo(7, 7, 7, (C.c_int32 * 4)(7, 7, 7, 7))

    def opts(spp=4, h=0.5, md=1.0, direct=0):
        return hip.ProbeRelightOpts(1, spp, 0, h, 0, direct, 1, md, (C.c_int32 * 8)(*([0] * 8)))

    def call(o=None, sh=D["sh"].ptr, mom=D["moments"].ptr, cnt=D["counts"].ptr, vis=v, out_sh=out["sh"].ptr, out_mom=out["moments"].ptr,
             out_cnt=out["counts"].ptr):
        pv = hip.ProbeVolume(C.pointer(g), sh, mom, cnt, C.pointer(vis) if vis is not None else None)
        po = hip.ProbeRelightOutputs(out_sh, out_mom, out_cnt, None)
        return L.mcpt_probe_volume_relight(hs.h, C.byref(pv), C.byref(o or opts()), C.byref(po), None, C.byref(info))

    for kw, word in ((dict(sh=host.ctypes.data), b"device"), (dict(mom=host.ctypes.data), b"device"), (dict(cnt=host.ctypes.data), b"device"),
                     (dict(out_sh=host.ctypes.data), b"device"), (dict(out_mom=host.ctypes.data), b"device"), (dict(out_cnt=host.ctypes.data), b"device"),
                     (dict(out_sh=D["sh"].ptr), b"overlap"), (dict(out_sh=D["sh"].ptr + 4 * 27 * (PROBES - 1)), b"overlap"),
                     (dict(out_mom=D["moments"].ptr), b"overlap"), (dict(out_cnt=D["counts"].ptr + 8), b"overlap"),
                     (dict(o=opts(h=1.0)), b"hysteresis"), (dict(o=opts(spp=0)), b"spp"), (dict(o=opts(md=0.0)), b"max_distance"),
                     (dict(o=opts(direct=4097)), b"direct_samples"), (dict(mom=None), b"all null"), (dict(out_cnt=None), b"both null")):
        rc = call(**kw)
        assert rc == 1 and b"mcpt_probe_volume_relight" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert info.launches == 7 and info.grew == 7 and info.staged_bytes == 7
    assert (out["sh"].get() == f32(SENTINEL)).all() and (out["moments"].get() == f32(SENTINEL)).all()  # nothing was written
    assert (out["counts"].get() == pdc.COUNT_SENTINEL).all()
    assert_equal(D["sh"].get(), c.vol.sh, "volume->sh")
    # ... and the handle still relights
    assert call() == 0 and info.launches >= 1
    want = prc.relight(hs, c.vol, True, spp=4, seed=1, hysteresis=0.5)[0]
    assert_equal(out["sh"].get(), want, "after the refusals")
    # the Python side: a buffer of the wrong size never reaches the library
    with pytest.raises(ValueError):
        hs.relight_probe_volume(*c.grid, D["sh"], out={"sh": pdc.Guarded((PROBES + 1, 27))})
    with pytest.raises(ValueError):
        hs.relight_probe_volume(*c.grid, D["sh"], moments=D["moments"], out={"sh": out["sh"]})


def test_torch_tensors_on_a_side_stream():
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_relight_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["on_side_stream"] and rec["outputs_are_torch"]
    assert rec["sh_differ"] == 0 and rec["moments_differ"] == 0 and rec["counts_differ"] == 0 and rec["chained_differ"] == 0
    assert rec["edit_behind_the_call"] and rec["after_edit_differ"] == 0
    assert rec["non_contiguous_refused"] and rec["overlap_refused"]
