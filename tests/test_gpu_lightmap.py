"""mcpt_lightmap_texels / mcpt_lightmap_scatter / mcpt_bake_lightmap on the GPU.

The expectation of the texel pass is the host function (mcpt_lightmap_texels_host: csrc/mcpt_lightmap.h compiled for the CPU, which
tests/test_lightmap_cpu.py holds to the numpy restatement) on the description the scene stands for -- after an edit, the description
edited by the library's own host helpers.  The expectation of a bake is query_radiance at the sensors the texel pass returns, and the
numpy dilation of tests/lightmap_cases.py.  Every comparison is of bits.  Device buffers are made without torch
(tests/ray_query_cases.py), every output is followed by 64 guard elements that must survive.  torch and a non-default stream:
tests/lightmap_torch_child.py, a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightmap_cases as lc  # noqa: E402
from deform_cases import deformed_scene, object_positions, rotate_y, wave  # noqa: E402
from ray_query_cases import GUARD, DevBuf  # noqa: E402
from sensor_query_cases import radiance  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
# name -> (dtype, values per row, what the buffers hold before a call)
OUT = {"texel": (np.int32, 1, -77), "prim": (np.int32, 1, -78), "bary": (f32, 2, -9.5), "origins": (f32, 3, -10.5), "normals": (f32, 3, -11.5)}
BAKE = dict(spp=8, seed=6, spp_per_pass=4)


def texel_buffers(cap, want=lc.NAMES):
    return {w: DevBuf(shape=(cap,) if OUT[w][1] == 1 else (cap, OUT[w][1]), dtype=OUT[w][0], fill=OUT[w][2], guard=GUARD) for w in want}


def device_texels(hs, ob, W, H, flip=False, want=lc.NAMES):
    """lightmap_texels on the null stream into guarded buffers of W*H rows -> dict of numpy arrays cut to n; the rows behind n and the
    guards must be untouched."""
    out = texel_buffers(W * H, want)
    res, n = hs.lightmap_texels(ob, W, H, flip_normals=flip, want=want, out=out)
    assert set(res) == set(want) | {"texel"} and 0 <= n <= W * H
    got = {}
    for w in want:
        a = out[w].get()
        assert (a[n:] == OUT[w][0](OUT[w][2])).all(), "%s: rows behind n were written" % w
        got[w] = a[:n]
    return got


def assert_same(got, want, what):
    for w in want:
        if w in got:
            assert lc.same_bits(got[w], want[w]), "%s: %s differs (%d and %d rows)" % (what, w, len(got[w]), len(want[w]))


def planes(W, H, variance=False):
    out = {"image": DevBuf(shape=(H, W, 3), dtype=f32, fill=-3.5, guard=GUARD), "coverage": DevBuf(shape=(H, W), dtype=np.uint8, fill=0xAB, guard=GUARD)}
    if variance:
        out["variance"] = DevBuf(shape=(H, W, 3), dtype=f32, fill=-4.5, guard=GUARD)
    return out


def bake(hs, ob, W, H, dilate, variance=False, **kw):
    out = planes(W, H, variance)
    _, _, _, info, st = hs.bake_lightmap(ob, W, H, dilate=dilate, variance=variance, out=out, **kw)
    return out["image"].get(), out["coverage"].get(), (out["variance"].get() if variance else None), info, st


# ---------------------------------------------------------------- 1. texels against the host function
BUILDS = [(name, b) for name in sorted(lc.CASES) for b in ("sah", "lbvh")] + [("grid of 512 at 64x64", "ploc"), ("random triangles 29x23", "ploc")]


@pytest.mark.parametrize("name,builder", BUILDS)
def test_texels_equal_the_host_function(pkg, hip, name, builder):
    sd, ob, W, H = lc.case_scene(pkg, name)
    hs = hip.HipScene(sd, builder=builder)
    try:
        if builder == "sah" and name in ("quad 8x8", "grid of 512 at 64x64"):  # the two flavours of scene both occur
            assert hs.info()["lds_resident"] == (1 if name == "quad 8x8" else 0), hs.info()
        for flip in (False, True):
            want = hip.lightmap_texels(sd, ob, W, H, flip_normals=flip)
            assert_same(device_texels(hs, ob, W, H, flip), want, "%s, %s, flip %d" % (name, builder, flip))
        print("%s (%s): %d texels" % (name, builder, len(want["texel"])))
        # any selection of the optional outputs
        assert_same(device_texels(hs, ob, W, H, want=("texel",)), want, name + ", texel alone")
        assert_same(device_texels(hs, ob, W, H, want=("origins", "texel")), want, name + ", origins and texel")
    finally:
        hs.close()


def test_the_lower_id_owns_the_shared_diagonal(pkg, hip):
    sd, ob, W, H = lc.case_scene(pkg, "quad 8x8")
    hs = hip.HipScene(sd)
    got = device_texels(hs, ob, W, H)
    hs.close()
    a = int(sd.objects["first_tri"][ob])
    assert np.array_equal(got["texel"], np.arange(64)) and (got["prim"][np.arange(8) * 9] == a).all() and set(got["prim"]) == {a, a + 1}


@pytest.mark.parametrize("name", lc.PLANAR + ("cornell",))
def test_normals_are_those_of_query_closest(pkg, hip, name):
    """A ray from just above a sensor straight down onto it: where it hits the sensor's own triangle, query_closest reports the bits of the
    sensor's normal."""
    if name == "cornell":
        sd, ob, W, H = lc.cornell_charted(pkg), 0, 24, 24
    else:
        sd, ob, W, H = lc.case_scene(pkg, name)
    hs = hip.HipScene(sd, builder="sah")
    try:
        got = device_texels(hs, ob, W, H)
        n = len(got["texel"])
        scale = f32(0.5 if name == "cornell" else 1e-2)
        o = (got["origins"] + got["normals"] * scale).astype(f32)
        d = (-got["normals"]).astype(f32)
        out = {"prim": DevBuf(shape=(n,), dtype=np.int32, fill=-77, guard=GUARD), "normal": DevBuf(shape=(n, 3), dtype=f32, fill=-10.5, guard=GUARD)}
        hs.query_closest(DevBuf(o), DevBuf(d), want=("prim", "normal"), out=out)
        prim, nrm = out["prim"].get(), out["normal"].get()
        own = prim == got["prim"]
        print("%s: %d of %d rays hit their sensor's triangle" % (name, int(own.sum()), n))
        assert n > 0 and own.sum() >= 0.8 * n
        assert lc.same_bits(nrm[own], got["normals"][own])
    finally:
        hs.close()


# ---------------------------------------------------------------- 2. live scenes
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_texels_of_a_live_scene(pkg, hip, builder):
    sd = lc.cornell_charted(pkg)
    W, H, ob = 40, 24, 0
    hs = hip.HipScene(sd, builder=builder)
    try:
        def check(now, o, what):
            want = hip.lightmap_texels(now, o, W, H)
            assert len(want["texel"]) > 100, what
            assert_same(device_texels(hs, o, W, H), want, "%s (%s)" % (what, builder))
            return want

        fresh = check(sd, ob, "fresh")
        m = rotate_y(0.3, (278.0, 0.0, 279.6), shift=(5.0, 2.0, -3.0))
        hs.update([(ob, m)])
        moved = check(deformed_scene(pkg, hip, sd, {}, {ob: m}), ob, "update with a rotation")
        assert np.array_equal(moved["texel"], fresh["texel"]) and not lc.same_bits(moved["origins"], fresh["origins"])
        assert not lc.same_bits(moved["normals"], fresh["normals"])
        P = wave(object_positions(sd, ob))
        hs.deform([(ob, P)])
        now = deformed_scene(pkg, hip, sd, {ob: P}, {ob: m})
        bent = check(now, ob, "deform")
        assert not lc.same_bits(bent["origins"], moved["origins"])
        # an added mesh: its triangles follow every triangle the scene had, and the spheres' ids move up behind them
        case, cob, _, _ = lc.case_scene(pkg, "grid at 33x17")
        a, k = int(case.objects["first_tri"][cob]), int(case.objects["n_tri"][cob])
        tris = case.triangles[a:a + k].copy()
        for v in ("v0", "v1", "v2"):
            tris[v] = (tris[v] * f32(40.0) + np.array([200.0, 150.0, 200.0], f32)).astype(f32)
        obj = np.zeros(1, sd.objects.dtype)
        obj["kind"], obj["material"], obj["first_tri"], obj["n_tri"] = 0, 0, 0, k
        first, _ = hs.add_objects(obj, tris)
        ext = hip.extend_scene(now, obj, tris)
        assert first == len(sd.objects) and int(ext.objects["first_tri"][first]) == len(sd.triangles)
        added = check(ext, first, "add_objects: the added mesh")
        assert added["prim"].min() >= len(sd.triangles)
        check(ext, ob, "add_objects: the first mesh")
        # hidden: the records stay, and so do the sensors
        hs.set_visibility([(ob, False)])
        assert hs.visibility()[0][ob] == 0
        check(ext, ob, "hidden")
        img, cov, _, info, _ = bake(hs, ob, 16, 16, 0, **BAKE)
        tex = device_texels(hs, ob, 16, 16)
        rad, _, _ = radiance(hs, tex["origins"], tex["normals"], kind="hemisphere", **BAKE)
        assert info["n_texels"] == len(tex["texel"]) > 0 and lc.same_bits(img.reshape(-1, 3)[tex["texel"]], rad), "bake of the hidden object"
        assert rad.any()  # it receives the light of the scene without it
        hs.set_visibility([(ob, True)])
        check(ext, ob, "shown again")
    finally:
        hs.close()


# ---------------------------------------------------------------- 3. the bake
@pytest.fixture(scope="module")
def cornell(pkg, hip):
    sd = lc.cornell_charted(pkg)
    hs = hip.HipScene(sd, builder="sah")
    yield hs, sd
    hs.close()


def test_bake_is_texels_radiance_scatter(pkg, hip, cornell):
    hs, sd = cornell
    W = H = 16
    tex = device_texels(hs, 0, W, H)
    n = len(tex["texel"])
    assert 0 < n < W * H  # the margin of the chart stays empty
    rad, var, _ = radiance(hs, tex["origins"], tex["normals"], kind="hemisphere", variance=True, **BAKE)
    assert rad.any() and np.isfinite(rad).all()
    img, cov, vimg, info, st = bake(hs, 0, W, H, 0, variance=True, **BAKE)
    print("16x16 floor: %d texels, %d items; bake info %s" % (n, info["items"], info))
    assert info["n_texels"] == n and info["items"] > 0 and st.samples == n * BAKE["spp"]
    covered = np.zeros(W * H, bool)
    covered[tex["texel"]] = True
    assert lc.same_bits(img.reshape(-1, 3)[tex["texel"]], rad) and lc.same_bits(vimg.reshape(-1, 3)[tex["texel"]], var)
    assert not img.reshape(-1, 3)[~covered].any() and not vimg.reshape(-1, 3)[~covered].any()
    assert np.array_equal(cov.reshape(-1), covered.astype(np.uint8))
    for dilate in (1, 2, 3):  # odd and even: either plane of the ping-pong is the first
        want_img, want_cov = lc.model_dilate(W, H, tex["texel"], rad, dilate)
        got_img, got_cov, got_var, _, _ = bake(hs, 0, W, H, dilate, variance=True, **BAKE)
        assert lc.same_bits(got_img, want_img) and lc.same_bits(got_cov, want_cov), dilate
        assert lc.same_bits(got_var, vimg), "the variance is not dilated"
        assert (got_cov == 2).any()
    # flipped normals: the sensors look down through the floor
    fimg, _, _, _, _ = bake(hs, 0, W, H, 0, flip_normals=True, **BAKE)
    ftex = device_texels(hs, 0, W, H, flip=True)
    frad, _, _ = radiance(hs, ftex["origins"], ftex["normals"], kind="hemisphere", **BAKE)
    assert lc.same_bits(fimg.reshape(-1, 3)[ftex["texel"]], frad) and not lc.same_bits(frad, rad)


@pytest.mark.parametrize("dilate", [0, 1, 2, 5])
def test_scatter_equals_the_model(pkg, hip, cornell, dilate):
    hs, sd = cornell
    W, H = 33, 17
    tex = device_texels(hs, 0, W, H, want=("texel",))["texel"]
    rng = np.random.default_rng(dilate)
    v = rng.uniform(0, 3, size=(len(tex), 3)).astype(f32)
    want_img, want_cov = lc.model_dilate(W, H, tex, v, dilate)
    out = planes(W, H)
    hs.lightmap_scatter(0, W, H, DevBuf(tex, dtype=np.int32), DevBuf(v), dilate=dilate, out=out)
    assert lc.same_bits(out["image"].get(), want_img) and lc.same_bits(out["coverage"].get(), want_cov)
    only = {"image": DevBuf(shape=(H, W, 3), dtype=f32, fill=-3.5, guard=GUARD)}
    hs.lightmap_scatter(0, W, H, DevBuf(tex, dtype=np.int32), DevBuf(v), dilate=dilate, coverage=False, out=only)
    assert lc.same_bits(only["image"].get(), want_img)
    # an empty list: a zero map
    hs.lightmap_scatter(0, W, H, DevBuf(np.zeros(0, np.int32), dtype=np.int32), DevBuf(np.zeros((0, 3), f32)), dilate=dilate, out=out)
    assert not out["image"].get().any() and not out["coverage"].get().any()


def test_an_object_without_a_covered_texel(pkg, hip):
    sd, ob, W, H = lc.case_scene(pkg, "sub-texel triangles")
    hs = hip.HipScene(sd)
    img, cov, var, info, st = bake(hs, ob, W, H, 2, variance=True, **BAKE)
    hs.close()
    assert info["n_texels"] == 0 and st.samples == 0 and not img.any() and not cov.any() and not var.any()


def test_steady_state_allocates_nothing(pkg, hip):
    sd = lc.cornell_charted(pkg)
    hs = hip.HipScene(sd, builder="sah")
    try:
        a = bake(hs, 0, 16, 16, 2, variance=True, **BAKE)
        b = bake(hs, 0, 16, 16, 2, variance=True, **BAKE)
        assert a[3]["grew"] == 1 and b[3]["grew"] == 0
        assert all(lc.same_bits(x, y) for x, y in zip(a[:3], b[:3]))
        c = bake(hs, 0, 48, 32, 2, variance=True, **BAKE)
        d = bake(hs, 0, 48, 32, 2, variance=True, **BAKE)
        e = bake(hs, 0, 16, 16, 2, variance=True, **BAKE)  # a smaller map afterwards fits what is there
        assert c[3]["grew"] == 1 and d[3]["grew"] == 0 and e[3]["grew"] == 0
        assert all(lc.same_bits(x, y) for x, y in zip(c[:3], d[:3])) and all(lc.same_bits(x, y) for x, y in zip(a[:3], e[:3]))
    finally:
        hs.close()


# ---------------------------------------------------------------- 4. refusals that need a device
def test_refusals_on_a_live_scene(pkg, hip, cornell):
    hs, sd = cornell
    L = hip.lib()
    W = H = 8
    bufs = texel_buffers(W * H)
    img = planes(W, H, variance=True)
    host = np.zeros((H, W, 3), f32)
    p = hs.params(**BAKE)
    n = C.c_int64(-5)

    def ptr(b):
        return C.c_void_p(b.ptr)

    def texels(desc, texel=None, prim=None):
        out = hip.LightmapTexelsOut(texel=(texel if texel is not None else bufs["texel"].ptr), prim=prim)
        return L.mcpt_lightmap_texels(hs.h, C.byref(desc), C.byref(out), C.byref(n), None)

    def bake_rc(desc, params=p, dilate=1, image=None, variance=None):
        return L.mcpt_bake_lightmap(hs.h, C.byref(desc), C.byref(params), dilate, C.c_void_p(image if image is not None else img["image"].ptr),
                                    ptr(img["coverage"]), C.c_void_p(variance), None, None, None)

    def scatter_rc(desc, nn=4, texel=None, values=None, dilate=1, image=None):
        return L.mcpt_lightmap_scatter(hs.h, C.byref(desc), nn, C.c_void_p(texel if texel is not None else bufs["texel"].ptr),
                                       C.c_void_p(values if values is not None else bufs["origins"].ptr), dilate,
                                       C.c_void_p(image if image is not None else img["image"].ptr), None, None)

    good = hip.LightmapDesc(0, W, H, 0)
    bad_descs = {"object": hip.LightmapDesc(len(sd.objects), W, H, 0), "sphere": hip.LightmapDesc(6, W, H, 0), "width": hip.LightmapDesc(0, 0, H, 0),
                 "width and height": hip.LightmapDesc(0, 2 ** 15, 2 ** 15, 0)}
    for k in range(4):
        d = hip.LightmapDesc(0, W, H, 0)
        d.reserved[k] = 7
        bad_descs["reserved"] = d
        for rc in (texels(d), bake_rc(d), scatter_rc(d)):
            assert rc == 1 and b"reserved" in L.mcpt_last_error()
    for what, d in bad_descs.items():
        for rc in (texels(d), bake_rc(d), scatter_rc(d)):
            assert rc == 1 and what.split()[0].encode() in L.mcpt_last_error(), (what, L.mcpt_last_error())
    # pointers that are not device memory
    assert texels(good, texel=host.ctypes.data) == 1 and b"device" in L.mcpt_last_error()
    assert texels(good, prim=host.ctypes.data) == 1 and b"device" in L.mcpt_last_error()
    assert texels(good, texel=0) == 1 and b"null" in L.mcpt_last_error()
    assert bake_rc(good, image=host.ctypes.data) == 1 and b"device" in L.mcpt_last_error()
    assert bake_rc(good, variance=host.ctypes.data) == 1 and b"device" in L.mcpt_last_error()
    assert scatter_rc(good, image=host.ctypes.data) == 1 and scatter_rc(good, texel=host.ctypes.data) == 1 and scatter_rc(good, values=host.ctypes.data) == 1
    # the other arguments
    assert scatter_rc(good, dilate=-1) == 1 and b"dilate" in L.mcpt_last_error()
    assert scatter_rc(good, nn=-1) == 1 and scatter_rc(good, nn=W * H + 1) == 1
    assert bake_rc(good, dilate=-1) == 1 and b"dilate" in L.mcpt_last_error()
    for kw, word in ((dict(spp=0), b"spp"), (dict(n_dir_sample=0), b"n_dir_sample"), (dict(nranks=2), b"nranks"), (dict(rank=1), b"rank"),
                     (dict(sample_offset=1), b"sample_offset"), (dict(spp_total=16), b"spp_total"), (dict(accumulate=1), b"accumulate")):
        args = dict(BAKE)
        args.update(kw)
        assert bake_rc(good, params=hs.params(**args)) == 1 and word in L.mcpt_last_error(), kw
    assert bake_rc(good, params=hs.params(spp=1), variance=img["variance"].ptr) == 1 and b"variance" in L.mcpt_last_error()
    # nothing was written by any of them
    assert (bufs["texel"].get() == -77).all() and (img["image"].get() == f32(-3.5)).all() and (img["variance"].get() == f32(-4.5)).all() and n.value == -5
    # and the scene still answers
    assert texels(good) == 0 and n.value > 0


def test_an_instanced_scene_is_refused(pkg, hip):
    sd = pkg.scenes.chess_scene(width=32, height=32, spp=1)
    hs = hip.HipScene(sd, builder="sah", instancing=True)
    try:
        assert hs.info()["n_instances"] > 0
        mesh = int(np.flatnonzero(sd.objects["kind"] == 0)[0])
        with pytest.raises(hip.McptError) as e:
            hs.lightmap_texels(mesh, 8, 8, out=texel_buffers(64))
        assert e.value.code == 1 and "instanced" in str(e.value)
        with pytest.raises(hip.McptError) as e:
            hs.bake_lightmap(mesh, 8, 8, out=planes(8, 8), **BAKE)
        assert e.value.code == 1 and "instanced" in str(e.value)
    finally:
        hs.close()


# ---------------------------------------------------------------- 5. torch and streams
def test_torch_tensors_on_a_side_stream():
    """tests/lightmap_torch_child.py (torch imported first): values produced by a torch kernel on a non-default stream and scattered on
    that stream, texels and a bake whose outputs the calls allocate as torch tensors, against the numpy path in the same process."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "lightmap_torch_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    if rec.get("error") == "torch sees no GPU":
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "error" not in rec, rec
    assert rec["n"] > 0 and rec["on_side_stream"] and rec["outputs_are_torch"]
    assert rec["texels_differ"] == 0 and rec["scatter_differ"] == 0 and rec["staged_scatter_differ"] == 0 and rec["bake_differ"] == 0
    assert rec["non_contiguous_refused"]
