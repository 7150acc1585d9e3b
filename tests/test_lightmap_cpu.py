"""The lightmap rule without a GPU (include/mcpt.h: mcpt_lightmap_texels_host, mcpt_lightmap_dilate_host): the header csrc/mcpt_lightmap.h
compiled for the CPU against the numpy restatement of tests/lightmap_cases.py, bit for bit, on every layout of CASES; the dilation on
scattered values; and the refusals that need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightmap_cases as lc  # noqa: E402

f32 = np.float32


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_texels_host_equals_the_model(pkg, hip, name, flip):
    sd, ob, W, H = lc.case_scene(pkg, name)
    got = hip.lightmap_texels(sd, ob, W, H, flip_normals=flip)
    want = lc.model_texels(sd, ob, W, H, flip)
    print("%s: %d of %d texels covered by %d triangles" % (name, len(want["texel"]), W * H, int(sd.objects["n_tri"][ob])))
    for w in lc.NAMES:
        assert lc.same_bits(got[w], want[w]), (name, w)
    assert (np.diff(got["texel"]) > 0).all()
    a = int(sd.objects["first_tri"][ob])
    assert ((got["prim"] >= a) & (got["prim"] < a + int(sd.objects["n_tri"][ob]))).all()


def test_expected_coverage_of_the_cases(pkg, hip):
    """What the layouts were made for, so that no case passes on an empty list."""
    n = {}
    for name in lc.CASES:
        sd, ob, W, H = lc.case_scene(pkg, name)
        n[name] = hip.lightmap_texels(sd, ob, W, H)
    assert len(n["quad 8x8"]["texel"]) == 64 and len(n["quad 13x7"]["texel"]) == 91 and len(n["quad 1x1"]["texel"]) == 1
    assert len(n["one triangle beyond 64x64"]["texel"]) == 64 * 64
    assert len(n["sub-texel triangles"]["texel"]) == 0
    assert 0 < len(n["chart partly outside"]["texel"]) < 16 * 12
    assert 60 <= len(n["huge coordinates"]["texel"]) < 120 and set(n["huge coordinates"]["prim"]) == {2, 4}
    assert len(n["grid of 512 at 64x64"]["texel"]) == 64 * 64 and len(np.unique(n["grid of 512 at 64x64"]["prim"])) == 512
    assert set(n["sub-texel among good"]["prim"]) == {2 + 20}  # the one good triangle (the light's two come first)
    assert set(n["degenerate among good"]["prim"]) == {2, 2 + 6}  # the two good triangles (the light's two come first)
    assert len(set(n["two overlapping charts"]["prim"])) == 4


@pytest.mark.parametrize("name", ["quad 8x8", "quad reversed winding"])
def test_the_lower_id_owns_the_shared_diagonal(pkg, hip, name):
    """The centres (x + 0.5) / 8 on the diagonal are exact, so both triangles cover them with a weight of exactly 0."""
    sd, ob, W, H = lc.case_scene(pkg, name)
    got = hip.lightmap_texels(sd, ob, W, H)
    a = int(sd.objects["first_tri"][ob])
    diag = np.arange(8) * 8 + np.arange(8)
    assert np.array_equal(got["texel"], np.arange(64))
    assert (got["prim"][diag] == a).all()
    assert set(got["prim"]) == {a, a + 1}
    on_edge = got["bary"][diag]
    assert (on_edge == 0).any(axis=1).all()


def test_winding_does_not_change_coverage(pkg, hip):
    a = hip.lightmap_texels(*lc.case_scene(pkg, "quad 8x8"))
    b = hip.lightmap_texels(*lc.case_scene(pkg, "quad reversed winding"))
    assert np.array_equal(a["texel"], b["texel"]) and np.array_equal(a["prim"], b["prim"])


def _values(n, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 4, size=(n, 3)).astype(f32)
    v[::7] *= f32(1e-3)
    return v


ISLAND = np.array([5 * 9 + 4], np.int32)  # one texel in a 9 x 9 map
COLUMN = (np.arange(2, 9) * 11 + 5).astype(np.int32)  # an island one texel wide in an 11 x 11 map
DILATE_CASES = {
    "empty list": (7, 5, np.zeros(0, np.int32)),
    "one texel": (9, 9, ISLAND),
    "island one texel wide": (11, 11, COLUMN),
    "corner and edge texels": (6, 4, np.array([0, 5, 18, 23, 9], np.int32)),
    "1x1 map": (1, 1, np.array([0], np.int32)),
    "a row": (13, 1, np.array([2, 3, 9], np.int32)),
}


@pytest.mark.parametrize("dilate", [0, 1, 3])
@pytest.mark.parametrize("name", sorted(DILATE_CASES))
def test_dilate_host_equals_the_model(hip, name, dilate):
    W, H, texel = DILATE_CASES[name]
    v = _values(len(texel))
    img, cov = hip.lightmap_dilate(W, H, texel, v, dilate)
    want_img, want_cov = lc.model_dilate(W, H, texel, v, dilate)
    assert lc.same_bits(img, want_img) and lc.same_bits(cov, want_cov), name
    assert (cov.reshape(-1)[texel] == 1).all() and lc.same_bits(img.reshape(-1, 3)[texel], v)
    if dilate == 0:
        assert int((cov != 0).sum()) == len(texel)
    assert not img[cov == 0].any()


@pytest.mark.parametrize("dilate", [0, 1, 3])
@pytest.mark.parametrize("name", ["two overlapping charts", "random triangles 29x23", "grid at 33x17"])
def test_dilate_host_on_a_chart(pkg, hip, name, dilate):
    sd, ob, W, H = lc.case_scene(pkg, name)
    texel = hip.lightmap_texels(sd, ob, W, H)["texel"]
    v = _values(len(texel), seed=8)
    img, cov = hip.lightmap_dilate(W, H, texel, v, dilate)
    want_img, want_cov = lc.model_dilate(W, H, texel, v, dilate)
    assert lc.same_bits(img, want_img) and lc.same_bits(cov, want_cov)


def test_dilation_grows_by_one_ring_per_round(hip):
    img, cov = hip.lightmap_dilate(9, 9, ISLAND, np.array([[1, 2, 3]], f32), 3)
    yy, xx = np.mgrid[0:9, 0:9]
    ring = np.maximum(abs(yy - 5), abs(xx - 4))
    assert np.array_equal(cov, np.where(ring == 0, 1, np.where(ring <= 3, 2, 0)).astype(np.uint8))
    assert (img[ring <= 3] == np.array([1, 2, 3], f32)).all()  # means of equal values


def test_texels_host_refusals(pkg, hip):
    sd, ob, W, H = lc.case_scene(pkg, "quad 8x8")
    cornell = pkg.scenes.cornell_demo(16, 16, 1)
    bad = [dict(sd=sd, object=-1), dict(sd=sd, object=2), dict(sd=sd, width=0), dict(sd=sd, height=0), dict(sd=sd, height=-3),
           dict(sd=sd, width=2 ** 16, height=2 ** 16), dict(sd=sd, width=(2 ** 31 - 1) // 3 + 1, height=1), dict(sd=cornell, object=6)]  # a sphere
    for kw in bad:
        args = dict(object=ob, width=W, height=H)
        args.update(kw)
        with pytest.raises(hip.McptError) as e:
            hip.lightmap_texels(args.pop("sd"), **args)
        assert e.value.code == 1 and "mcpt_lightmap_texels_host" in str(e.value), kw
    L = hip.lib()
    n = C.c_int64(-1)
    ld = hip.LightmapDesc(ob, W, H, 0)
    assert L.mcpt_lightmap_texels_host(None, C.byref(ld), None, None, None, None, None, C.byref(n)) == 1
    keep = []
    d = hip._make_desc(sd, keep)
    assert L.mcpt_lightmap_texels_host(C.byref(d), None, None, None, None, None, None, C.byref(n)) == 1
    assert L.mcpt_lightmap_texels_host(C.byref(d), C.byref(ld), None, None, None, None, None, None) == 1
    assert L.mcpt_lightmap_texels_host(C.byref(d), C.byref(ld), None, None, None, None, None, C.byref(n)) == 0 and n.value == 64  # every array is optional


def test_dilate_host_refusals(hip):
    v, t = np.zeros((2, 3), f32), np.array([0, 1], np.int32)
    for W, H, dilate in [(0, 4, 1), (4, 0, 1), (4, 4, -1), (2 ** 16, 2 ** 16, 0)]:
        with pytest.raises(hip.McptError) as e:
            hip.lightmap_dilate(W, H, t, v, dilate)
        assert e.value.code == 1
    with pytest.raises(hip.McptError):  # more values than texels
        hip.lightmap_dilate(1, 1, t, v, 0)
    L = hip.lib()
    img = np.zeros((4, 4, 3), f32)
    assert L.mcpt_lightmap_dilate_host(4, 4, 2, hip._ptr(t), hip._ptr(v), 1, None, None) == 1
    assert L.mcpt_lightmap_dilate_host(4, 4, 2, None, hip._ptr(v), 1, hip._ptr(img), None) == 1
    assert L.mcpt_lightmap_dilate_host(4, 4, 2, hip._ptr(t), None, 1, hip._ptr(img), None) == 1
    assert L.mcpt_lightmap_dilate_host(4, 4, 2, hip._ptr(t), hip._ptr(v), 1, hip._ptr(img), None) == 0  # coverage is optional
    # a texel index off the map is ignored
    off = np.array([3, 99, -1], np.int32)
    img, cov = hip.lightmap_dilate(4, 4, off, np.ones((3, 3), f32), 0)
    assert int(cov.sum()) == 1 and cov.reshape(-1)[3] == 1
