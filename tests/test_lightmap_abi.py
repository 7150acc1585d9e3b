"""The lightmap calls without a GPU (include/mcpt.h: mcpt_lightmap_texels, mcpt_lightmap_scatter, mcpt_bake_lightmap): the struct sizes,
the refusal of a null scene and of reserved words, and the checks of HipScene.lightmap_texels / lightmap_scatter / bake_lightmap that
raise before the library is called (the buffers here are fake objects that only expose __cuda_array_interface__)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightmap_cases as lc  # noqa: E402
from ray_query_cases import FakeDevice  # noqa: E402


def test_struct_sizes(hip):
    assert C.sizeof(hip.LightmapDesc) == 32
    assert C.sizeof(hip.LightmapTexelsOut) == 40
    assert C.sizeof(hip.LightmapInfo) == 64
    assert hip.LightmapInfo.ms_texels.offset == 24 and hip.LightmapInfo.reserved.offset == 48
    assert tuple(hip.LIGHTMAP_OUTPUTS) == ("texel", "prim", "bary", "origins", "normals") == lc.NAMES


def test_null_scene_and_null_desc_are_refused(hip):
    L = hip.lib()
    d, out, n = hip.LightmapDesc(0, 8, 8, 0), hip.LightmapTexelsOut(), C.c_int64(0)
    p = hip.Params(spp=1, rr_rate=0.8, n_dir_sample=1, nranks=1)
    assert L.mcpt_lightmap_texels(None, C.byref(d), C.byref(out), C.byref(n), None) == 1
    assert b"mcpt_lightmap_texels: null scene" in L.mcpt_last_error()
    assert L.mcpt_lightmap_scatter(None, C.byref(d), 0, None, None, 0, None, None, None) == 1
    assert b"mcpt_lightmap_scatter: null scene" in L.mcpt_last_error()
    assert L.mcpt_bake_lightmap(None, C.byref(d), C.byref(p), 0, None, None, None, None, None, None) == 1
    assert b"mcpt_bake_lightmap: null scene" in L.mcpt_last_error()


def test_reserved_words_are_refused_by_the_host_form(pkg, hip):
    """The device calls share the check (tests/test_gpu_lightmap.py asks them on a live scene)."""
    sd, ob, W, H = lc.case_scene(pkg, "quad 8x8")
    L, keep, n = hip.lib(), [], C.c_int64(0)
    desc = hip._make_desc(sd, keep)
    for k in range(4):
        d = hip.LightmapDesc(ob, W, H, 0)
        d.reserved[k] = 1
        assert L.mcpt_lightmap_texels_host(C.byref(desc), C.byref(d), None, None, None, None, None, C.byref(n)) == 1
        assert b"reserved" in L.mcpt_last_error()


class NoLibraryScene:
    """The lightmap methods of HipScene over a handle that must never be used: every case below is refused before the library is called."""

    def __init__(self, hip):
        self.h, self.L, self.sd, self.device = None, None, None, 0
        for m in ("lightmap_texels", "lightmap_scatter", "bake_lightmap", "_lightmap_planes"):
            setattr(self, m, getattr(hip.HipScene, m).__get__(self))

    def params(self, **kw):
        raise AssertionError("the parameters were built: the inputs passed their checks")


def _texel_out(cap, **bad):
    out = {"texel": FakeDevice((cap,), "<i4"), "prim": FakeDevice((cap,), "<i4"), "bary": FakeDevice((cap, 2)), "origins": FakeDevice((cap, 3)),
           "normals": FakeDevice((cap, 3))}
    out.update(bad)
    return out


def test_bad_texel_outputs_raise_before_the_library(hip):
    hs = NoLibraryScene(hip)
    cap = 8 * 4
    for bad in (dict(texel=FakeDevice((cap,), "<f4")), dict(prim=FakeDevice((cap - 1,), "<i4")), dict(bary=FakeDevice((cap, 3))),
                dict(origins=FakeDevice((cap * 3,))), dict(normals=FakeDevice((cap, 3), "<f8")), dict(origins=FakeDevice((cap, 3), strides=(4, 4 * cap))),
                dict(normals=np.zeros((cap, 3), np.float32))):
        with pytest.raises(ValueError):
            hs.lightmap_texels(1, 8, 4, out=_texel_out(cap, **bad))
    with pytest.raises(ValueError):  # a wanted output without a buffer ("texel" is always wanted)
        hs.lightmap_texels(1, 8, 4, want=("prim",), out={"prim": FakeDevice((cap,), "<i4")})
    for want in (("texel", "texel"), ("point",), ("texel", "uv")):
        with pytest.raises(ValueError):
            hs.lightmap_texels(1, 8, 4, want=want, out=_texel_out(cap))
    with pytest.raises(AttributeError):  # and good buffers do get as far as the library (which this scene does not have)
        hs.lightmap_texels(1, 8, 4, out=_texel_out(cap))


def test_bad_planes_raise_before_the_library(hip):
    hs = NoLibraryScene(hip)
    W, H, n = 8, 4, 5
    texel, values = FakeDevice((n,), "<i4"), FakeDevice((n, 3))
    good = {"image": FakeDevice((H, W, 3)), "coverage": FakeDevice((H, W), "|u1"), "variance": FakeDevice((H, W, 3))}
    for name, bad in (("image", FakeDevice((W, H, 3))), ("image", FakeDevice((H * W * 3,))), ("image", FakeDevice((H, W, 3), "<f8")),
                      ("coverage", FakeDevice((H, W), "<i4")), ("coverage", FakeDevice((H, W, 1), "|u1")), ("variance", FakeDevice((H, W)))):
        out = dict(good)
        out[name] = bad
        with pytest.raises(ValueError):
            hs.bake_lightmap(0, W, H, variance=True, out=out)
        if name != "variance":
            with pytest.raises(ValueError):
                hs.lightmap_scatter(0, W, H, texel, values, out=out)
    with pytest.raises(ValueError):
        hs.bake_lightmap(0, W, H, out={"image": good["image"]})  # no coverage
    for t, v in ((FakeDevice((n,), "<f4"), values), (FakeDevice((n, 1), "<i4"), values), (texel, FakeDevice((n + 1, 3))), (texel, FakeDevice((n * 3,)))):
        with pytest.raises(ValueError):
            hs.lightmap_scatter(0, W, H, t, v, out=good)
    with pytest.raises(AssertionError):  # good planes get as far as the parameters
        hs.bake_lightmap(0, W, H, variance=True, out=good)
