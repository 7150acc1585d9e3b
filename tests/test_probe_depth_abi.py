"""The probe-visibility ABI without a GPU (include/mcpt.h: mcpt_probe_depth_params, mcpt_probe_visibility and the calls that take them):
struct sizes and exports, the refusals that need no device, and the checks of HipScene.query_probe_depth / probe_shade_visible /
bake_probe_volume that raise before the library is called."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402
from test_probes_cpu import grid_struct  # noqa: E402

f32 = np.float32


def test_struct_sizes_and_exports(hip):
    assert C.sizeof(hip.ProbeDepthParams) == 32 and C.sizeof(hip.ProbeVisibility) == 16
    assert hip.PROBE_DEPTH_RES == 8 and hip.PROBE_DEPTH_ROW == 192
    L = hip.lib()
    for s in ("mcpt_query_probe_depth", "mcpt_probe_shade_visible", "mcpt_bake_probe_volume", "mcpt_probe_depth_dirs_host",
              "mcpt_probe_depth_texel_host", "mcpt_probe_depth_fold_host", "mcpt_probe_shade_visible_host"):
        assert s in hip.EXPORTS and hasattr(L, s)


def depth_params(hip, seed=1, spp=4, sample_offset=0, accumulate=0, max_distance=2.0, reserved=(0, 0, 0)):
    return hip.ProbeDepthParams(seed, spp, sample_offset, accumulate, max_distance, (C.c_int32 * 3)(*reserved))


def visibility(hip, normal_bias=0.0, backface_max=0.25, reserved=(0, 0)):
    return hip.ProbeVisibility(normal_bias, backface_max, (C.c_int32 * 2)(*reserved))


def test_host_forms_refuse_bad_arguments(hip):
    L = hip.lib()
    d, r, bf = np.zeros((2, 4, 3), f32), np.ones((2, 4), f32), np.zeros((2, 4), np.uint8)
    mom, cnt = np.full((2, 192), -13.5, f32), np.full((2, 2), -7, np.int32)
    P = [a.ctypes.data for a in (d, r, bf)]

    def fold(n=2, spp=4, acc=0, ptrs=P, m=mom.ctypes.data, c=cnt.ctypes.data):
        return L.mcpt_probe_depth_fold_host(n, spp, ptrs[0], ptrs[1], ptrs[2], acc, m, c)

    for kw, word in ((dict(n=-1), b"n must"), (dict(n=(2 ** 31 - 1) // 192 + 1), b"n must"), (dict(spp=0), b"spp"), (dict(spp=-3), b"spp"),
                     (dict(acc=2), b"accumulate"), (dict(ptrs=[None, P[1], P[2]]), b"null"), (dict(m=None), b"null"), (dict(c=None), b"null"),
                     (dict(acc=1), b"counts")):  # (accumulate onto negative counts)
        rc = fold(**kw)
        assert rc == 1 and b"mcpt_probe_depth_fold_host" in L.mcpt_last_error() and word in L.mcpt_last_error(), (rc, L.mcpt_last_error())
    full = np.array([[2 ** 31 - 4, 0], [0, 0]], np.int32)
    assert fold(acc=1, c=full.ctypes.data) == 1 and b"int32" in L.mcpt_last_error()  # 2^31 - 4 + 4 samples do not fit
    assert (mom == f32(-13.5)).all() and (cnt == -7).all() and full[0, 0] == 2 ** 31 - 4  # nothing was written
    assert fold(n=0, ptrs=[None] * 3, m=None, c=None) == 0  # n == 0: a valid no-op
    assert L.mcpt_probe_depth_dirs_host(None) == 1 and b"null" in L.mcpt_last_error()
    assert L.mcpt_probe_depth_texel_host(1, None, None) == 1 and L.mcpt_probe_depth_texel_host(-1, P[0], cnt.ctypes.data) == 1
    assert L.mcpt_probe_depth_texel_host(0, None, None) == 0
    # the host lookup: the grid's refusals, the options', null pointers
    sh, m8, c8 = np.zeros((8, 27), f32), np.zeros((8, 192), f32), np.zeros((8, 2), np.int32)
    p = n = np.zeros((4, 3), f32)
    out = np.full((4, 3), -13.5, f32)

    def look(g=None, o=None, coef=sh.ctypes.data, k=4):
        g, o = g or grid_struct(hip), o or visibility(hip)
        return L.mcpt_probe_shade_visible_host(C.byref(g), coef, m8.ctypes.data, c8.ctypes.data, C.byref(o), k, p.ctypes.data, n.ctypes.data, out.ctypes.data, None)

    for kw, word in ((dict(g=grid_struct(hip, dims=(0, 2, 2))), b"dims"), (dict(g=grid_struct(hip, spacing=(1, 0, 1))), b"spacing"),
                     (dict(g=grid_struct(hip, reserved=(0, 1, 0))), b"reserved"), (dict(g=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 2))), b"192"),
                     (dict(o=visibility(hip, normal_bias=-0.1)), b"normal_bias"), (dict(o=visibility(hip, normal_bias=float("nan"))), b"normal_bias"),
                     (dict(o=visibility(hip, backface_max=-1.0)), b"backface_max"), (dict(o=visibility(hip, backface_max=float("inf"))), b"backface_max"),
                     (dict(o=visibility(hip, reserved=(0, 3))), b"reserved"), (dict(coef=None), b"null"), (dict(k=-1), b"n < 0")):
        rc = look(**kw)
        assert rc == 1 and b"mcpt_probe_shade_visible_host" in L.mcpt_last_error() and word in L.mcpt_last_error(), (rc, L.mcpt_last_error())
    g = grid_struct(hip)
    assert L.mcpt_probe_shade_visible_host(C.byref(g), sh.ctypes.data, m8.ctypes.data, c8.ctypes.data, None, 4, p.ctypes.data, n.ctypes.data, out.ctypes.data, None) == 1
    assert (out == f32(-13.5)).all()
    assert look(k=0) == 0


def test_device_calls_refuse_before_any_device_work(hip):
    """Without a scene nothing can reach the device: the null scene is refused first, by name."""
    L = hip.lib()
    g, o, dp = grid_struct(hip), visibility(hip), depth_params(hip)
    prm = hip.Params(spp=1, rr_rate=0.8, n_dir_sample=1, nranks=1)
    assert L.mcpt_query_probe_depth(None, C.byref(dp), 1, None, None, None, None, None) == 1 and b"mcpt_query_probe_depth: null scene" in L.mcpt_last_error()
    assert L.mcpt_probe_shade_visible(None, C.byref(g), None, None, None, C.byref(o), 0, None, None, None, None, None) == 1
    assert b"mcpt_probe_shade_visible: null scene" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_volume(None, C.byref(g), C.byref(prm), C.byref(dp), None, None, None, None, None) == 1
    assert b"mcpt_bake_probe_volume: null scene" in L.mcpt_last_error()
    info = hip.QueryInfo(7, 7, 7)
    assert L.mcpt_query_probe_depth(None, C.byref(dp), 1, None, None, None, None, C.byref(info)) == 1 and info.launches == 0 and info.grew == 0


# ---------------------------------------------------------------- Python-side validation before the library
class NoLibraryScene:
    """The probe-visibility methods of HipScene over a handle that must never be used."""

    def __init__(self, hip):
        self.h, self.L, self.sd, self.device = None, None, None, 0
        for m in ("query_probe_depth", "probe_shade_visible", "bake_probe_volume"):
            setattr(self, m, getattr(hip.HipScene, m).__get__(self))

    def params(self, **kw):
        raise AssertionError("the parameters were built: the inputs passed their checks")


def test_bad_depth_inputs_raise_before_the_library(hip):
    hs, n = NoLibraryScene(hip), 8
    o = FakeDevice((n, 3))
    good = {"moments": FakeDevice((n, 192)), "counts": FakeDevice((n, 2), "<i4")}
    for bad in (FakeDevice((n, 3), "<f8"), FakeDevice((n * 3,)), FakeDevice((n, 4)), FakeDevice((n, 3), strides=(4, 4 * n)), np.zeros((n, 3), f32)):
        with pytest.raises(ValueError):
            hs.query_probe_depth(bad, 4, 2.0, out=good)
    for kw in (dict(spp=0), dict(spp=-1), dict(spp=2 ** 31), dict(spp=2, sample_offset=-1), dict(spp=2, sample_offset=2 ** 31 - 2),
               dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("inf")), dict(max_distance=float("nan"))):
        a = dict(spp=4, max_distance=2.0)
        a.update(kw)
        with pytest.raises(ValueError):
            hs.query_probe_depth(o, a.pop("spp"), a.pop("max_distance"), out=good, **a)
    with pytest.raises(ValueError):  # no torch tensors: the outputs must be supplied
        hs.query_probe_depth(o, 4, 2.0)
    for name, bad in (("moments", FakeDevice((n, 64))), ("moments", FakeDevice((n, 192), "<f8")), ("moments", FakeDevice((n - 1, 192))),
                      ("counts", FakeDevice((n, 2))), ("counts", FakeDevice((n,), "<i4")), ("counts", FakeDevice((n, 2), "<i4", strides=(4, 4 * n)))):
        out = dict(good)
        out[name] = bad
        with pytest.raises(ValueError):
            hs.query_probe_depth(o, 4, 2.0, out=out)
    with pytest.raises(ValueError):
        hs.query_probe_depth(o, 4, 2.0, out={"moments": good["moments"]})
    with pytest.raises(AttributeError):  # good buffers get as far as the library (which this scene does not have)
        hs.query_probe_depth(o, 4, 2.0, out=good)


def test_bad_visible_lookups_raise_before_the_library(hip):
    hs, n = NoLibraryScene(hip), 8
    dims, m = (3, 2, 4), 24
    good = dict(sh=FakeDevice((m, 27)), moments=FakeDevice((m, 192)), counts=FakeDevice((m, 2), "<i4"), points=FakeDevice((n, 3)),
                normals=FakeDevice((n, 3)), out=FakeDevice((n, 3)), weight=FakeDevice((n,)))

    def call(origin=(0, 0, 0), spacing=(1, 1, 1), dims=dims, normal_bias=0.0, backface_max=0.25, **kw):
        a = dict(good)
        a.update(kw)
        return hs.probe_shade_visible(origin, spacing, dims, a["sh"], a["moments"], a["counts"], a["points"], a["normals"], normal_bias=normal_bias,
                                      backface_max=backface_max, weight=a["weight"], out=a["out"])

    for kw in (dict(dims=(0, 2, 4)), dict(dims=(3, 2)), dict(dims=(2 ** 12, 2 ** 12, 2)), dict(spacing=(1, 0, 1)), dict(normal_bias=-1.0),
               dict(normal_bias=float("nan")), dict(backface_max=-0.5), dict(backface_max=float("inf")), dict(sh=FakeDevice((m - 1, 27))),
               dict(moments=FakeDevice((m, 64))), dict(moments=FakeDevice((m, 192), "<f8")), dict(counts=FakeDevice((m, 2))),
               dict(counts=FakeDevice((m, 3), "<i4")), dict(points=FakeDevice((n, 4))), dict(normals=FakeDevice((n + 1, 3))),
               dict(weight=FakeDevice((n, 1))), dict(weight=FakeDevice((n,), "<f8")), dict(out=FakeDevice((n, 3), strides=(4, 4 * n))), dict(out=None),
               dict(points=np.zeros((n, 3), f32))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(AttributeError):
        call()
    with pytest.raises(AttributeError):
        call(weight=None)
    # the composite
    out = {"sh": good["sh"], "moments": good["moments"], "counts": good["counts"]}
    for kw in (dict(dims=(0, 2, 4)), dict(depth_spp=0), dict(max_distance=0.0), dict(out={"sh": good["sh"], "moments": good["moments"]}),
               dict(out=dict(out, counts=FakeDevice((m, 2)))), dict(out=dict(out, moments=FakeDevice((m, 27))))):
        a = dict(dims=dims, depth_spp=8, max_distance=2.0, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            hs.bake_probe_volume((0, 0, 0), (1, 1, 1), a["dims"], a["depth_spp"], a["max_distance"], out=a["out"])
    with pytest.raises(AssertionError):  # good inputs get as far as the parameters
        hs.bake_probe_volume((0, 0, 0), (1, 1, 1), dims, 8, 2.0, out=out)
    # the module-level host forms
    z = np.zeros
    with pytest.raises(ValueError):
        hip.probe_depth_fold(z((2, 4, 3), f32), z((2, 3), f32), z((2, 4)))
    with pytest.raises(ValueError):
        hip.probe_depth_fold(z((2, 0, 3), f32), z((2, 0), f32), z((2, 0)))
    with pytest.raises(ValueError):
        hip.probe_depth_fold(z((2, 4, 3), f32), z((2, 4), f32), z((2, 4)), moments=z((2, 192), f32))
    with pytest.raises(ValueError):
        hip.probe_shade_visible((0, 0, 0), (1, 1, 1), dims, z((m, 27)), z((m, 64)), z((m, 2)), z((n, 3)), z((n, 3)))
    with pytest.raises(ValueError):
        hip.probe_shade_visible((0, 0, 0), (1, 1, 1), dims, z((m, 27)), z((m, 192)), z((m, 2)), z((n, 3)), z((n, 3)), backface_max=-1)
