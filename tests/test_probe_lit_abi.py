"""The probe-lit frame's ABI without a GPU (include/mcpt.h: mcpt_lit_opts, mcpt_probe_volume, mcpt_lit_outputs, mcpt_lit_info,
mcpt_render_probe_lit): struct sizes and the export, every refusal the library makes before it reads the scene or touches a device (the
handle is not a scene and not mapped memory), and the checks of HipScene.render_probe_lit that raise before the library is called."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = b"mcpt_render_probe_lit"


def test_struct_sizes_header_and_export(hip):
    assert C.sizeof(hip.LitOpts) == 32 and C.sizeof(hip.ProbeVolume) == 40 and C.sizeof(hip.LitOutputs) == 32 and C.sizeof(hip.LitInfo) == 32
    assert hip.LitOpts.seed.offset == 12 and hip.LitOpts.reserved.offset == 16 and hip.LitInfo.samples.offset == 8 and hip.LitInfo.ms_total.offset == 24
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "} mcpt_lit_opts;            /* 32 bytes */" in h and "int mcpt_render_probe_lit(" in h
    assert "mcpt_render_probe_lit" in hip.EXPORTS and hasattr(hip.lib(), "mcpt_render_probe_lit")


def grid_struct(hip, origin=(0, 0, 0), spacing=(1, 1, 1), dims=(2, 2, 2), reserved=(0, 0, 0)):
    return hip.ProbeGrid((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*dims), (C.c_int32 * 3)(*reserved))


def visibility(hip, normal_bias=0.0, backface_max=0.25, reserved=(0, 0)):
    return hip.ProbeVisibility(normal_bias, backface_max, (C.c_int32 * 2)(*reserved))


def opts(hip, aov_spp=1, specular_depth=0, centre=1, seed=1, reserved=(0, 0, 0, 0)):
    return hip.LitOpts(aov_spp, specular_depth, centre, seed, (C.c_int32 * 4)(*reserved))


def test_refusals_before_any_device_work(pkg, hip):
    L = hip.lib()
    fake = C.c_void_p(0x1000)  # never read: every refusal below comes first
    A = 0x2000                 # "device" addresses, never dereferenced either
    cam = np.ascontiguousarray(pkg.scenes.make_camera(4, 3, 40, (0, 0, -5), (0, 0, 0)))
    pcam = cam.ctypes.data_as(C.c_void_p)
    info = hip.LitInfo(7, 7, 7, 7, 7.0)

    def call(sc=fake, cam=pcam, o=None, grid=None, sh=A, moments=A, counts=A, vis="default", lit=A, position=None, reserved=(None, None), vol="default",
             out="default"):
        o = opts(hip) if o is None else o
        g = grid_struct(hip) if grid is None else grid
        v = visibility(hip) if vis == "default" else vis
        pv = hip.ProbeVolume(C.pointer(g) if g != "null" else None, sh, moments, counts, C.pointer(v) if v is not None else None)
        po = hip.LitOutputs(lit, position, (C.c_void_p * 2)(*reserved))
        return L.mcpt_render_probe_lit(sc, cam, None if o == "null" else C.byref(o), None if vol is None else C.byref(pv),
                                       None if out is None else C.byref(po), None, C.byref(info))

    cases = [(dict(sc=None), b"null"), (dict(cam=None), b"null"), (dict(o="null"), b"null"), (dict(vol=None), b"null"), (dict(out=None), b"null"),
             (dict(lit=None), b"null"), (dict(grid="null"), b"null grid"), (dict(sh=None), b"null"),
             (dict(o=opts(hip, aov_spp=-1, centre=0)), b"aov_spp"), (dict(o=opts(hip, aov_spp=65537, centre=0)), b"aov_spp"),
             (dict(o=opts(hip, specular_depth=-1)), b"specular_depth"), (dict(o=opts(hip, specular_depth=9)), b"specular_depth"),
             (dict(o=opts(hip, centre=2)), b"centre"), (dict(o=opts(hip, centre=-1)), b"centre"),
             (dict(o=opts(hip, aov_spp=2, centre=1)), b"centre"), (dict(o=opts(hip, aov_spp=65536, centre=1)), b"centre"),
             (dict(reserved=(A, None)), b"reserved"), (dict(reserved=(None, A)), b"reserved"),
             (dict(moments=None), b"all null"), (dict(counts=None), b"all null"), (dict(vis=None), b"all null"),
             (dict(moments=None, counts=None), b"all null"), (dict(moments=None, vis=None), b"all null"), (dict(counts=None, vis=None), b"all null"),
             (dict(grid=grid_struct(hip, dims=(0, 2, 2))), b"dims"), (dict(grid=grid_struct(hip, spacing=(1, 0, 1))), b"spacing"),
             (dict(grid=grid_struct(hip, spacing=(1, float("inf"), 1))), b"spacing"), (dict(grid=grid_struct(hip, reserved=(0, 1, 0))), b"reserved"),
             (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 2))), b"192"), (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 8))), b"27"),
             (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 8)), moments=None, counts=None, vis=None), b"27"),
             (dict(vis=visibility(hip, normal_bias=-0.1)), b"normal_bias"), (dict(vis=visibility(hip, normal_bias=float("nan"))), b"normal_bias"),
             (dict(vis=visibility(hip, backface_max=-1.0)), b"backface_max"), (dict(vis=visibility(hip, backface_max=float("inf"))), b"backface_max"),
             (dict(vis=visibility(hip, reserved=(0, 3))), b"reserved")]
    for k in range(4):
        r = [0, 0, 0, 0]
        r[k] = 1
        cases.append((dict(o=opts(hip, reserved=r)), b"reserved"))
    for kw, word in cases:
        rc = call(**kw)
        assert rc == 1 and NAME in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert info.chunks == 0 and info.samples == 0 and info.lookups == 0 and info.ms_total == 0.0
    bad = cam.copy()
    bad["width"] = 0
    assert call(cam=bad.ctypes.data_as(C.c_void_p)) == 1 and b"width" in L.mcpt_last_error()
    # a null info is fine as far as the refusals go
    g, o = grid_struct(hip), opts(hip, centre=3)
    pv = hip.ProbeVolume(C.pointer(g), A, None, None, None)
    po = hip.LitOutputs(A, None, (C.c_void_p * 2)(None, None))
    assert L.mcpt_render_probe_lit(fake, pcam, C.byref(o), C.byref(pv), C.byref(po), None, None) == 1 and b"centre" in L.mcpt_last_error()


# ---------------------------------------------------------------- Python-side validation before the library
class NoLibraryScene:
    """render_probe_lit of HipScene over a handle that must never be used."""

    def __init__(self, pkg, hip, W=6, H=4):
        self.h, self.L, self.device = None, None, 0
        self.sd = type("SD", (), {"camera": pkg.scenes.make_camera(W, H, 40, (0, 0, -5), (0, 0, 0))})()
        self.render_probe_lit = hip.HipScene.render_probe_lit.__get__(self)


def test_bad_inputs_raise_before_the_library(pkg, hip):
    W, H = 6, 4
    hs = NoLibraryScene(pkg, hip, W, H)
    dims, m = (3, 2, 4), 24
    good = dict(sh=FakeDevice((m, 27)), moments=FakeDevice((m, 192)), counts=FakeDevice((m, 2), "<i4"))
    out = {"lit": FakeDevice((H, W, 3)), "position": FakeDevice((H, W, 3))}

    def call(origin=(0, 0, 0), spacing=(1, 1, 1), dims=dims, out=out, position=True, **kw):
        a = dict(good)
        a.update(kw)
        return hs.render_probe_lit(origin, spacing, dims, a.pop("sh"), out=out, position=position, **a)

    for kw in (dict(dims=(0, 2, 4)), dict(dims=(3, 2)), dict(spacing=(1, 0, 1)), dict(dims=(2 ** 12, 2 ** 12, 2)), dict(sh=FakeDevice((m - 1, 27))),
               dict(sh=FakeDevice((m, 27), "<f8")), dict(sh=np.zeros((m, 27), f32)), dict(moments=None), dict(counts=None),
               dict(moments=FakeDevice((m, 64))), dict(counts=FakeDevice((m, 2))), dict(counts=FakeDevice((m, 3), "<i4")),
               dict(normal_bias=-1.0), dict(normal_bias=float("nan")), dict(backface_max=-0.5), dict(backface_max=float("inf")),
               dict(aov_spp=-1), dict(aov_spp=65537), dict(specular_depth=-1), dict(specular_depth=9), dict(centre=True, aov_spp=2),
               dict(out={"position": out["position"]}), dict(out={"lit": out["lit"]}), dict(out=dict(out, lit=FakeDevice((H, W, 4)))),
               dict(out=dict(out, lit=FakeDevice((W, H, 3)))), dict(out=dict(out, lit=FakeDevice((H, W, 3), "<f8"))),
               dict(out=dict(out, position=FakeDevice((H * W, 3)))), dict(out=dict(out, lit=np.zeros((H, W, 3), f32))),
               dict(out=dict(out, lit=FakeDevice((H, W, 3), strides=(4, 4 * H, 4 * H * W))))):
        with pytest.raises(ValueError):
            call(**kw)
    cam = np.array(hs.sd.camera, copy=True)
    cam["height"] = 0
    with pytest.raises(ValueError):
        call(camera=cam)
    # good inputs get as far as the library, which this scene does not have: with and without visibility, with and without position
    for kw in (dict(), dict(moments=None, counts=None), dict(position=False, out={"lit": out["lit"]}), dict(centre=True, aov_spp=1),
               dict(aov_spp=3, specular_depth=8, seed=2 ** 32 + 5)):
        with pytest.raises(AttributeError):
            call(**kw)
