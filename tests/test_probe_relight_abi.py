"""mcpt_probe_volume_relight's ABI without a GPU (include/mcpt.h: mcpt_probe_relight_opts, mcpt_probe_relight_outputs): struct sizes and
the exports, every refusal the library makes before it reads the scene or touches a device (the handle is not a scene and not mapped
memory, as in tests/test_probe_lit_abi.py; the one refusal that needs the scene's device, a pointer that is not its memory, is made on a
live handle in tests/test_gpu_probe_relight.py), and the checks of HipScene.relight_probe_volume that raise before the library is called."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402
from test_probe_lit_abi import grid_struct, visibility  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = b"mcpt_probe_volume_relight"
PROBES = 8  # grid_struct's default 2 x 2 x 2


def test_struct_sizes_header_and_export(hip):
    assert C.sizeof(hip.ProbeRelightOpts) == 64 and C.sizeof(hip.ProbeRelightOutputs) == 32
    assert hip.ProbeRelightOpts.hysteresis.offset == 12 and hip.ProbeRelightOpts.max_distance.offset == 28 and hip.ProbeRelightOpts.reserved.offset == 32
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "} mcpt_probe_relight_opts;    /* 64 bytes */" in h and "} mcpt_probe_relight_outputs; /* 32 bytes */" in h
    assert "int mcpt_probe_volume_relight(" in h and "int mcpt_probe_relight_fold_host(" in h
    for name in ("mcpt_probe_volume_relight", "mcpt_probe_relight_fold_host"):
        assert name in hip.EXPORTS and hasattr(hip.lib(), name)


def opts(hip, seed=1, spp=4, sample_offset=0, hysteresis=0.5, indirect_only=0, direct_samples=0, direct_seed=1, max_distance=0.0, reserved=(0,) * 8):
    return hip.ProbeRelightOpts(seed, spp, sample_offset, hysteresis, indirect_only, direct_samples, direct_seed, max_distance, (C.c_int32 * 8)(*reserved))


def test_refusals_before_any_device_work(hip):
    L = hip.lib()
    fake = C.c_void_p(0x1000)  # never read: every refusal below comes first
    A, B = 0x200000, 0x400000  # "device" addresses of the volume and of the outputs, never dereferenced either
    SH, MOM, CNT = PROBES * 27 * 4, PROBES * 192 * 4, PROBES * 2 * 4
    info = hip.QueryInfo(7, 7, 7, (C.c_int32 * 4)(7, 7, 7, 7))

    def call(sc=fake, o=None, grid=None, sh=A, moments=A + 0x10000, counts=A + 0x20000, vis="default", out_sh=B, out_moments=None, out_counts=None,
             reserved=None, vol="default", out="default"):
        o = opts(hip) if o is None else o
        g = grid_struct(hip) if grid is None else grid
        v = visibility(hip) if vis == "default" else vis
        pv = hip.ProbeVolume(C.pointer(g) if g != "null" else None, sh, moments, counts, C.pointer(v) if v is not None else None)
        po = hip.ProbeRelightOutputs(out_sh, out_moments, out_counts, reserved)
        return L.mcpt_probe_volume_relight(sc, None if vol is None else C.byref(pv), None if o == "null" else C.byref(o), None if out is None else C.byref(po),
                                           None, C.byref(info))

    depth = dict(out_moments=B + 0x10000, out_counts=B + 0x20000)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(sc=None), b"null"), (dict(vol=None), b"null"), (dict(o="null"), b"null"), (dict(out=None), b"null"), (dict(out_sh=None), b"null sh"),
             (dict(sh=None), b"null sh"), (dict(grid="null"), b"null grid"),
             # the grid, visibility and all-or-none refusals of mcpt_render_probe_lit
             (dict(moments=None), b"all null"), (dict(counts=None), b"all null"), (dict(vis=None), b"all null"),
             (dict(moments=None, counts=None), b"all null"), (dict(moments=None, vis=None), b"all null"), (dict(counts=None, vis=None), b"all null"),
             (dict(grid=grid_struct(hip, dims=(0, 2, 2))), b"dims"), (dict(grid=grid_struct(hip, spacing=(1, 0, 1))), b"spacing"),
             (dict(grid=grid_struct(hip, spacing=(1, inf, 1))), b"spacing"), (dict(grid=grid_struct(hip, reserved=(0, 1, 0))), b"reserved"),
             (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 2))), b"192"), (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 8))), b"27"),
             (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 8)), moments=None, counts=None, vis=None), b"27"),
             (dict(grid=grid_struct(hip, dims=(2 ** 12, 2 ** 12, 2)), moments=None, counts=None, vis=None, **depth, o=opts(hip, spp=1, max_distance=1.0)), b"192"),
             (dict(vis=visibility(hip, normal_bias=-0.1)), b"normal_bias"), (dict(vis=visibility(hip, normal_bias=nan)), b"normal_bias"),
             (dict(vis=visibility(hip, backface_max=-1.0)), b"backface_max"), (dict(vis=visibility(hip, backface_max=inf)), b"backface_max"),
             (dict(vis=visibility(hip, reserved=(0, 3))), b"reserved"),
             # the options
             (dict(o=opts(hip, spp=0)), b"spp"), (dict(o=opts(hip, spp=-1)), b"spp"), (dict(o=opts(hip, sample_offset=-1)), b"sample_offset"),
             (dict(o=opts(hip, spp=2, sample_offset=2 ** 31 - 2)), b"sample_offset"),
             (dict(o=opts(hip, hysteresis=1.0)), b"hysteresis"), (dict(o=opts(hip, hysteresis=-0.001)), b"hysteresis"),
             (dict(o=opts(hip, hysteresis=nan)), b"hysteresis"), (dict(o=opts(hip, hysteresis=inf)), b"hysteresis"),
             (dict(o=opts(hip, indirect_only=2)), b"indirect_only"), (dict(o=opts(hip, indirect_only=-1)), b"indirect_only"),
             (dict(o=opts(hip, direct_samples=-1)), b"direct_samples"), (dict(o=opts(hip, direct_samples=4097)), b"direct_samples"),
             (dict(o=opts(hip, max_distance=0.0), **depth), b"max_distance"), (dict(o=opts(hip, max_distance=-1.0), **depth), b"max_distance"),
             (dict(o=opts(hip, max_distance=nan), **depth), b"max_distance"), (dict(o=opts(hip, max_distance=inf), **depth), b"max_distance"),
             # the outputs
             (dict(out_moments=B + 0x10000), b"both null"), (dict(out_counts=B + 0x20000), b"both null"), (dict(reserved=A), b"reserved"),
             # the staging indices
             (dict(o=opts(hip, spp=2 ** 28 + 1)), b"probes * spp"), (dict(o=opts(hip, spp=2 ** 20, direct_samples=257)), b"direct_samples"),
             # overlaps: the same buffer, the output starting inside the volume's, and ending inside it
             (dict(out_sh=A), b"overlap"), (dict(out_sh=A + SH - 4), b"overlap"), (dict(out_sh=A - SH + 4), b"overlap"),
             (dict(o=opts(hip, max_distance=1.0), out_moments=A + 0x10000 + MOM - 4, out_counts=B + 0x20000), b"overlap"),
             (dict(o=opts(hip, max_distance=1.0), out_moments=B + 0x10000, out_counts=A + 0x20000 - CNT + 4), b"overlap")]
    for k in range(8):
        r = [0] * 8
        r[k] = 1
        cases.append((dict(o=opts(hip, reserved=r)), b"reserved"))
    for kw, word in cases:
        rc = call(**kw)
        assert rc == 1 and NAME in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert info.launches == 7 and info.grew == 7 and info.staged_bytes == 7 and list(info.reserved) == [7] * 4  # untouched
    # a null info is fine as far as the refusals go
    g, o = grid_struct(hip), opts(hip, hysteresis=2.0)
    pv = hip.ProbeVolume(C.pointer(g), A, None, None, None)
    po = hip.ProbeRelightOutputs(B, None, None, None)
    assert L.mcpt_probe_volume_relight(fake, C.byref(pv), C.byref(o), C.byref(po), None, None) == 1 and b"hysteresis" in L.mcpt_last_error()


# ---------------------------------------------------------------- Python-side validation before the library
class NoLibraryScene:
    """relight_probe_volume of HipScene over a handle that must never be used."""

    def __init__(self, hip):
        self.h, self.L, self.device = None, None, 0
        self.relight_probe_volume = hip.HipScene.relight_probe_volume.__get__(self)


def test_bad_inputs_raise_before_the_library(hip):
    hs = NoLibraryScene(hip)
    dims, m = (3, 2, 4), 24
    good = dict(sh=FakeDevice((m, 27)), moments=FakeDevice((m, 192)), counts=FakeDevice((m, 2), "<i4"))
    out = {"sh": FakeDevice((m, 27))}
    dout = dict(out, moments=FakeDevice((m, 192)), counts=FakeDevice((m, 2), "<i4"))

    def call(origin=(0, 0, 0), spacing=(1, 1, 1), dims=dims, out=out, **kw):
        a = dict(good)
        a.update(kw)
        return hs.relight_probe_volume(origin, spacing, dims, a.pop("sh"), out=out, **a)

    for kw in (dict(dims=(0, 2, 4)), dict(dims=(3, 2)), dict(spacing=(1, 0, 1)), dict(dims=(2 ** 12, 2 ** 12, 2)), dict(sh=FakeDevice((m - 1, 27))),
               dict(sh=FakeDevice((m, 27), "<f8")), dict(sh=np.zeros((m, 27), f32)), dict(moments=None), dict(counts=None),
               dict(moments=FakeDevice((m, 64))), dict(counts=FakeDevice((m, 2))), dict(normal_bias=-1.0), dict(backface_max=float("inf")),
               dict(spp=0), dict(sample_offset=-1), dict(spp=2, sample_offset=2 ** 31 - 2), dict(hysteresis=1.0), dict(hysteresis=-0.5),
               dict(hysteresis=float("nan")), dict(direct_samples=-1), dict(direct_samples=4097), dict(spp=2 ** 27), dict(spp=2 ** 16, direct_samples=4096),
               dict(depth=True, out=dout), dict(depth=True, max_distance=0.0, out=dout), dict(depth=True, max_distance=float("inf"), out=dout),
               dict(depth=True, max_distance=2.0), dict(depth=True, max_distance=2.0, out=dict(dout, counts=FakeDevice((m, 2)))),
               dict(out={}), dict(out={"sh": FakeDevice((m, 28))}), dict(out={"sh": np.zeros((m, 27), f32)})):
        with pytest.raises(ValueError):
            call(**kw)
    # good inputs get as far as the library, which this scene does not have
    for kw in (dict(), dict(moments=None, counts=None), dict(depth=True, max_distance=2.0, out=dout), dict(spp=130, hysteresis=0.75, direct_samples=3,
                                                                                                            indirect_only=True, seed=2 ** 32 + 5)):
        with pytest.raises(AttributeError):
            call(**kw)
