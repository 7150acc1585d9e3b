"""The ABI of the sampled direct term, the indirect-only probes and the lit frames with direct light without a GPU (include/mcpt.h:
mcpt_direct_opts, mcpt_probe_opts, mcpt_lit_direct_opts, mcpt_lit_direct_info and the calls that take them): struct sizes, offsets and
exports, every refusal the four new device entry points make before they read the scene or touch a device (the handle is not a scene
and not mapped memory), the host forms' refusals, and the checks of the HipScene methods that raise before the library is called."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402
from test_probe_lit_abi import grid_struct, opts, visibility  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a scene handle that is never read: every refusal below comes first
A = 0x2000     # "device" addresses, never dereferenced either


def test_struct_sizes_offsets_header_and_exports(hip):
    assert C.sizeof(hip.DirectOpts) == 32 and C.sizeof(hip.ProbeOpts) == 32 and C.sizeof(hip.LitDirectOpts) == 32 and C.sizeof(hip.LitDirectInfo) == 32
    assert (hip.DirectOpts.seed.offset, hip.DirectOpts.n_samples.offset, hip.DirectOpts.key_sample.offset, hip.DirectOpts.reserved.offset) == (0, 4, 8, 12)
    assert (hip.ProbeOpts.indirect_only.offset, hip.ProbeOpts.reserved.offset) == (0, 4)
    assert (hip.LitDirectOpts.n_samples.offset, hip.LitDirectOpts.seed.offset, hip.LitDirectOpts.reserved.offset) == (0, 4, 8)
    assert (hip.LitDirectInfo.light_samples.offset, hip.LitDirectInfo.shadow_rays.offset, hip.LitDirectInfo.pieces.offset, hip.LitDirectInfo.reserved.offset) == (0, 8, 16, 20)
    assert hip.DIRECT_MAX_SAMPLES == 4096 and hip.DIRECT_STREAM == 5
    # the existing structs keep their layout
    assert C.sizeof(hip.LitOpts) == 32 and C.sizeof(hip.QueryInfo) == 32 and C.sizeof(hip.ProbeOutputs) == 32
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = hip.lib()
    for s in ("mcpt_query_direct", "mcpt_query_probes_ex", "mcpt_bake_probe_grid_ex", "mcpt_bake_probe_volume_ex", "mcpt_render_probe_lit_direct",
              "mcpt_rng_uniforms_host", "mcpt_direct_samples_host", "mcpt_direct_fold_host"):
        assert s in hip.EXPORTS and hasattr(L, s) and ("int %s(" % s) in h
    for s in ("} mcpt_direct_opts;      /* 32 bytes */", "} mcpt_probe_opts;         /* 32 bytes */", "} mcpt_lit_direct_opts;  /* 32 bytes */",
              "} mcpt_lit_direct_info;  /* 32 bytes */"):
        assert s in h
    assert not [s for s in hip.EXPORTS if s.startswith("mcpt_group_") and ("direct" in s or "probe" in s)]  # no group forms


def dopts(hip, seed=1, n_samples=4, key_sample=0, reserved=(0,) * 5):
    return hip.DirectOpts(seed, n_samples, key_sample, (C.c_int32 * 5)(*reserved))


def test_query_direct_refuses_before_any_device_work(hip):
    L = hip.lib()
    info = hip.QueryInfo(7, 7, 7)

    def call(sc=FAKE, o=None, n=8, p=A, nr=A, out=A):
        o = dopts(hip) if o is None else o
        return L.mcpt_query_direct(sc, None if o == "null" else C.byref(o), n, p, nr, out, None, C.byref(info))

    cases = [(dict(sc=None), b"null scene"), (dict(o="null"), b"null opts"), (dict(o=dopts(hip, n_samples=0)), b"n_samples"),
             (dict(o=dopts(hip, n_samples=-1)), b"n_samples"), (dict(o=dopts(hip, n_samples=4097)), b"n_samples"), (dict(n=-1), b"n must"),
             (dict(n=(2 ** 31 - 1) // 4 + 1), b"n must"), (dict(n=2 ** 31 - 1, o=dopts(hip, n_samples=2)), b"n must"), (dict(p=None), b"null points"),
             (dict(nr=None), b"null points"), (dict(out=None), b"null points")]
    for k in range(5):
        r = [0] * 5
        r[k] = 1
        cases.append((dict(o=dopts(hip, reserved=r)), b"reserved"))
    for kw, word in cases:
        rc = call(**kw)
        assert rc == 1 and b"mcpt_query_direct" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert (info.launches, info.grew, info.staged_bytes) == (7, 7, 7)  # untouched
    assert L.mcpt_query_direct(None, C.byref(dopts(hip)), 0, None, None, None, None, None) == 1  # (a null scene even with n == 0)


def test_probe_ex_calls_refuse_before_any_device_work(hip):
    L = hip.lib()
    prm = hip.Params(spp=4, rr_rate=0.8, n_dir_sample=1, nranks=1)
    g, dp = grid_struct(hip), hip.ProbeDepthParams(1, 4, 0, 0, 2.0, (C.c_int32 * 3)(0, 0, 0))
    outs = hip.ProbeOutputs(A, None, None, None)

    def popts(indirect_only=1, reserved=(0,) * 7):
        return hip.ProbeOpts(indirect_only, (C.c_int32 * 7)(*reserved))

    bad = [(popts(indirect_only=2), b"indirect_only"), (popts(indirect_only=-1), b"indirect_only")]
    for k in range(7):
        r = [0] * 7
        r[k] = 5
        bad.append((popts(reserved=r), b"reserved"))
    for o, word in bad:
        assert L.mcpt_query_probes_ex(FAKE, C.byref(prm), 4, A, C.byref(outs), None, None, C.byref(o)) == 1
        assert b"mcpt_query_probes" in L.mcpt_last_error() and word in L.mcpt_last_error()
        assert L.mcpt_bake_probe_grid_ex(FAKE, C.byref(g), C.byref(prm), A, None, None, C.byref(o)) == 1
        assert b"mcpt_bake_probe_grid" in L.mcpt_last_error() and word in L.mcpt_last_error()
        assert L.mcpt_bake_probe_volume_ex(FAKE, C.byref(g), C.byref(prm), C.byref(dp), A, A, A, None, None, C.byref(o)) == 1
        assert b"mcpt_bake_probe_volume" in L.mcpt_last_error() and word in L.mcpt_last_error()
    # with good options the plain calls' refusals are made, in the plain calls' names
    for o in (None, C.byref(popts()), C.byref(popts(indirect_only=0))):
        assert L.mcpt_query_probes_ex(None, C.byref(prm), 4, A, C.byref(outs), None, None, o) == 1 and b"mcpt_query_probes: null scene" in L.mcpt_last_error()
        assert L.mcpt_query_probes_ex(FAKE, None, 4, A, C.byref(outs), None, None, o) == 1 and b"null params" in L.mcpt_last_error()
        assert L.mcpt_query_probes_ex(FAKE, C.byref(prm), -1, A, C.byref(outs), None, None, o) == 1 and b"n must" in L.mcpt_last_error()
        assert L.mcpt_bake_probe_grid_ex(None, C.byref(g), C.byref(prm), A, None, None, o) == 1 and b"null scene" in L.mcpt_last_error()
        assert L.mcpt_bake_probe_grid_ex(FAKE, C.byref(grid_struct(hip, dims=(0, 1, 1))), C.byref(prm), A, None, None, o) == 1 and b"dims" in L.mcpt_last_error()
        assert L.mcpt_bake_probe_grid_ex(FAKE, C.byref(g), C.byref(prm), None, None, None, o) == 1 and b"null" in L.mcpt_last_error()
        assert L.mcpt_bake_probe_volume_ex(None, C.byref(g), C.byref(prm), C.byref(dp), A, A, A, None, None, o) == 1 and b"null scene" in L.mcpt_last_error()
        assert L.mcpt_bake_probe_volume_ex(FAKE, C.byref(g), C.byref(prm), None, A, A, A, None, None, o) == 1 and b"depth params" in L.mcpt_last_error()
        assert L.mcpt_bake_probe_volume_ex(FAKE, C.byref(g), C.byref(prm), C.byref(dp), A, None, A, None, None, o) == 1 and b"null" in L.mcpt_last_error()


def test_lit_direct_refuses_before_any_device_work(pkg, hip):
    L = hip.lib()
    NAME = b"mcpt_render_probe_lit_direct"
    cam = np.ascontiguousarray(pkg.scenes.make_camera(4, 3, 40, (0, 0, -5), (0, 0, 0)))
    pcam = cam.ctypes.data_as(C.c_void_p)
    info, dinfo = hip.LitInfo(7, 7, 7, 7, 7.0), hip.LitDirectInfo(7, 7, 7)

    def ldo(n_samples=4, seed=1, reserved=(0,) * 6):
        return hip.LitDirectOpts(n_samples, seed, (C.c_int32 * 6)(*reserved))

    def call(sc=FAKE, cam=pcam, o=None, d=None, sh=A, moments=A, counts=A, vis="default", lit=A, reserved=(None, None), vol="default", out="default", grid=None):
        o = opts(hip) if o is None else o
        d = ldo() if d is None else d
        g = grid_struct(hip) if grid is None else grid
        v = visibility(hip) if vis == "default" else vis
        pv = hip.ProbeVolume(C.pointer(g), sh, moments, counts, C.pointer(v) if v is not None else None)
        po = hip.LitOutputs(lit, None, (C.c_void_p * 2)(*reserved))
        return L.mcpt_render_probe_lit_direct(sc, cam, None if o == "null" else C.byref(o), None if d == "null" else C.byref(d),
                                              None if vol is None else C.byref(pv), None if out is None else C.byref(po), None, C.byref(info), C.byref(dinfo))

    cases = [(dict(d=ldo(n_samples=-1)), b"n_samples"), (dict(d=ldo(n_samples=4097)), b"n_samples"),
             # the plain call's refusals, with direct on, off (n_samples 0) and null
             (dict(sc=None), b"null"), (dict(cam=None), b"null"), (dict(o="null"), b"null"), (dict(vol=None), b"null"), (dict(out=None), b"null"),
             (dict(lit=None), b"null"), (dict(sh=None), b"null"), (dict(o=opts(hip, aov_spp=-1, centre=0)), b"aov_spp"),
             (dict(o=opts(hip, specular_depth=9)), b"specular_depth"), (dict(o=opts(hip, centre=2)), b"centre"), (dict(o=opts(hip, aov_spp=2, centre=1)), b"centre"),
             (dict(reserved=(A, None)), b"reserved"), (dict(moments=None), b"all null"), (dict(vis=None), b"all null"),
             (dict(grid=grid_struct(hip, dims=(0, 2, 2))), b"dims"), (dict(vis=visibility(hip, normal_bias=-0.1)), b"normal_bias"),
             (dict(d=ldo(n_samples=0), o=opts(hip, centre=2)), b"centre"), (dict(d="null", o=opts(hip, centre=2)), b"centre"),
             (dict(d=ldo(n_samples=0), lit=None), b"null")]
    for k in range(6):
        r = [0] * 6
        r[k] = 1
        cases.append((dict(d=ldo(reserved=r)), b"direct: reserved"))
        cases.append((dict(d=ldo(n_samples=0, reserved=r)), b"direct: reserved"))
    for k in range(4):  # tests/test_probe_lit_abi.py pins them for the plain call: nothing of mcpt_lit_opts is repurposed
        r = [0, 0, 0, 0]
        r[k] = 1
        cases.append((dict(o=opts(hip, reserved=r)), b"reserved"))
    for kw, word in cases:
        rc = call(**kw)
        assert rc == 1 and NAME in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, rc, L.mcpt_last_error())
        assert (info.chunks, info.samples, info.lookups, info.ms_total) == (7, 7, 7, 7.0)  # untouched, unlike the plain call's
        assert (dinfo.light_samples, dinfo.shadow_rays, dinfo.pieces) == (7, 7, 7)


def test_host_forms_refuse_bad_arguments(hip):
    L = hip.lib()
    p, nf, rows = np.zeros((2, 3), f32), np.zeros((2, 3), f32), np.zeros((2, 4, 10), f32)
    outs = [np.full(s, -13.5, f32) for s in ((2, 4, 3), (2, 4, 3), (2, 4))] + [np.full((2, 4), 0xAB, np.uint8), np.full((2, 4, 3), -13.5, f32)]
    P = [a.ctypes.data for a in [p, nf, rows] + outs]

    def samples(n=2, N=4, ptrs=P):
        return L.mcpt_direct_samples_host(n, N, *ptrs)

    for kw, word in [(dict(N=0), b"N must"), (dict(N=-1), b"N must"), (dict(N=4097), b"N must"), (dict(n=-1), b"n must"), (dict(n=2 ** 31 // 4 + 1), b"n must")] + \
                    [(dict(ptrs=P[:k] + [None] + P[k + 1:]), b"null") for k in range(8)]:
        rc = samples(**kw)
        assert rc == 1 and b"mcpt_direct_samples_host" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, L.mcpt_last_error())
    assert all((o == f32(-13.5)).all() for o in outs[:3] + outs[4:]) and (outs[3] == 0xAB).all()  # nothing was written
    assert samples(n=0, ptrs=[None] * 8) == 0
    c, v, out = np.zeros((2, 4, 3), f32), np.ones((2, 4), np.uint8), np.full((2, 3), -13.5, f32)
    Q = [c.ctypes.data, v.ctypes.data, out.ctypes.data]
    for kw, word in [(dict(N=0), b"N must"), (dict(N=4097), b"N must"), (dict(n=-1), b"n must"), (dict(n=2 ** 31 // 4 + 1), b"n must")] + \
                    [(dict(ptrs=Q[:k] + [None] + Q[k + 1:]), b"null") for k in range(3)]:
        a = dict(n=2, N=4, ptrs=Q)
        a.update(kw)
        rc = L.mcpt_direct_fold_host(a["n"], a["N"], *a["ptrs"])
        assert rc == 1 and b"mcpt_direct_fold_host" in L.mcpt_last_error() and word in L.mcpt_last_error(), (kw, L.mcpt_last_error())
    assert (out == f32(-13.5)).all()
    assert L.mcpt_direct_fold_host(0, 4, None, None, None) == 0
    u = np.zeros(4, np.uint32)
    o4 = np.full((4, 4), -13.5, f32)
    U = [u.ctypes.data] * 4 + [o4.ctypes.data]
    assert L.mcpt_rng_uniforms_host(1, 2, -1, *U) == 1 and b"mcpt_rng_uniforms_host" in L.mcpt_last_error()
    for k in range(5):
        assert L.mcpt_rng_uniforms_host(1, 2, 4, *(U[:k] + [None] + U[k + 1:])) == 1
    assert (o4 == f32(-13.5)).all() and L.mcpt_rng_uniforms_host(1, 2, 0, None, None, None, None, None) == 0
    # the Python forms
    z = np.zeros
    for bad in (lambda: hip.direct_samples(z((2, 4), f32), z((2, 4), f32), z((2, 4, 10), f32)), lambda: hip.direct_samples(z((2, 3)), z((3, 3)), z((2, 4, 10))),
                lambda: hip.direct_samples(z((2, 3)), z((2, 3)), z((2, 4, 9))), lambda: hip.direct_samples(z((2, 3)), z((2, 3)), z((2, 0, 10))),
                lambda: hip.direct_fold(z((2, 4)), z((2, 4))), lambda: hip.direct_fold(z((2, 4, 3)), z((2, 3))), lambda: hip.direct_fold(z((2, 0, 3)), z((2, 0)))):
        with pytest.raises(ValueError):
            bad()


class NoLibraryScene:
    """The new and extended methods of HipScene over a handle that must never be used."""

    def __init__(self, pkg, hip):
        self.h, self.L, self.device = None, None, 0
        self.sd = type("SD", (), {"camera": pkg.scenes.make_camera(6, 4, 40, (0, 0, -5), (0, 0, 0))})()
        for m in ("query_direct", "render_probe_lit"):
            setattr(self, m, getattr(hip.HipScene, m).__get__(self))


def test_bad_inputs_raise_before_the_library(pkg, hip):
    hs, n = NoLibraryScene(pkg, hip), 8
    p, nr, out = FakeDevice((n, 3)), FakeDevice((n, 3)), FakeDevice((n, 3))
    for kw in (dict(points=FakeDevice((n, 4))), dict(points=np.zeros((n, 3), f32)), dict(normals=FakeDevice((n + 1, 3))), dict(normals=FakeDevice((n, 3), "<f8")),
               dict(out=FakeDevice((n, 4))), dict(out=FakeDevice((n, 3), strides=(4, 4 * n))), dict(out=None), dict(n_samples=0), dict(n_samples=-2),
               dict(n_samples=4097)):
        a = dict(points=p, normals=nr, n_samples=4, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            hs.query_direct(a["points"], a["normals"], a["n_samples"], out=a["out"])
    with pytest.raises(AttributeError):  # good inputs get as far as the library (which this scene does not have)
        hs.query_direct(p, nr, 4, seed=2 ** 32 + 3, key_sample=7, out=out)
    m = 24
    lit = {"lit": FakeDevice((4, 6, 3))}
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            hs.render_probe_lit((0, 0, 0), (1, 1, 1), (3, 2, 4), FakeDevice((m, 27)), out=lit, direct_samples=bad)
    for good in (0, 1, 4096):
        with pytest.raises(AttributeError):
            hs.render_probe_lit((0, 0, 0), (1, 1, 1), (3, 2, 4), FakeDevice((m, 27)), out=lit, direct_samples=good, direct_seed=9)
