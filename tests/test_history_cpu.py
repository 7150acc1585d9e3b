"""History rejection without a GPU (include/mcpt.h: mcpt_history_opts, mcpt_temporal_accumulate_ex, mcpt_sequence_create_ex,
mcpt_sequence_flags): the ctypes struct has the header's layout; both entry points refuse invalid arguments before they touch a device; the
host compilation of tp::accumulate_pixel_ex (tests/native/history_driver.cpp, g++ -ffp-contract=off) follows the rule of include/mcpt.h --
a numpy float32 restatement in the header's order, bit for bit in colour, variance, length and flags; with both switches off it is the
host build of tp::accumulate_pixel; and a stand-alone program (tests/native/history_main.cpp) runs the same header under AddressSanitizer
and UBSan.  tests/test_gpu_history.py checks that the kernel gives the host build's bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_temporal_cpu import SHAPES, bits_equal, blend_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "final-project-monte-carlo-path-tracer-with-microfacet-bsdf_amd", "csrc")
f32 = np.float32

HIST_KINDS = ["fractional", "crease", "nan_normals", "nan_colour_neighbours", "constant_neighbourhood", "far_outside", "inside", "max_history_1"]
SWITCHES = [(1, 1), (1, 0), (0, 1)]  # (normal_test, color_clamp)


def build_driver(out_dir):
    """tests/native/history_driver.cpp as a shared library (ctypes handle)."""
    so = os.path.join(str(out_dir), "libhistory_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "history_driver.cpp"), "-o", so])
    L = C.CDLL(so)
    L.tp_accumulate_ex.restype = C.c_int
    L.tp_accumulate_ex.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 15
    L.tp_accumulate_plain.restype = C.c_int
    L.tp_accumulate_plain.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 11
    L.tp_resolve_history.restype = C.c_int
    L.tp_resolve_history.argtypes = [C.c_void_p] * 3
    return L


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("hist_cpu"))


def _arr(x):
    return None if x is None else np.ascontiguousarray(x, f32)


def _p(x):
    return None if x is None else x.ctypes.data


def host_accumulate_ex(L, hip, color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal, history=None, **opts):
    """The host build of accumulate_pixel_ex over a frame: (out, out_variance, out_len, flags).  history: keywords of hip.history_opts."""
    a = [_arr(x) for x in (color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal)]
    H, W = a[0].shape[:2]
    out, out_var, out_len, flags = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32), np.full((H, W), 255, np.uint8)
    o, ho = hip.temporal_opts(**opts), hip.history_opts(**(history or {}))
    rc = L.tp_accumulate_ex(W, H, *[_p(x) for x in a], C.addressof(o), C.addressof(ho), out.ctypes.data, out_var.ctypes.data, out_len.ctypes.data,
                            flags.ctypes.data)
    assert rc == 0
    return out, out_var, out_len, flags


def host_accumulate_plain(L, hip, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, **opts):
    a = [_arr(x) for x in (color, variance, motion, prev_color, prev_variance, prev_depth, prev_len)]
    H, W = a[0].shape[:2]
    out, out_var, out_len = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
    o = hip.temporal_opts(**opts)
    assert L.tp_accumulate_plain(W, H, *[x.ctypes.data for x in a], C.addressof(o), out.ctypes.data, out_var.ctypes.data, out_len.ctypes.data) == 0
    return out, out_var, out_len


def numpy_accumulate_ex(color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal, normal_test=0, color_clamp=0,
                        normal_min=0.0, clamp_k=0.0, max_history=0, depth_tol=0.0):
    """mcpt_temporal_accumulate_ex as include/mcpt.h states it, in float32, every operation in the header's order.
    Returns (out, out_variance, out_len, flags)."""
    mh = f32(max_history if max_history else 32)
    tol = f32(depth_tol if depth_tol else 0.02)
    nmn = f32(normal_min if normal_min else 0.9)
    ck = f32(clamp_k if clamp_k else 1.0)
    c = np.ascontiguousarray(color, f32)
    vc = np.ascontiguousarray(variance, f32)
    H, W = c.shape[:2]
    jj, ii = np.mgrid[0:H, 0:W]
    dx, dy, zp, valid = (np.ascontiguousarray(motion[..., k], f32) for k in range(4))
    go = (valid > 0) & np.isfinite(c).all(-1)
    with np.errstate(all="ignore"):
        fx, fy = ii.astype(f32) + dx, jj.astype(f32) + dy
        x0, y0 = np.floor(fx), np.floor(fy)
        a, b = fx - x0, fy - y0
        wx, wy = [f32(1) - a, a], [f32(1) - b, b]
        ztol = tol * zp
        sw, sv, nmin = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
        s = np.zeros((H, W, 3), f32)
        used = np.zeros((H, W), bool)
        nskip = np.zeros((H, W), bool)
        for t in range(4):
            w = wx[t & 1] * wy[t >> 1]
            tx, ty = x0 + f32(t & 1), y0 + f32(t >> 1)
            use = go & (w != 0) & (tx >= 0) & (tx < f32(W)) & (ty >= 0) & (ty < f32(H))
            xi, yi = np.where(use, tx, 0).astype(np.int64), np.where(use, ty, 0).astype(np.int64)
            n, p, pv = prev_len[yi, xi].astype(f32), prev_color[yi, xi].astype(f32), prev_variance[yi, xi].astype(f32)
            dz = prev_depth[yi, xi].astype(f32) - zp
            use = use & (n > 0) & np.isfinite(p).all(-1) & (np.abs(dz) <= ztol)
            if normal_test:
                pn, nn = prev_normal[yi, xi].astype(f32), np.ascontiguousarray(normal, f32)
                d = pn[..., 0] * nn[..., 0] + (pn[..., 1] * nn[..., 1] + pn[..., 2] * nn[..., 2])
                assert d.dtype == f32
                keep = d >= nmn  # (false for a NaN)
                nskip |= use & ~keep
                use = use & keep
            sw = np.where(use, sw + w, sw)
            s = np.where(use[..., None], s + w[..., None] * p, s)
            sv = np.where(use, sv + (w * w) * pv, sv)
            nmin = np.where(use & (~used | (n < nmin)), n, nmin)
            used = used | use
        hist = s / sw[..., None]
        clamped = np.zeros((H, W), bool)
        if color_clamp:
            fin = np.isfinite(c).all(-1)
            s1, s2, cnt = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
            for ddy in (-1, 0, 1):
                for ddx in (-1, 0, 1):
                    y, x = jj + ddy, ii + ddx
                    ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
                    yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
                    ok = ok & fin[yc, xc]
                    q = c[yc, xc]
                    s1 = np.where(ok[..., None], s1 + q, s1)
                    s2 = np.where(ok[..., None], s2 + q * q, s2)
                    cnt = np.where(ok, cnt + f32(1), cnt)
            fn = cnt[..., None]
            mu = s1 / fn
            v = s2 / fn - mu * mu
            var_n = np.where(v > 0, v, f32(0))
            sd = np.sqrt(var_n)
            ksd = ck * sd
            lo, hi = mu - ksd, mu + ksd
            t1 = np.where(hist < lo, lo, hist)
            hist2 = np.where(t1 > hi, hi, t1)
            assert hist2.dtype == f32
            clamped = (hist2 != hist).any(-1)
            hist = hist2
        n1 = nmin + f32(1)
        N = np.where(n1 < mh, n1, mh)
        k = f32(1) / N
        out = hist + (c - hist) * k[..., None]
        hv = sv / (sw * sw)
        omk = f32(1) - k
        var = (omk * omk) * hv + (k * k) * vc
        var = np.where(~clamped & np.isfinite(hv) & (hv >= 0), var, vc)
    assert out.dtype == f32 and var.dtype == f32 and N.dtype == f32
    flags = (np.where(used & nskip, 1, 0) | np.where(used & clamped, 2, 0)).astype(np.uint8)
    return np.where(used[..., None], out, c), np.where(used, var, vc), np.where(used, N, f32(1)), flags


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def history_case(kind, H, W):
    """(color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal), temporal opts, history values:
    a blend case of test_temporal_cpu (a gentle depth plane, so neighbouring taps pass the depth test) with variances and normals."""
    base = {"fractional": "fractional", "max_history_1": "max_history_1"}.get(kind, "half")
    (color, motion, prev_color, prev_depth, prev_len), opts = blend_case(base, H, W)
    rng = np.random.default_rng(9000 + H * 100 + W + HIST_KINDS.index(kind))
    variance = (rng.random((H, W)) * 0.1).astype(f32)
    prev_variance = (rng.random((H, W)) * 0.05).astype(f32)
    # folded normals: means of unit vectors, a little shorter than 1; the previous frame's differ enough to straddle normal_min 0.9
    normal = (_unit(rng.standard_normal((H, W, 3)) + np.array([0, 0, 3.0])) * (1 - 0.05 * rng.random((H, W, 1)))).astype(f32)
    prev_normal = (_unit(normal + 0.35 * rng.standard_normal((H, W, 3))) * (1 - 0.05 * rng.random((H, W, 1)))).astype(f32)
    values = {}
    if kind == "fractional":
        opts = dict(max_history=8)  # (the default depth tolerance: most taps reach the normal test)
        values = dict(normal_min=0.95, clamp_k=1.5)
    elif kind == "crease":
        # two faces that meet at nearly the same depth: the history's left half faces +x, its right half +z; every pixel reads the four
        # taps (i, j) .. (i + 1, j + 1), so the pixels left of the edge see one tap column of the other face
        motion[..., 0:2] = 0.5
        motion[..., 3] = 1
        face = np.where((np.arange(W) < (W + 1) // 2)[None, :, None], np.array([1, 0, 0], f32), np.array([0, 0, 1], f32))
        normal = np.broadcast_to(face, (H, W, 3)).astype(f32).copy()
        prev_normal = normal.copy()
    elif kind == "nan_normals":
        motion[..., 3] = 1
        normal[rng.random((H, W)) < 0.2, 1] = np.nan
        prev_normal[rng.random((H, W)) < 0.2, 2] = np.nan
        prev_normal[0, 0, 0] = np.nan
        normal[H - 1, W - 1, 0] = np.inf
    elif kind == "nan_colour_neighbours":
        motion[..., 3] = 1
        bad = rng.random((H, W)) < 0.25
        color[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
        color[0, W - 1, 0] = np.inf
    elif kind == "constant_neighbourhood":
        motion[..., 0:2] = 0  # (one tap of weight 1: hist is the history's own pixel)
        motion[..., 3] = 1
        color[...] = np.array([0.25, 0.5, 0.75], f32)  # sd == 0: lo == hi == mu, all exact
        prev_color[::2, ::2] = color[::2, ::2]         # a history that already sits on mu is left alone
    elif kind == "far_outside":
        motion[..., 3] = 1
        color[H // 2, W // 2, 2] = 1.5  # (finite, so that a 1 x 1 frame takes history)
        prev_color = (prev_color + f32(100)).astype(f32)
    elif kind == "inside":
        # zero motion and history == the new frame: hist is the pixel itself, which lies within sqrt(n - 1) <= sqrt(8) < 3 population
        # standard deviations of the mean of its n <= 9 neighbours (Samuelson's inequality), so clamp_k 3 never moves it
        motion[..., 0:2] = 0
        motion[..., 3] = 1
        color[H // 2, W // 2, 2] = 1.5
        prev_color = color.copy()
        prev_normal = normal.copy()
        values = dict(clamp_k=3.0)
    return (color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal), opts, values


def plain_args(args):
    color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal = args
    return color, variance, motion, prev_color, prev_variance, prev_depth, prev_len


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", HIST_KINDS)
def test_accumulate_ex_host_build_equals_numpy(pkg, hip, driver, kind, shape):
    H, W = shape
    args, opts, values = history_case(kind, H, W)
    color, variance = args[0], args[1]
    plain, plain_var, plain_len = host_accumulate_plain(driver, hip, *plain_args(args), **opts)
    for nt, cc in SWITCHES:
        hist = dict(normal_test=nt, color_clamp=cc, **values)
        got, got_var, got_len, got_flags = host_accumulate_ex(driver, hip, *args, history=hist, **opts)
        want, want_var, want_len, want_flags = numpy_accumulate_ex(*args, **hist, **opts)
        assert bits_equal(got, want), (nt, cc, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert bits_equal(got_var, want_var), (nt, cc)
        assert bits_equal(got_len, want_len), (nt, cc)
        assert np.array_equal(got_flags, want_flags), (nt, cc)
        assert (got_flags & ~np.uint8((1 if nt else 0) | (2 if cc else 0)) == 0).all()
        if not nt:
            assert bits_equal(got_len, plain_len)  # the clamp does not change which taps are used, nor the length
            same = (got_flags & 2) == 0
            assert bits_equal(got[same], plain[same]) and bits_equal(got_var[same], plain_var[same])
            moved = ~same
            assert bits_equal(got_var[moved], variance[moved])  # a clamped history: this frame's own variance
        big = H * W > 4
        if kind == "crease" and nt and big:
            # the last column of the left face drops the tap column of the other face, and no other pixel drops a tap (a pixel whose own
            # colour is not finite takes no history and has no flag)
            expect = np.zeros((H, W), np.uint8)
            expect[:, (W + 1) // 2 - 1] = 1
            expect[~np.isfinite(color).all(-1)] = 0
            assert np.array_equal(got_flags & 1, expect) and expect.any()
        if kind == "nan_normals" and nt:
            ok = np.isfinite(color).all(-1)
            assert np.isfinite(got[ok]).all()
            assert (got_len[np.isnan(args[3]).any(-1)] == 1).all()  # a pixel whose own normal is NaN takes no history
        if kind == "nan_colour_neighbours" and cc:
            ok = np.isfinite(color).all(-1)
            assert np.isfinite(got[ok]).all()  # a NaN neighbour never reaches a finite pixel
        if kind == "constant_neighbourhood" and cc and not nt:
            had = plain_len > 1
            assert had.any() and bits_equal(got[had], color[had])  # the history is clamped onto mu == the colour, and c + (c - c) k == c
            on_mu = np.zeros((H, W), bool)
            on_mu[::2, ::2] = True
            assert ((got_flags[on_mu] & 2) == 0).all() and ((got_flags[had & ~on_mu] & 2) == 2).all()
        if kind == "far_outside" and cc and not nt:
            had = plain_len > 1
            assert ((got_flags[had] & 2) == 2).all() and bits_equal(got_var[had], variance[had])
            if big:
                assert had.any()
        if kind == "inside" and cc:
            assert ((got_flags & 2) == 0).all()
            if not nt:
                assert bits_equal(got, plain) and bits_equal(got_var, plain_var) and (got_len > 1).any()
        if kind == "max_history_1":
            assert (got_len == 1).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", HIST_KINDS)
def test_switches_off_is_accumulate_pixel(pkg, hip, driver, kind, shape):
    """Both switches 0: the outputs of the host build of accumulate_pixel bit for bit, flags 0, and the normal arrays are not read (null)."""
    H, W = shape
    args, opts, values = history_case(kind, H, W)
    plain, plain_var, plain_len = host_accumulate_plain(driver, hip, *plain_args(args), **opts)
    for normals in (True, False):
        a = list(args)
        if not normals:
            a[3] = a[8] = None
        got, got_var, got_len, flags = host_accumulate_ex(driver, hip, *a, history=values, **opts)
        assert bits_equal(got, plain) and bits_equal(got_var, plain_var) and bits_equal(got_len, plain_len)
        assert (flags == 0).all()


def test_struct_layout_and_header(hip):
    T = hip.HistoryOpts
    assert C.sizeof(T) == 32
    assert (T.normal_test.offset, T.color_clamp.offset, T.normal_min.offset, T.clamp_k.offset, T.reserved.offset) == (0, 4, 8, 12, 16)
    assert T.reserved.size == 16
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    for text in ("} mcpt_history_opts;     /* 32 bytes; a zeroed struct switches both tests off */", "int32_t normal_test; /* 0 off, 1 on */",
                 "int32_t color_clamp; /* 0 off, 1 on */", "float normal_min;    /* 0 => 0.9; otherwise in (0, 1] */", "int32_t reserved[4]; /* must be 0 */",
                 "d = pn.x*n.x + (pn.y*n.y + pn.z*n.z)", "var = max(s2/n - mu*mu, 0)", "hist' = min(max(hist, lo), hi)"):
        assert text in h, text
    body = h[h.index("int32_t normal_test;"):h.index("} mcpt_history_opts;")]
    order = [ln.split(";")[0].split()[-1].split("[")[0] for ln in body.splitlines() if ";" in ln]
    assert order == [k for k, _ in T._fields_], order
    for name in ("mcpt_temporal_accumulate_ex", "mcpt_sequence_create_ex", "mcpt_sequence_flags"):
        assert name in h and name in hip.EXPORTS
    o = hip.history_opts()
    assert bytes(o) == bytes(32)  # the default is the zeroed struct: both tests off


def test_history_option_ranges_host_build(pkg, hip, driver):
    sw, val = (C.c_int * 2)(), (C.c_float * 2)()

    def rc(o):
        return driver.tp_resolve_history(C.addressof(o), C.addressof(sw), C.addressof(val))

    assert rc(hip.history_opts()) == 0 and tuple(sw) == (0, 0) and val[0] == f32(0.9)
    default_k = val[1]
    assert default_k in (1.0, 1.5, 2.0, 3.0)  # one of the issue's candidates
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "float clamp_k;       /* 0 => %g; otherwise > 0 and finite */" % default_k in h
    assert rc(hip.history_opts(True, True, 1.0, 0.25)) == 0 and tuple(sw) == (1, 1) and tuple(val) == (1.0, 0.25)
    for kw in (dict(normal_min=1e-6), dict(normal_min=1.0), dict(clamp_k=1e-6), dict(clamp_k=3e38)):
        assert rc(hip.history_opts(**kw)) == 0, kw
    for kw in BAD_HISTORY:
        assert rc(hip.history_opts(**kw)) == 1, kw
    for k in range(4):
        o = hip.history_opts(True, True)
        o.reserved[k] = 1
        assert rc(o) == 1, k


BAD_HISTORY = (dict(normal_test=2), dict(normal_test=-1), dict(color_clamp=2), dict(color_clamp=-1), dict(normal_min=-0.5), dict(normal_min=1.5),
               dict(normal_min=float("nan")), dict(normal_min=float("inf")), dict(clamp_k=-1.0), dict(clamp_k=float("nan")), dict(clamp_k=float("inf")),
               # ... also while the switch the value belongs to is off, and while the other one is on
               dict(color_clamp=1, normal_min=2.0), dict(normal_test=1, clamp_k=-2.0))


def test_argument_checks_come_before_any_device_call(pkg, hip):
    """Every refusal below happens before the library touches a device (there is none on the machines that run this test) and before it
    reads the scene: the handle is not a scene and not mapped memory."""
    L = hip.lib()
    fake = C.c_void_p(0x1000)
    W, H = 4, 3
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    col, var, mo, nrm = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W, 4), f32), np.zeros((H, W, 3), f32)
    pc, pv, z, n, pn = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    out, out_var, out_len, flags = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), np.uint8)
    ok, on = hip.temporal_opts(), hip.history_opts(True, True)
    # 0 scene, 1 W, 2 H, 3 color, 4 variance, 5 motion, 6 normal, 7 prev_color, 8 prev_variance, 9 prev_depth, 10 prev_len, 11 prev_normal,
    # 12 opts, 13 history_opts, 14 out_color, 15 out_variance, 16 out_len, 17 out_flags
    full = [fake, W, H, p(col), p(var), p(mo), p(nrm), p(pc), p(pv), p(z), p(n), p(pn), C.byref(ok), C.byref(on), p(out), p(out_var), p(out_len), p(flags)]
    acc = L.mcpt_temporal_accumulate_ex
    # every case mcpt_temporal_accumulate refuses: a null pointer (the flags alone may be null, which gets as far as the scene), ...
    for k in (0, 3, 4, 5, 7, 8, 9, 10, 12, 13, 14, 15, 16):
        args = list(full)
        args[k] = None
        assert acc(*args) == 1, k
        assert b"mcpt_temporal_accumulate_ex" in L.mcpt_last_error()
    # ... normal_test on with a null normal array (either one), also with the clamp off
    for k in (6, 11):
        for o in (on, hip.history_opts(True, False)):
            args = list(full)
            args[k], args[13] = None, C.byref(o)
            assert acc(*args) == 1, k
    # ... a bad frame size, out-of-range temporal options, their reserved words
    for w, h in ((0, H), (W, 0), (-1, H), (1 << 15, 1 << 15)):
        args = list(full)
        args[1], args[2] = w, h
        assert acc(*args) == 1, (w, h)
    for kw in (dict(max_history=-1), dict(max_history=4097), dict(depth_tol=-1.0), dict(depth_tol=float("nan"))):
        args = list(full)
        o = hip.temporal_opts(**kw)
        args[12] = C.byref(o)
        assert acc(*args) == 1, kw
    for k in range(6):
        o = hip.temporal_opts()
        o.reserved[k] = 7
        args = list(full)
        args[12] = C.byref(o)
        assert acc(*args) == 1, k
    # the history options
    for kw in BAD_HISTORY:
        args = list(full)
        o = hip.history_opts(**kw)
        args[13] = C.byref(o)
        assert acc(*args) == 1, kw
        assert b"mcpt_temporal_accumulate_ex" in L.mcpt_last_error()
    for k in range(4):
        for o in (hip.history_opts(True, True), hip.history_opts()):
            o.reserved[k] = 1
            args = list(full)
            args[13] = C.byref(o)
            assert acc(*args) == 1, k

    # mcpt_sequence_create_ex: every refusal of mcpt_sequence_create, and the history options
    h = C.c_void_p()

    def create(o, ho=on, scene=fake, w=W, hh=H, out=h):
        return L.mcpt_sequence_create_ex(scene, w, hh, C.byref(o) if o is not None else None, C.byref(ho) if ho is not None else None,
                                         C.byref(out) if out is not None else None)

    good = hip.SequenceOpts(filter=1)
    assert create(good, scene=None) == 1 and b"mcpt_sequence_create" in L.mcpt_last_error()
    assert create(None) == 1 and create(good, out=None) == 1
    assert create(good, ho=None, scene=None) == 1 and create(None, ho=None) == 1
    for w, hh in ((0, H), (W, 0), (-3, H), (1 << 15, 1 << 15)):
        assert create(good, w=w, hh=hh) == 1, (w, hh)
        assert create(good, ho=None, w=w, hh=hh) == 1, (w, hh)

    def bad(**kw):
        o = hip.SequenceOpts(filter=1)
        for key, val in kw.items():
            obj, name = (o.temporal, key[2:]) if key.startswith("t_") else (o.denoise, key[2:]) if key.startswith("d_") else (o, key)
            setattr(obj, name, val)
        return o

    for kw in (dict(t_max_history=-1), dict(t_max_history=4097), dict(t_depth_tol=-0.5), dict(t_depth_tol=float("nan")),
               dict(d_iterations=9), dict(d_iterations=-1), dict(d_sigma_l=-1.0), dict(d_sigma_n=2000.0), dict(d_sigma_z=float("nan")),
               dict(d_specular_depth=9), dict(d_specular_depth=-1), dict(d_aov_spp=-1), dict(d_aov_spp=65537),
               dict(filter=2), dict(filter=-1)):
        assert create(bad(**kw)) == 1, kw
        assert b"mcpt_sequence_create" in L.mcpt_last_error()
    for k in range(7):
        o = hip.SequenceOpts(filter=0)
        o.reserved[k] = 1
        assert create(o) == 1, k
    for k in range(6):
        o = hip.SequenceOpts()
        o.temporal.reserved[k] = 1
        assert create(o) == 1, k
    for k in range(2):
        o = hip.SequenceOpts()
        o.denoise.reserved[k] = 1
        assert create(o) == 1, k
    for kw in BAD_HISTORY:
        assert create(good, ho=hip.history_opts(**kw)) == 1, kw
        assert b"mcpt_sequence_create" in L.mcpt_last_error()
    for k in range(4):
        for ho in (hip.history_opts(True, True), hip.history_opts()):
            ho.reserved[k] = 1
            assert create(good, ho=ho) == 1, k
    assert h.value is None
    assert L.mcpt_sequence_flags(None, p(flags)) == 1 and b"mcpt_sequence_flags" in L.mcpt_last_error()


def _sanitizer_runtime_present(tmp):
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    exe = os.path.join(tmp, "probe")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_sanitizer_program(tmp_path):
    """tests/native/history_main.cpp, a program of its own, under AddressSanitizer and UBSan: the host build of accumulate_pixel_ex over the
    three shapes on exactly-sized heap arrays, with huge, infinite and NaN motions.  Nothing is loaded into this process."""
    tmp = str(tmp_path)
    if not _sanitizer_runtime_present(tmp):
        pytest.skip("g++ cannot link an AddressSanitizer / UBSan program here")
    exe = os.path.join(tmp, "history_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "history_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 13, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
