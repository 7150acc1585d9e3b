"""The light-probe rule without a GPU (include/mcpt.h: mcpt_sh_basis_host, mcpt_sh_irradiance_host, mcpt_probe_grid_points_host,
mcpt_probe_shade_host): csrc/mcpt_sh.h compiled for the CPU against the closed forms and against the numpy float32 restatements of
tests/probe_cases.py, bit for bit; the refusals that need no device; and the checks of HipScene.query_probes / probe_shade /
bake_probe_grid that raise before the library is called."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_cases as pc  # noqa: E402
from ray_query_cases import FakeDevice  # noqa: E402

f32, f64 = np.float32, np.float64


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def assert_bits(got, want, what=""):
    bad = ~pc.same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


# ---------------------------------------------------------------- basis
def test_basis_against_the_closed_forms(hip):
    """Each Y_j is a float constant times at most two factors and one difference: at most five float operations on terms no larger than
    the largest term t of the expression (|c|, |c x y|, 3 |c| z z, |c|, ...), each rounding within half an ulp of t, the constant's own
    rounding another half: 4 ulp(t) bounds the error against float64 of the float inputs."""
    d = np.concatenate([unit(np.random.default_rng(1), 400), np.eye(3, dtype=f32), -np.eye(3, dtype=f32)])
    Y = hip.sh_basis(d)
    assert Y.shape == (406, 9) and Y.dtype == f32
    assert_bits(Y, pc.basis(d), "host against the restatement")
    want = pc.basis_f64(d)
    x, y, z = (np.abs(d[:, k].astype(f64)) for k in range(3))
    c1, c2, c20, c22 = np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi)), np.sqrt(5 / (16 * np.pi)), np.sqrt(15 / (16 * np.pi))
    term = np.stack([np.full(len(d), np.sqrt(1 / (4 * np.pi))), c1 * y, c1 * z, c1 * x, c2 * np.maximum(x, x * y), c2 * np.maximum(y, y * z),
                     c20 * np.maximum(3 * z * z, 1.0), c2 * np.maximum(x, x * z), c22 * np.maximum(x * x, y * y)], axis=1)
    ulp = np.spacing(np.maximum(term, np.finfo(f32).tiny).astype(f32)).astype(f64)
    err = np.abs(Y.astype(f64) - want) / ulp
    print("\n[probes] basis: largest error %.2f ulp of the largest term" % err.max())
    assert err.max() <= 4.0
    # the literals of the header are the float roundings of the closed forms
    assert Y[0, 0] == pc.K0 and hip.sh_basis([[0, 1, 0]])[0, 1] == pc.K1 and hip.sh_basis([[0, 0, 1]])[0, 6] == f32(pc.K20 * f32(2))


def test_basis_is_orthonormal(hip):
    """Gauss-Legendre in z (24 nodes) times uniform phi (48): exact for the degree-4 products; summed in float64 over the float outputs."""
    zs, wz = np.polynomial.legendre.leggauss(24)
    phi = (np.arange(48) + 0.5) * (2 * np.pi / 48)
    z, p = np.meshgrid(zs, phi, indexing="ij")
    r = np.sqrt(1 - z * z)
    d = np.stack([r * np.cos(p), r * np.sin(p), z], axis=-1).reshape(-1, 3)
    w = (wz[:, None] * np.full((1, 48), 2 * np.pi / 48)).reshape(-1)
    Y = hip.sh_basis(d.astype(f32)).astype(f64)
    gram = (Y * w[:, None]).T @ Y
    print("\n[probes] |gram - I| max %.3g" % np.abs(gram - np.eye(9)).max())
    assert np.abs(gram - np.eye(9)).max() <= 1e-5


# ---------------------------------------------------------------- irradiance
def test_irradiance_of_a_linear_field(hip):
    """L(w) = a + b w_z: L[0] = a sqrt(4 pi), L[2] = b sqrt(4 pi / 3) per channel; E / pi = a + (2/3) b n_z."""
    rng = np.random.default_rng(2)
    n = np.concatenate([unit(rng, 200), np.eye(3, dtype=f32), -np.eye(3, dtype=f32)])
    a, b = np.array([1.0, 0.5, 2.0]), np.array([0.3, -0.2, 0.9])
    L = np.zeros(27, f32)
    L[0:3] = a * np.sqrt(4 * np.pi)
    L[6:9] = b * np.sqrt(4 * np.pi / 3)
    got = hip.sh_irradiance(L, n)
    want = a[None, :] + (2.0 / 3.0) * b[None, :] * n[:, 2:3].astype(f64)
    rel = np.abs(got - want) / np.abs(want)
    print("\n[probes] irradiance of a + b w_z: relative error %.3g" % rel.max())
    assert rel.max() <= 1e-5
    assert_bits(got, pc.irradiance(np.broadcast_to(L, (len(n), 27)), n), "against the restatement")
    Lr = rng.normal(size=(len(n), 27)).astype(f32)
    assert_bits(hip.sh_irradiance(Lr, n), pc.irradiance(Lr, n), "random coefficients")
    assert (hip.sh_irradiance(Lr, n) < 0).any()  # not clamped at zero


# ---------------------------------------------------------------- grid lookup
def lookup_points(rng, origin, spacing, dims, n):
    origin, spacing, dims = np.asarray(origin, f64), np.asarray(spacing, f64), np.asarray(dims)
    ext = spacing * (dims - 1)
    inside = origin + rng.uniform(0, 1, (n, 3)) * ext
    outside = origin + rng.uniform(-0.7, 1.7, (n, 3)) * np.maximum(ext, spacing)
    face = inside.copy()
    face[:, 0] = origin[0] + ext[0] * rng.integers(0, 2, n)
    at = pc.grid_points(origin, spacing, dims)
    return np.concatenate([inside, outside, face, at]).astype(f32)


# (origins and spacings are dyadic, so origin + i * spacing and (p - origin) / spacing are exact: a grid point IS at its probe in float)
GRIDS = {"3x2x4": ((-1.0, 0.5, 2.0), (0.75, 1.5, 0.5), (3, 2, 4)), "1x1x1": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)),
         "flat y": ((10.0, -3.0, 0.0), (2.0, 1.0, 0.25), (4, 1, 3))}


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grid_lookup_against_the_restatement(hip, name):
    origin, spacing, dims = GRIDS[name]
    rng = np.random.default_rng(3)
    m = dims[0] * dims[1] * dims[2]
    sh = rng.normal(size=(m, 27)).astype(f32)
    p = lookup_points(rng, origin, spacing, dims, 100)
    n = unit(rng, len(p))
    got = hip.probe_shade(origin, spacing, dims, sh, p, n)
    assert_bits(got, pc.shade(origin, spacing, dims, sh, p, n), name)
    pts = hip.probe_grid_points(origin, spacing, dims)
    assert pts.shape == (m, 3)
    assert_bits(pts, pc.grid_points(origin, spacing, dims), name + ", points")
    # a point at a probe returns that probe's own evaluation
    nn = unit(rng, m)
    assert_bits(hip.probe_shade(origin, spacing, dims, sh, pts, nn), hip.sh_irradiance(sh, nn), name + ", at the probes")
    # probe index (iz * ny + iy) * nx + ix
    k = (dims[2] - 1) * dims[1] * dims[0] + (dims[1] - 1) * dims[0] + (dims[0] - 1)
    want_last = np.asarray(origin, f32) + (np.asarray(dims, f32) - f32(1)) * np.asarray(spacing, f32)
    assert k == m - 1 and np.array_equal(pts[k], want_last)


def test_a_linear_field_is_reproduced(hip):
    origin, spacing, dims = GRIDS["3x2x4"]
    rng = np.random.default_rng(4)
    pts = pc.grid_points(origin, spacing, dims).astype(f64)
    A, c = rng.normal(size=(27, 3)), rng.normal(size=27)
    sh = (pts @ A.T + c).astype(f32)
    ext = np.asarray(spacing) * (np.asarray(dims) - 1)
    p = (np.asarray(origin) + rng.uniform(0.02, 0.98, (300, 3)) * ext).astype(f32)
    n = unit(rng, 300)
    got = hip.probe_shade(origin, spacing, dims, sh, p, n).astype(f64)
    want = pc.irradiance((p.astype(f64) @ A.T + c).astype(f32), n).astype(f64)
    scale = np.abs(sh).max()
    print("\n[probes] linear field: largest error %.3g of coefficients up to %.3g" % (np.abs(got - want).max(), scale))
    # 27 blended coefficients, each a sum of 8 products with weights that sum to 1 (about 10 roundings), then the 9-term irradiance sum
    assert np.abs(got - want).max() <= 64 * np.finfo(f32).eps * scale


# ---------------------------------------------------------------- refusals that need no device
def test_struct_sizes_and_exports(hip):
    assert C.sizeof(hip.ProbeGrid) == 48 and C.sizeof(hip.ProbeOutputs) == 32
    for s in ("mcpt_query_probes", "mcpt_probe_rays", "mcpt_probe_shade", "mcpt_bake_probe_grid", "mcpt_sh_basis_host", "mcpt_sh_irradiance_host",
              "mcpt_probe_grid_points_host", "mcpt_probe_shade_host"):
        assert s in hip.EXPORTS


def grid_struct(hip, origin=(0, 0, 0), spacing=(1, 1, 1), dims=(2, 2, 2), reserved=(0, 0, 0)):
    return hip.ProbeGrid((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*dims), (C.c_int32 * 3)(*reserved))


def test_refusals_without_a_device(hip):
    L = hip.lib()
    pts = np.zeros((64, 3), f32)
    sh = np.zeros((8, 27), f32)
    out = np.full((4, 3), -13.5, f32)
    p = n = np.zeros((4, 3), f32)

    def refused(g, word):
        for rc in (L.mcpt_probe_grid_points_host(C.byref(g), pts.ctypes.data), L.mcpt_probe_shade_host(C.byref(g), sh.ctypes.data, 4, p.ctypes.data, n.ctypes.data, out.ctypes.data)):
            assert rc == 1 and word in L.mcpt_last_error(), (rc, L.mcpt_last_error())

    refused(grid_struct(hip, dims=(0, 2, 2)), b"dims")
    refused(grid_struct(hip, dims=(2, -1, 2)), b"dims")
    refused(grid_struct(hip, dims=(2 ** 20, 2 ** 10, 2)), b"dims")
    refused(grid_struct(hip, spacing=(0, 1, 1)), b"spacing")
    refused(grid_struct(hip, spacing=(1, -1, 1)), b"spacing")
    refused(grid_struct(hip, spacing=(1, 1, float("inf"))), b"spacing")
    refused(grid_struct(hip, spacing=(float("nan"), 1, 1)), b"spacing")
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 1
        refused(grid_struct(hip, reserved=r), b"reserved")
    assert (out == f32(-13.5)).all() and not pts.any()  # nothing was written
    g = grid_struct(hip)
    assert L.mcpt_probe_grid_points_host(None, pts.ctypes.data) == 1 and b"null" in L.mcpt_last_error()
    assert L.mcpt_probe_grid_points_host(C.byref(g), None) == 1 and b"null" in L.mcpt_last_error()
    assert L.mcpt_probe_shade_host(C.byref(g), None, 4, p.ctypes.data, n.ctypes.data, out.ctypes.data) == 1 and b"null" in L.mcpt_last_error()
    assert L.mcpt_probe_shade_host(C.byref(g), sh.ctypes.data, 0, None, None, None) == 0  # n == 0: a valid no-op
    assert L.mcpt_sh_basis_host(1, None, None) == 1 and L.mcpt_sh_irradiance_host(1, None, None, None) == 1
    assert L.mcpt_sh_basis_host(0, None, None) == 0
    # the device calls refuse a null scene before anything else
    prm = hip.Params(spp=1, rr_rate=0.8, n_dir_sample=1, nranks=1)
    assert L.mcpt_query_probes(None, C.byref(prm), 1, None, C.byref(hip.ProbeOutputs()), None, None) == 1 and b"mcpt_query_probes: null scene" in L.mcpt_last_error()
    assert L.mcpt_probe_rays(None, 1, 0, None, None, None, None, None) == 1 and b"mcpt_probe_rays" in L.mcpt_last_error()
    assert L.mcpt_probe_shade(None, C.byref(g), None, 0, None, None, None, None) == 1 and b"mcpt_probe_shade: null scene" in L.mcpt_last_error()
    assert L.mcpt_bake_probe_grid(None, C.byref(g), C.byref(prm), None, None, None) == 1 and b"mcpt_bake_probe_grid: null scene" in L.mcpt_last_error()


# ---------------------------------------------------------------- Python-side validation before the library
class NoLibraryScene:
    """The probe methods of HipScene over a handle that must never be used: every case below is refused before the library is called."""

    def __init__(self, hip):
        self.h, self.L, self.sd, self.device = None, None, None, 0
        for m in ("query_probes", "probe_shade", "bake_probe_grid"):
            setattr(self, m, getattr(hip.HipScene, m).__get__(self))

    def params(self, **kw):
        raise AssertionError("the parameters were built: the inputs passed their checks")


def test_bad_probe_inputs_raise_before_the_library(hip):
    hs, n = NoLibraryScene(hip), 8
    good = {"sh": FakeDevice((n, 27)), "radiance": FakeDevice((n, 3)), "variance": FakeDevice((n, 3))}
    for bad in (FakeDevice((n, 3), "<f8"), FakeDevice((n * 3,)), FakeDevice((n, 4)), FakeDevice((n, 3), strides=(4, 4 * n)), [[0.0] * 3] * n,
                np.zeros((n, 3), f32)):
        with pytest.raises(ValueError):
            hs.query_probes(bad, out=good)
    o = FakeDevice((n, 3))
    with pytest.raises(ValueError):  # no torch tensors: the outputs must be supplied
        hs.query_probes(o)
    with pytest.raises(ValueError):  # a wanted output without a buffer
        hs.query_probes(o, variance=True, out={"sh": good["sh"], "radiance": good["radiance"]})
    for name, bad in (("sh", FakeDevice((n, 9))), ("sh", FakeDevice((n * 27,))), ("sh", FakeDevice((n, 27), "<f8")), ("sh", FakeDevice((n - 1, 27))),
                      ("radiance", FakeDevice((n, 27))), ("variance", FakeDevice((n, 3), strides=(4, 4 * n)))):
        out = dict(good)
        out[name] = bad
        with pytest.raises(ValueError):
            hs.query_probes(o, variance=True, out=out)
    with pytest.raises(AssertionError):  # and good inputs do get as far as the parameters
        hs.query_probes(o, variance=True, out=good)


def test_bad_grids_and_lookups_raise_before_the_library(hip):
    hs, n = NoLibraryScene(hip), 8
    dims, m = (3, 2, 4), 24
    sh, p, nr, out = FakeDevice((m, 27)), FakeDevice((n, 3)), FakeDevice((n, 3)), FakeDevice((n, 3))
    for bad_dims in ((0, 2, 4), (3, 2), (3, 2.5, 4), (2 ** 20, 2 ** 10, 2)):
        with pytest.raises(ValueError):
            hs.probe_shade((0, 0, 0), (1, 1, 1), bad_dims, sh, p, nr, out=out)
        with pytest.raises(ValueError):
            hs.bake_probe_grid((0, 0, 0), (1, 1, 1), bad_dims, out=sh)
        with pytest.raises(ValueError):
            hip.probe_grid_points((0, 0, 0), (1, 1, 1), bad_dims)
    for bad_spacing in ((0, 1, 1), (1, -1, 1), (1, 1, float("inf")), (float("nan"), 1, 1)):
        with pytest.raises(ValueError):
            hs.probe_shade((0, 0, 0), bad_spacing, dims, sh, p, nr, out=out)
        with pytest.raises(ValueError):
            hs.bake_probe_grid((0, 0, 0), bad_spacing, dims, out=sh)
    for kw in (dict(sh=FakeDevice((m - 1, 27))), dict(sh=FakeDevice((m, 27), "<f8")), dict(p=FakeDevice((n, 4))), dict(nr=FakeDevice((n + 1, 3))),
               dict(out=FakeDevice((n, 3), strides=(4, 4 * n))), dict(out=None), dict(p=np.zeros((n, 3), f32))):
        a = dict(sh=sh, p=p, nr=nr, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            hs.probe_shade((0, 0, 0), (1, 1, 1), dims, a["sh"], a["p"], a["nr"], out=a["out"])
    with pytest.raises(ValueError):
        hs.bake_probe_grid((0, 0, 0), (1, 1, 1), dims, out=FakeDevice((m, 9)))
    with pytest.raises(AttributeError):  # good buffers get as far as the library (which this scene does not have)
        hs.probe_shade((0, 0, 0), (1, 1, 1), dims, sh, p, nr, out=out)
    with pytest.raises(AssertionError):  # ... and as far as the parameters
        hs.bake_probe_grid((0, 0, 0), (1, 1, 1), dims, out=sh)
