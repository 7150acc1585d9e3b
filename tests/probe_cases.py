"""Shared by tests/test_probes_cpu.py, tests/test_gpu_probes.py and tests/probe_torch_child.py (include/mcpt.h: mcpt_query_probes,
mcpt_probe_shade and their host forms): numpy float32 restatements of the basis, the projection fold, the irradiance sum and the grid
lookup, every operation rounded to float32 in the written order (no FMA), and the float64 restatement of the whole-sphere first ray."""
import numpy as np

from ray_query_cases import GUARD, DevBuf
from sensor_query_cases import SENTINEL, cast_values, fold, same_bits  # noqa: F401  (re-exported to the tests)

f32, f64 = np.float32, np.float64
# the float roundings of the closed forms; the header states the same literals
K0, K1, K2, K20, K22 = (f32(v) for v in (np.sqrt(1 / (4 * np.pi)), np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi)), np.sqrt(5 / (16 * np.pi)),
                                         np.sqrt(15 / (16 * np.pi))))
K_FOUR_PI = f32(4 * np.pi)
BAND = np.array([1.0] + [2.0 / 3.0] * 3 + [0.25] * 5, f64).astype(f32)
K_PI = f32(3.141592653589793)


def basis(d):
    """Y (n, 9) float32 of unit directions (n, 3): a * b * c is (a * b) * c."""
    d = np.asarray(d, f32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = np.zeros((len(d), 9), f32)
    Y[:, 0] = K0
    Y[:, 1] = K1 * y
    Y[:, 2] = K1 * z
    Y[:, 3] = K1 * x
    Y[:, 4] = (K2 * x) * y
    Y[:, 5] = (K2 * y) * z
    Y[:, 6] = K20 * (((f32(3) * z) * z) - f32(1))
    Y[:, 7] = (K2 * x) * z
    Y[:, 8] = K22 * ((x * x) - (y * y))
    return Y


def basis_f64(d):
    """The closed forms in float64."""
    d = np.asarray(d, f64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c1, c2 = np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi))
    return np.stack([np.full(len(d), np.sqrt(1 / (4 * np.pi))), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z,
                     np.sqrt(5 / (16 * np.pi)) * (3 * z * z - 1), c2 * x * z, np.sqrt(15 / (16 * np.pi)) * (x * x - y * y)], axis=1)


def irradiance(L, n):
    """out[c] = sum over j in index order, from 0, of (A(j) * L[3j + c]) * Y_j(n), float32.  L: (m, 27), n: (m, 3)."""
    L = np.asarray(L, f32).reshape(-1, 9, 3)
    Y = basis(n)
    e = np.zeros((len(L), 3), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(9):
            e = e + (BAND[j] * L[:, j, :]) * Y[:, j:j + 1]
    return e


def sh_fold(v, d, spp_total=None, start=None):
    """sh (n, 27): acc = start or 0; for k in sample order: acc[3j + c] += (v[:, k, c] * (kFourPi * Y_j(d[:, k]))) / spp_total, float32."""
    n, spp, _ = v.shape
    tot = f32(spp_total if spp_total else spp)
    acc = np.zeros((n, 9, 3), f32) if start is None else np.array(start, f32).reshape(n, 9, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):
            w = K_FOUR_PI * basis(d[:, k, :])                              # (n, 9)
            acc = acc + (v[:, k, None, :].astype(f32) * w[:, :, None]) / tot
    return acc.reshape(n, 27)


def grid_axis(p, origin, spacing, dim):
    p = np.asarray(p, f32)
    if dim == 1:
        return np.zeros(len(p), np.int64), np.zeros(len(p), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (p - f32(origin)) / f32(spacing)
    g = np.where(np.isnan(g), f32(0), g)
    g = np.minimum(np.maximum(g, f32(0)), f32(dim - 1)).astype(f32)
    i0 = np.minimum(np.floor(g).astype(np.int64), dim - 2)
    return i0, (g - i0.astype(f32)).astype(f32)


def shade(origin, spacing, dims, sh, points, normals):
    """The grid lookup of include/mcpt.h in float32: corners in the order (dz, dy, dx) = 000 .. 111, w = (wz * wy) * wx."""
    sh = np.asarray(sh, f32).reshape(-1, 27)
    points, normals = np.asarray(points, f32).reshape(-1, 3), np.asarray(normals, f32).reshape(-1, 3)
    nx, ny, nz = (int(v) for v in dims)
    ax = [grid_axis(points[:, a], origin[a], spacing[a], int(dims[a])) for a in range(3)]
    step = [1 if int(dims[a]) > 1 else 0 for a in range(3)]
    b = np.zeros((len(points), 27), f32)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        wx = ax[0][1] if dx else f32(1) - ax[0][1]
        wy = ax[1][1] if dy else f32(1) - ax[1][1]
        wz = ax[2][1] if dz else f32(1) - ax[2][1]
        w = (wz * wy) * wx
        probe = ((ax[2][0] + dz * step[2]) * ny + (ax[1][0] + dy * step[1])) * nx + (ax[0][0] + dx * step[0])
        with np.errstate(invalid="ignore", over="ignore"):
            b = b + w[:, None] * sh[probe]
    return irradiance(b, normals)


def grid_points(origin, spacing, dims):
    nx, ny, nz = (int(v) for v in dims)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)], axis=1).astype(f32)
    return (np.asarray(origin, f32)[None, :] + idx * np.asarray(spacing, f32)[None, :]).astype(f32)


def sphere_f64(oracle, p, sensor, sample, seed):
    """The whole-sphere rule in float64, the uniforms from oracle.philox: counter (sample, 0, 0, stream 4), key (seed, probe)."""
    d = np.zeros((len(sensor), 3))
    two_pi = f64(f32(f32(2) * K_PI))
    for j, (i, k) in enumerate(zip(sensor, sample)):
        w = oracle.philox([int(k), 0, 0, 4], [int(seed), int(i)])
        u0, u1 = (int(w[0]) >> 8) / 16777216.0, (int(w[1]) >> 8) / 16777216.0
        z = 1 - 2 * u0
        r = np.sqrt(max(0.0, 1 - z * z))
        v = np.array([r * np.cos(two_pi * u1), r * np.sin(two_pi * u1), z])
        d[j] = v / np.linalg.norm(v)
    return np.asarray(p, f32).astype(f64)[np.asarray(sensor)], d


def probe_pairs(hs, p, spp, seed, sample_offset=0):
    """probe_rays for every (probe, sample) of a call -> (o, d) of shape (n, spp, 3)."""
    n = len(p)
    si = np.repeat(np.arange(n, dtype=np.uint32), spp)
    sm = np.tile(np.arange(spp, dtype=np.uint32) + np.uint32(sample_offset), n)
    o, d = hs.probe_rays(p, si, sm, seed=seed)
    return o.reshape(n, spp, 3), d.reshape(n, spp, 3)


def probe_points(sd, n=805, seed=31):
    """n points inside the inner 80 % of the bounding box of the scene's triangles."""
    v = np.concatenate([sd.triangles["v0"], sd.triangles["v1"], sd.triangles["v2"]]).astype(f64)
    lo, hi = v.min(0), v.max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.8
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(mid - half, mid + half, (n, 3)), f32)


def probe_outputs(n, radiance=True, variance=False):
    out = {"sh": DevBuf(shape=(n, 27), dtype=f32, fill=SENTINEL, guard=GUARD)}
    if radiance or variance:
        out["radiance"] = DevBuf(shape=(n, 3), dtype=f32, fill=SENTINEL, guard=GUARD)
    if variance:
        out["variance"] = DevBuf(shape=(n, 3), dtype=f32, fill=SENTINEL, guard=GUARD)
    return out


def probes(hs, p, radiance=True, variance=False, out=None, **kw):
    """query_probes on the null stream for points uploaded here, into guarded buffers -> (sh, radiance, variance, Stats) as numpy."""
    dp = DevBuf(np.ascontiguousarray(p, f32))
    out = out or probe_outputs(len(p), radiance, variance)
    _, _, _, st = hs.query_probes(dp, radiance=radiance, variance=variance, out=out, **kw)
    return out["sh"].get(), (out["radiance"].get() if "radiance" in out else None), (out["variance"].get() if variance else None), st
