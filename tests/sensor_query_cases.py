"""Shared by tests/test_gpu_sensor_query.py and tests/sensor_query_torch_child.py (include/mcpt.h: mcpt_query_radiance, mcpt_sensor_rays):
the expectation of a sensor's radiance -- the numpy float32 fold of mcpt_cast_rays in sample order -- the float64 evaluation of the
variance, the float64 restatement of the hemisphere rule, and the rays the tests ask about."""
import numpy as np

from ray_query_cases import GUARD, DevBuf

f32, f64 = np.float32, np.float64
SENTINEL = -13.5   # what the guarded output buffers hold before a call
K_EPS = f32(1e-4)  # EPSILON, csrc/mcpt_internal.h
K_PI = f32(3.141592653589793)


def same_bits(a, b):
    """Equal bits where the expectation is finite, NaN where it is NaN."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def cast_values(hs, o, d, spp, sample_offset=0, **kw):
    """v[i, k, c] = cast_rays of the first ray of (sensor i, sample k) with pixel = i, sample = sample_offset + k, channel = c.
    o, d: (n, 3), one ray for every sample of a sensor, or (n, spp, 3)."""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    n = len(o)
    if o.ndim == 2:
        o, d = np.repeat(o[:, None, :], spp, axis=1), np.repeat(d[:, None, :], spp, axis=1)
    assert o.shape == (n, spp, 3) and d.shape == o.shape
    oo = np.repeat(o.reshape(-1, 3), 3, axis=0)
    dd = np.repeat(d.reshape(-1, 3), 3, axis=0)
    pix = np.repeat(np.arange(n, dtype=np.uint32), spp * 3)
    smp = np.tile(np.repeat(np.arange(spp, dtype=np.uint32) + np.uint32(sample_offset), 3), n)
    ch = np.tile(np.arange(3, dtype=np.int32), n * spp)
    return hs.cast_rays(oo, dd, pix, smp, ch, **kw).reshape(n, spp, 3)


def fold(v, spp_total=None, start=None):
    """acc = start (or 0); for k in sample order: acc += v[:, k] / spp_total, in float32: k_accumulate's arithmetic."""
    n, spp, _ = v.shape
    tot = f32(spp_total if spp_total else spp)
    acc = np.zeros((n, 3), f32) if start is None else np.array(start, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):
            acc = (acc + (v[:, k, :].astype(f32) / tot).astype(f32)).astype(f32)
    return acc


def variance_f64(v):
    """max(s2/n - (s1/n)^2, 0) * n/(n-1) / n in float64, s1 and s2 summed in sample order."""
    n_s, spp, _ = v.shape
    s1, s2 = np.zeros((n_s, 3), f64), np.zeros((n_s, 3), f64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):
            x = v[:, k, :].astype(f64)
            s1 = s1 + x
            s2 = s2 + x * x
        n = f64(spp)
        mean = s1 / n
        diff = s2 / n - mean * mean
        pop = np.where(diff < 0, 0.0, diff)
        return pop * n / (n - 1.0) / n


def outputs(n, variance=False):
    out = {"radiance": DevBuf(shape=(n, 3), dtype=f32, fill=SENTINEL, guard=GUARD)}
    if variance:
        out["variance"] = DevBuf(shape=(n, 3), dtype=f32, fill=SENTINEL, guard=GUARD)
    return out


def radiance(hs, o, d, kind="ray", variance=False, out=None, **kw):
    """query_radiance on the null stream for sensors uploaded here, into guarded buffers -> (radiance, variance or None, Stats) as numpy
    (get() insists that the guards survived)."""
    do, dd = DevBuf(np.ascontiguousarray(o, f32)), DevBuf(np.ascontiguousarray(d, f32))
    out = out or outputs(len(o), variance)
    _, _, st = hs.query_radiance(do, dd, kind=kind, variance=variance, out=out, **kw)
    return out["radiance"].get(), (out["variance"].get() if variance else None), st


def scene_rays(hs, sd, n, seed):
    """The scene_rays recipe of tests/test_gpu_ray_query.py: camera rays plus rays restarted at their hit points in random directions."""
    rng = np.random.default_rng(seed)
    Wd, Hd = int(sd.camera["width"]), int(sd.camera["height"])
    pix = rng.integers(0, Wd * Hd, size=n).astype(np.uint32)
    smp = rng.integers(0, 64, size=n).astype(np.uint32)
    o, d = hs.camera_rays(pix, smp, seed=7)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    p = (o + d * np.where(hit, t, 0.0)[:, None].astype(f32)).astype(f32)
    d2 = rng.normal(size=(n, 3)).astype(f32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    o2 = np.where(hit[:, None], p, o).astype(f32)
    return np.concatenate([o, o2]), np.concatenate([d, d2.astype(f32)])


def rays_805(hs, sd, seed=21):
    """n = 805 = 3 * 256 + 37: a partial block and a partial wave."""
    o, d = scene_rays(hs, sd, 403, seed)
    return np.ascontiguousarray(o[:805]), np.ascontiguousarray(d[:805])


def surface_sensors(hs, sd, n=805, seed=22):
    """Hemisphere sensors: the hit points of camera rays with the hit normals of query_closest, flipped towards the ray.  Rays that miss
    are replaced by later ones that hit."""
    rng = np.random.default_rng(seed)
    Wd, Hd = int(sd.camera["width"]), int(sd.camera["height"])
    m = 4 * n
    pix = rng.integers(0, Wd * Hd, size=m).astype(np.uint32)
    smp = rng.integers(0, 64, size=m).astype(np.uint32)
    o, d = hs.camera_rays(pix, smp, seed=7)
    out = {"prim": DevBuf(shape=(m,), dtype=np.int32, fill=-77, guard=GUARD), "normal": DevBuf(shape=(m, 3), dtype=f32, fill=-10.5, guard=GUARD),
           "point": DevBuf(shape=(m, 3), dtype=f32, fill=-11.5, guard=GUARD)}
    hs.query_closest(DevBuf(o), DevBuf(d), want=("prim", "normal", "point"), out=out)
    prim, nrm, pt = out["prim"].get(), out["normal"].get(), out["point"].get()
    hit = np.flatnonzero(prim >= 0)[:n]
    assert len(hit) == n, "only %d of %d camera rays hit" % (len(hit), m)
    nrm, pt, d = nrm[hit], pt[hit], d[hit]
    facing = (nrm * d).sum(1) < 0
    nrm = np.where(facing[:, None], nrm, -nrm).astype(f32)
    return np.ascontiguousarray(pt, f32), np.ascontiguousarray(nrm, f32)


def hemisphere_pairs(hs, p, nrm, spp, seed, sample_offset=0):
    """sensor_rays for every (sensor, sample) of a call -> (o, d) of shape (n, spp, 3)."""
    n = len(p)
    si = np.repeat(np.arange(n, dtype=np.uint32), spp)
    sm = np.tile(np.arange(spp, dtype=np.uint32) + np.uint32(sample_offset), n)
    o, d = hs.sensor_rays("hemisphere", p, nrm, si, sm, seed=seed)
    return o.reshape(n, spp, 3), d.reshape(n, spp, 3)


def hemisphere_f64(oracle, p, nrm, sensor, sample, seed):
    """The hemisphere rule of include/mcpt.h in float64, the uniforms from oracle.philox: counter (sample, 0, 0, stream 4), key (seed,
    sensor) -> (origins, dirs) float64."""
    p, nrm = np.asarray(p, f32).astype(f64), np.asarray(nrm, f32).astype(f64)
    o, d = np.zeros((len(sensor), 3)), np.zeros((len(sensor), 3))
    for j, (i, k) in enumerate(zip(sensor, sample)):
        w = oracle.philox([int(k), 0, 0, 4], [int(seed), int(i)])
        u0, u1 = (int(w[0]) >> 8) / 16777216.0, (int(w[1]) >> 8) / 16777216.0
        r, phi = np.sqrt(u0), f64(f32(f32(2) * K_PI)) * u1
        local = np.array([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - u0)])
        n = nrm[i]
        if abs(n[0]) > abs(n[1]):  # Material.hpp:95-106
            inv = 1.0 / np.sqrt(n[0] * n[0] + n[2] * n[2])
            T = np.array([-n[2] * inv, 0.0, n[0] * inv])
        else:
            inv = 1.0 / np.sqrt(n[1] * n[1] + n[2] * n[2])
            T = np.array([0.0, n[2] * inv, -n[1] * inv])
        B = np.cross(n, T)
        w3 = T * local[0] + B * local[1] + n * local[2]
        d[j] = w3 / np.linalg.norm(w3)
        o[j] = p[i] + n * f64(K_EPS)
    return o, d
