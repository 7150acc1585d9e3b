"""Shared by tests/test_probe_relight_cpu.py, tests/test_gpu_probe_relight.py and tests/probe_relight_torch_child.py (include/mcpt.h:
mcpt_probe_volume_relight): the numpy float32 restatement of one update of a probe volume from itself, built only from calls that
exist without the feature -- probe_rays, intersect, p = o + d * (float)t in numpy float32, the material table with query_closest's normal
flipped with dot(n, d) > 0, the host forms of the two grid lookups, the host composition of the sampled direct term with the key (probe,
sample_offset + k), cast_rays for the samples that end on the sky or on an emitter -- and the fold and the blend in numpy, every float32
operation rounded in the written order (no FMA).  No tests in here."""
import dataclasses

import numpy as np

import direct_cases as dc
import probe_cases as pc
import probe_depth_cases as pdc
import probe_lit_cases as plc
from material_edit_cases import emits, env_map, with_fields
from ray_query_cases import DevBuf, Rays, closest, scene_extent
from sensor_query_cases import cast_values

f32 = np.float32
ZERO, ONE = f32(0), f32(1)
DIM = (0.7, 0.5, 0.3)  # an emission below 1: emit * |cos| never reaches the clamp, so the cosine is in the value
DIMS = (3, 2, 3)


def fold(v, d):
    """fresh (n, 27): acc = 0; for k in sample order acc[3j + c] += (v[:, k, c] * (kFourPi * Y_j(d[:, k]))) / (float)spp."""
    return pc.sh_fold(np.asarray(v, f32), np.asarray(d, f32))


def basis_negative(d):
    """Where a basis function of the directions d (..., 3) is negative: (n, 9) bool."""
    return pc.basis(np.asarray(d, f32).reshape(-1, 3)) < 0


def blend(h, prev, fresh):
    """hysteresis == 0: fresh; otherwise h * prev + (1.f - h) * fresh, two products and one sum."""
    h = f32(h)
    if h == 0:
        return np.array(fresh, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (h * np.asarray(prev, f32) + (ONE - h) * np.asarray(fresh, f32)).astype(f32)


class HostVolume:
    """A probe volume given by host arrays, uploaded once: what plc.Volume is for a baked one (grid, sh, mom, cnt, nb, bm, dev, kw,
    lookup).  mom and cnt None: the plain lookup alone."""

    def __init__(self, grid, sh, mom=None, cnt=None, normal_bias=0.0, backface_max=0.25):
        self.grid, self.nb, self.bm = grid, normal_bias, backface_max
        self.sh = np.ascontiguousarray(sh, f32)
        self.mom = None if mom is None else np.ascontiguousarray(mom, f32)
        self.cnt = None if cnt is None else np.ascontiguousarray(cnt, np.int32)
        self.dev = {"sh": DevBuf(self.sh)}
        if mom is not None:
            self.dev.update(moments=DevBuf(self.mom), counts=DevBuf(self.cnt, dtype=np.int32))

    kw = plc.Volume.kw
    lookup = plc.Volume.lookup


def dimmed(sd, emission=DIM):
    """The description with every emitter's emission replaced by DIM."""
    mats = sd.materials.copy()
    for i in np.flatnonzero(emits(mats)):
        mats[i] = with_fields(mats[i], emission=emission)
    return dataclasses.replace(sd, materials=mats)


def make_scene(pkg, name):
    """(description, creation keywords, grid, max_distance) of a named Cornell case: a builder's name, "env" (sky through the opening) or
    "dim" (emission below the clamp)."""
    sd = pkg.scenes.cornell_demo(32, 24, 4)
    kw = dict(builder="sah")
    if name == "env":
        sd = dataclasses.replace(sd, env_pixels=env_map(16, 8, seed=3))
    elif name == "dim":
        sd = dimmed(sd)
    elif name == "dark":  # no emitter, and the description's background is black: nothing in the scene gives light
        sd = dimmed(sd, (0.0, 0.0, 0.0))
    else:
        kw = dict(builder=name)
    return sd, kw, plc.scene_grid(sd, DIMS), float(f32(0.3 * scene_extent(sd)))


def samples(hs, hip, sd, vol, visible, spp, seed=1, sample_offset=0, indirect_only=False, direct_samples=0, direct_seed=1):
    """The samples of one update -> dict(d (n, spp, 3), v (n, spp, 3), kind (n, spp), t, prim): v is the value the rule gives sample k of
    probe i, looked up in `vol` (a plc.Volume or a HostVolume)."""
    P = pc.grid_points(*vol.grid)
    n = len(P)
    o3, d3 = pc.probe_pairs(hs, P, spp, seed, sample_offset)
    o, d = np.ascontiguousarray(o3.reshape(-1, 3), f32), np.ascontiguousarray(d3.reshape(-1, 3), f32)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(hit[:, None], o + d * t.astype(f32)[:, None], ZERO).astype(f32)
    pm = plc.prim_materials(sd)
    mi = pm[np.where(hit, prim, 0)]
    emitter = hit & emits(sd.materials)[mi]
    kind = np.where(hit, np.where(emitter, plc.EMITTER, plc.SURFACE), plc.MISS)
    M = sd.materials[mi]
    s = kind == plc.SURFACE
    assert not M["textured"][s].any(), "the material-table albedo holds for untextured materials only"
    conductor = (M["type"] == 0) | (M["type"] == 1)
    alb = np.where(conductor[:, None], M["base_reflectance"], ONE).astype(f32)
    ng = closest(hs, Rays(o, d), want=("normal",))[0]["normal"]
    nf = np.where((plc.dot3(ng, d) > 0)[:, None], -ng, ng).astype(f32)
    v = np.zeros((len(o), 3), f32)
    E = vol.lookup(hip, p[s], nf[s], visible)
    D = np.zeros((int(s.sum()), 3), f32)
    if direct_samples > 0 and s.any():
        probe = np.repeat(np.arange(n), spp)
        key_sample = np.tile(np.arange(spp) + sample_offset, n)
        D = dc.host_direct(hip, hs, p[s], nf[s], direct_samples, seed=direct_seed, pixels=probe[s], key_samples=key_sample[s])[0]
    with np.errstate(over="ignore", invalid="ignore"):
        v[s] = alb[s] * (np.fmax(E, ZERO) + D)
    other = np.flatnonzero(~s)
    if len(other):  # the sky and the emitters: deterministic in cast_rays, whatever the sample
        v[other] = cast_values(hs, o[other], d[other], 1, seed=1)[:, 0, :]
    if indirect_only:
        v[kind == plc.EMITTER] = ZERO
    return dict(d=d3, v=v.reshape(n, spp, 3), kind=kind.reshape(n, spp), t=t, prim=prim, lookups=int(s.sum()))


def restate(hs, hip, sd, vol, visible, spp, hysteresis=0.0, **kw):
    """One update -> (sh (n, 27) float32, the samples)."""
    smp = samples(hs, hip, sd, vol, visible, spp, **kw)
    return blend(hysteresis, vol.sh, fold(smp["v"], smp["d"])), smp


def outputs(m, depth=False):
    out = {"sh": pdc.Guarded((m, 27))}
    if depth:
        out.update(pdc.depth_outputs(m))
    return out


def relight(hs, vol, visible, depth=False, out=None, **kw):
    """relight_probe_volume on the null stream into guarded buffers -> (sh, moments or None, counts or None, info) as numpy."""
    m = vol.grid[2][0] * vol.grid[2][1] * vol.grid[2][2]
    out = out or outputs(m, depth)
    vk = vol.kw(visible)
    _, _, _, info = hs.relight_probe_volume(*vol.grid, vk.pop("sh"), depth=depth, out=out, **vk, **kw)
    return out["sh"].get(), (out["moments"].get() if depth else None), (out["counts"].get() if depth else None), info
