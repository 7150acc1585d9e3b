"""The sky cull's bound and classifier (csrc/mcpt_cull.hip) without a GPU: the bound is host code (mcpt_cull_bound), the classifier is
plain float32 arithmetic over a tree that mcpt_bvh_dump exports, restated in tests/cull_cases.py.
  (a) the lemma behind rho, numerically: no camera ray leaves the rho-tube around its pixel's central ray inside the root box;
  (b) + (c) the restated classification is conservative against the oracle's closest hits for the worst-case rays of every pixel
      (jitter-square corners x lens rim) and for real sample rays, on every case of the shared table whose tree the host builds."""
import math

import numpy as np
import pytest

import cull_cases as cc

f32 = np.float32


def _random_camera(pkg, rng):
    """A camera and a root box: (camera, root_min, root_max)."""
    half = (10.0 ** rng.uniform(-1, 2, 3)).astype(f32)
    centre = rng.uniform(-100, 100, 3).astype(f32)
    lo, hi = (centre - half).astype(f32), (centre + half).astype(f32)
    where = rng.integers(3)
    if where == 0:  # inside
        eye = rng.uniform(lo, hi).astype(f32)
    elif where == 1:  # exactly on a face
        eye = rng.uniform(lo, hi).astype(f32)
        a = rng.integers(3)
        eye[a] = (lo, hi)[rng.integers(2)][a]
    else:  # outside
        v = rng.normal(0, 1, 3)
        eye = (centre + v / np.linalg.norm(v) * np.linalg.norm(half) * 10.0 ** rng.uniform(0.05, 1)).astype(f32)
    target = rng.uniform(lo, hi).astype(f32) if rng.random() < 0.8 else (eye + rng.normal(0, 1, 3) * 50).astype(f32)
    if np.linalg.norm(target - eye) < 1e-3 * np.linalg.norm(half):
        target = (eye + f32([0.3, 0.2, 1.0]) * np.linalg.norm(half)).astype(f32)
    sizes = [(1, 1), (1, int(rng.integers(2, 41))), (int(rng.integers(2, 65)), 1), (64, 40), (37, 19), (int(rng.integers(2, 65)), int(rng.integers(2, 41)))]
    W, H = sizes[rng.integers(len(sizes))]
    fov = float(10.0 ** rng.uniform(0, math.log10(150)))
    dist = max(float(np.linalg.norm(centre.astype(np.float64) - eye)), 0.1 * float(np.linalg.norm(half)))
    focal = dist * 10.0 ** rng.uniform(-2, 2)
    dof = bool(rng.integers(2))
    cut = cc._cutoff_aperture(pkg, W, H, fov, focal, 1.0)  # (may be negative at 150 degrees and 1 pixel: the footprint alone is too large)
    kind = rng.integers(5)
    aperture = [0.0, cut * rng.uniform(0, 0.9), cut * rng.uniform(0, 0.9), cut * 0.999, cut * 1.001][kind]
    cam = pkg.scenes.make_camera(W, H, fov, eye, target, (0.1, 1, 0.05), dof, focal, abs(aperture))
    if rng.random() < 0.03:  # not orthonormal: refused
        cam["orientation"] = (np.asarray(cam["orientation"], f32) * f32(1.2)).astype(f32)
    return cam, lo, hi


def _tube_excess(cam, info, lo, hi, rng):
    """max over rays and parameters s of |X(s) - X0(s)| - rho, in float64, for the extremal and some interior rays of a few pixels, over
    the part of each ray inside [lo, hi]; None if no ray meets the box."""
    W, H = int(cam["width"]), int(cam["height"])
    n = W * H
    pix = np.unique(np.concatenate([[0, W - 1, n - W, n - 1, n // 2], rng.integers(0, n, 3)]))
    eye0, d0 = cc.central_rays(cam, info)  # k_classify's own central rays
    eye0, d0 = eye0.astype(np.float64), d0.astype(np.float64)
    O = np.asarray(cam["orientation"], np.float64).reshape(3, 3)
    eye = np.asarray(cam["position"], np.float64)
    scale, aspect = float(info["scale"]), float(info["aspect"])
    F, R = float(info["focal"]), float(info["lens"])
    top = float(cc.ONE_BELOW)
    lens = [(0.0, 0.0)] + [(R * math.sqrt(top) * math.cos(k * math.pi / 4), R * math.sqrt(top) * math.sin(k * math.pi / 4)) for k in range(8)]
    rows = [(u0, u1, dx, dy) for u0 in (0.0, top) for u1 in (0.0, top) for dx, dy in lens]
    for _ in range(8):  # interior samples
        r, th = R * math.sqrt(rng.random()), 2 * math.pi * rng.random()
        rows.append((rng.random(), rng.random(), r * math.cos(th), r * math.sin(th)))
    rows = np.asarray(rows)
    worst = None
    for m in pix:
        i, j = m % W, m // W
        x = (1 - 2 * (i + rows[:, 0]) / W) * aspect * scale
        y = (1 - 2 * (j + rows[:, 1]) / H) * scale
        Lc = np.stack([rows[:, 2], rows[:, 3], np.zeros(len(rows))], axis=1)
        Pc = np.stack([x * F, y * F, np.full(len(rows), F)], axis=1)
        L, D = eye + Lc @ O.T, (Pc - Lc) @ O.T  # X(s) = L + s D
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo - L) / D, (hi - L) / D
        t1, t2 = np.where(np.isnan(t1), -np.inf, t1), np.where(np.isnan(t2), np.inf, t2)
        s_in = np.maximum(np.minimum(t1, t2).max(axis=1), 0.0)
        s_out = np.maximum(t1, t2).min(axis=1)
        ok = s_out >= s_in
        if not ok.any():
            continue
        s = s_in[ok, None] + (s_out[ok] - s_in[ok])[:, None] * np.linspace(0, 1, 9)[None, :]
        X = L[ok, None, :] + s[:, :, None] * D[ok, None, :]
        X0 = eye0[None, None, :] + s[:, :, None] * d0[m][None, None, :]
        e = float((np.linalg.norm(X - X0, axis=2)).max()) - float(info["rho"])
        worst = e if worst is None else max(worst, e)
    return worst


def test_no_camera_ray_leaves_the_tube_of_its_central_ray(pkg, hip):
    """(a) For a few thousand random cameras and root boxes -- the eye inside, outside and on a face of the box, with and without depth of
    field, apertures up to just under and just over the fmin cut-off, 1 to 150 degrees, 1x1 to 64x40 frames, focal distances 1e-2 to 1e2
    times the distance to the box -- every extremal ray stays within rho (mcpt_cull_bound) of k_classify's central ray at equal s."""
    rng = np.random.default_rng(2024)
    accepted = refused = checked = 0
    worst = -np.inf
    for _ in range(3000):
        cam, lo, hi = _random_camera(pkg, rng)
        info = hip.cull_bound(cam, lo, hi)
        if not info["classified"]:
            refused += 1
            assert info["rho"] == 0
            continue
        accepted += 1
        e = _tube_excess(cam, info, lo.astype(np.float64), hi.astype(np.float64), rng)
        if e is None:
            continue
        checked += 1
        worst = max(worst, e)
        assert e <= 0, (e, info, cam, lo, hi)
    print("\n[cull lemma] %d cameras accepted (%d with rays inside the box), %d refused; largest |X - X0| - rho = %.3g" % (accepted, checked, refused, worst))
    assert accepted > 1000 and refused > 100 and checked > 1000


def test_cull_bound_arguments_and_camera_constants(pkg, hip):
    """classified == 0 for a matrix that is not orthonormal and just over the aperture cut-off, 1 just under it; scale and aspect are those
    of the camera rays; null pointers and empty frames are refused."""
    import ctypes as C
    lo, hi = f32([-70, 0, -70]), f32([70, 90, 70])
    under = hip.cull_bound(cc.camera(pkg, "thin_aperture_under"), lo, hi)
    over = hip.cull_bound(cc.camera(pkg, "thin_aperture_over"), lo, hi)
    assert under["classified"] == 1 and under["rho"] > 0 and over["classified"] == 0 and over["rho"] == 0
    assert 0.05 * 10.0 < under["fmin"] < 0.051 * 10.0 and 0.049 * 10.0 < over["fmin"] < 0.05 * 10.0
    cam = cc.camera(pkg, "thin_dof")
    info = hip.cull_bound(cam, lo, hi)
    half = f32(cam["fov"]) * f32(0.5)
    assert info["scale"] == f32(math.tan(float(f32(float(half * f32(3.141592653589793)) / 180.0)))) and info["aspect"] == f32(64) / f32(40)
    assert info["focal"] == f32(150) and info["lens"] == f32(4) and info["s_far"] == info["reach"] / info["fmin"]
    nodof = hip.cull_bound(cc.camera(pkg, "thin"), lo, hi)
    assert nodof["focal"] == 1 and nodof["lens"] == 0
    odd = np.array(cam, copy=True)
    odd["orientation"] = (np.asarray(cam["orientation"], f32) * f32(1.3)).astype(f32)
    assert hip.cull_bound(odd, lo, hi)["classified"] == 0
    L = hip.lib()
    ci = hip.CullInfo()
    c = np.ascontiguousarray(cam)
    assert L.mcpt_cull_bound(None, hip._ptr(lo), hip._ptr(hi), C.byref(ci)) == 1
    assert L.mcpt_cull_bound(hip._ptr(c), None, hip._ptr(hi), C.byref(ci)) == 1
    assert L.mcpt_cull_bound(hip._ptr(c), hip._ptr(lo), hip._ptr(hi), None) == 1
    assert L.mcpt_debug_classify(None, hip._ptr(c), None, None, None) == 1
    c["width"] = 0
    assert L.mcpt_cull_bound(hip._ptr(c), hip._ptr(lo), hip._ptr(hi), C.byref(ci)) == 1
    assert C.sizeof(hip.CullInfo) == 56


@pytest.mark.parametrize("case", [c for c in cc.CASES if c.host_tree], ids=lambda c: c.id)
def test_restated_classification_is_conservative(pkg, hip, oracle, monkeypatch, case):
    """(c) Every primitive a worst-case or real camera ray of a pixel hits (the oracle's closest hit) is allowed by the pixel's class:
    no hit in a sky pixel, no hit outside a short list.  Zero exceptions; and the classes each case is there for do occur."""
    sd = cc.scene(pkg, case.scene)
    cc.set_tree(monkeypatch, case)
    bvh = hip.bvh_dump(sd)
    cam = cc.camera(pkg, case.cam, bvh[0]["root_min"], bvh[0]["root_max"])
    info = hip.cull_bound(cam, bvh[0]["root_min"], bvh[0]["root_max"])
    assert bvh[0]["n_instances"] == (14 if case.instancing else 0)
    may_hit, cand = cc.classify(bvh, cam, info)
    cc.check_non_vacuous(case, may_hit, cand)
    pix, prim = cc.oracle_rays(pkg, oracle, case, cam)
    bad = cc.violations(may_hit, cand, pix, prim)
    print("[cull rays] %s: %d rays, %d hits, %d violations" % (case.id, len(pix), int((prim >= 0).sum()), int(bad.sum())))
    assert not bad.any(), (int(bad.sum()), pix[bad][:8], prim[bad][:8], cand[pix[bad][:8]])
    if case.cam == "thin_37x19":  # the axis branch of beam_box runs: direction components that are exactly 0
        _, d = cc.central_rays(cam, info)
        assert (d[:, 0] == 0).sum() == 19 and (d[:, 1] == 0).sum() == 37
    if case.cam == "thin_aperture_over":
        assert info["classified"] == 0 and (cand[:, 0] == -2).all() and may_hit.all()
    if case.cam == "thin_face":
        assert float(cam["position"][2]) == float(bvh[0]["root_min"][2])
    if case.scene in ("sphere", "triangle"):
        assert bvh[0]["n_nodes"] == 0 and bvh[0]["root"] < 0  # the root is a leaf
