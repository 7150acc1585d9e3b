"""direct_is_zero's total-internal-reflection rule (csrc/mcpt_kernels.hip, DESIGN.md section 6 shortcut 8), restated in numpy, and the
scene that tests/test_gpu_direct_tir.py renders.

The rule: a Dirac dielectric seen from inside (wo.N < 0) beyond the refraction gate skips direct lighting if

    sin2 = ior^2 |wo - (wo.N) N|^2 > 1.001 (1 + 0.0143 (1 + ior))^2          (float32, the kernel's expression)

because Material::eval then fails `h.N >= 1 - EPSILON` for EVERY direction ws: h is the direction of -ws - ior wo, whose tangential part
is at least ior |wo_t| - 1 long against a length of at most 1 + ior, and h.N >= 1 - 1.01e-4 (EPSILON plus the float budget) allows a
tangential share of 0.014212.  This file checks that statement without a GPU over random indices and incidences around the bound, and
shows that the check can fail with a lower bound.  The kernel's own constants are checked on the GPU, where the scene below puts glass
faces on both sides of the bound with an emitter where eval comes closest to passing."""
import os

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = f32(1e-4)


def _pkg():
    import mcpt_loader
    return mcpt_loader.load()


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])).astype(f32)


def tir_bound(ior, factor=1.001):
    """The right-hand side of the rule in float32; factor: DevScene::tir_bound_factor (1.001 x the checking build's knob)."""
    b = f32(f32(1) + f32(0.0143) * f32(f32(1) + f32(ior)))
    return f32(f32(factor) * f32(b * b))


def sin2_of(n, wo, ior):
    """direct_is_zero's sin2 (float32)."""
    n, wo, ior = n.astype(f32), wo.astype(f32), f32(ior)
    wot = (wo - n * dot32(wo, n)).astype(f32)
    return f32(f32(ior * ior) * dot32(wot, wot))


def passes_eval_inside(ws, n, wo, ior):
    """Material::eval's test for a Dirac dielectric with isReflect = false, float32, for rows of unit directions ws: True where a light
    sample in that direction could give a non-zero contribution."""
    ws = ws.astype(f32)
    n, wo = n.astype(f32)[None, :], wo.astype(f32)[None, :]
    eta = np.where(dot32(ws, n) > 0, f32(ior), f32(f32(1) / f32(ior))).astype(f32)
    hv = ((-ws) - wo * eta[:, None]).astype(f32)
    h = (hv / np.sqrt(dot32(hv, hv))[:, None]).astype(f32)
    h = np.where((dot32(h, n) > 0)[:, None], h, -h)
    return ~((dot32(ws, n) * dot32(wo, n) >= 0) | (dot32(h, n) < f32(1) - EPS))


def _check(seed, n_conf, factor):
    """(claimed, violations): vertices the rule claims with `factor` on its bound, and those among them for which one of 8192 directions
    -- 4096 over the whole sphere, 4096 crowded around the tangent plane opposite wo_t, where eval comes closest -- passes eval."""
    rng = np.random.default_rng(seed)
    claimed = violations = 0
    for _ in range(n_conf):
        ior = f32(rng.uniform(1.02, 3.0))
        n = rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(f32)
        t = rng.normal(size=3)
        t -= n.astype(np.float64) * (t @ n)
        t /= np.linalg.norm(t)
        s_wo = min(np.sqrt(float(tir_bound(ior)) * 10.0 ** rng.uniform(-0.03, 0.02)) / float(ior), 0.9999)  # |wo_t| around the bound
        wo = (t * s_wo - n.astype(np.float64) * np.sqrt(1.0 - s_wo * s_wo)).astype(f32)
        if not sin2_of(n, wo, ior) > tir_bound(ior, factor):
            continue
        claimed += 1
        ws = rng.normal(size=(8192, 3))
        ws[4096:] = -t[None, :] + 0.05 * rng.normal(size=(4096, 3)) + n.astype(np.float64)[None, :] * np.abs(rng.normal(size=(4096, 1))) * 0.05
        ws /= np.linalg.norm(ws, axis=1)[:, None]
        violations += int(passes_eval_inside(ws, n, wo, ior).any())
    return claimed, violations


def test_total_internal_reflection_rule_claims_no_vertex_a_light_sample_could_reach():
    claimed, violations = _check(21, 600, 1.001)
    print("\n[rule T, numpy] %d vertices claimed, %d violations" % (claimed, violations))
    assert claimed > 150 and violations == 0


def test_total_internal_reflection_restatement_can_fail():
    """The negative control: with the bound scaled by 0.85 (the value the GPU test uses) the rule claims vertices just short of and just
    beyond total internal reflection, and directions near the tangent plane pass eval for some of them."""
    claimed, violations = _check(21, 600, 1.001 * 0.85)
    assert violations > 0


# --------------------------------------------------------------------------- the scene of tests/test_gpu_direct_tir.py
EYE = np.array([0.0, 0.0, 60.0])
IORS = (1.5, 1.8)
STEPS_DEG = [-5, -3, -2, -1.5, -1, -0.7, -0.4, -0.2, -0.1, 0.1, 0.2, 0.4, 0.7, 1, 1.5, 2, 3, 5]
BETA0 = np.deg2rad(43.0)  # the emitter's centre lies at this angle from the viewing direction, 6 away; it spans 29 to 57 degrees
LIGHT_C = 6.0 * np.array([0.0, np.sin(BETA0), -np.cos(BETA0)])


def _square(centre, n, e):
    """A square of half width e around `centre`, facing n (cross(v1 - v0, v2 - v0) is the normal the library computes)."""
    n = n / np.linalg.norm(n)
    t = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    t /= np.linalg.norm(t)
    u = np.cross(n, t)
    return (tuple(centre - e * t - e * u), tuple(centre + e * t - e * u), tuple(centre + e * t + e * u), tuple(centre - e * t + e * u))


def _tris(quads):
    t = np.zeros(2 * len(quads), _pkg().scenes.TRI_DTYPE)
    for i, (a, b, c, d) in enumerate(quads):
        t["v0"][2 * i], t["v1"][2 * i], t["v2"][2 * i] = a, b, c
        t["v0"][2 * i + 1], t["v1"][2 * i + 1], t["v2"][2 * i + 1] = a, c, d
    return t


def bound_angle(ior):
    """The inside incidence at which sin2 meets the rule's bound (radians)."""
    return np.arcsin(np.sqrt(float(tir_bound(ior))) / ior)


def tir_scene(w=240, h=160):
    """36 glass prisms seen from far away through an entry face perpendicular to the camera's ray, so that the ray meets the second face
    from inside at the prism's angle: the bound's angle (43.7 degrees for ior 1.5, 35.3 for 1.8) -5 ... +5 degrees in steps down to
    0.1 (the pixels of one prism sweep another +-0.05 continuously).  The second face is turned so that its tangent plane, in the
    direction opposite wo_t, points at one long emitter 6 away that covers elevations from below the plane to 15 degrees above it: where
    a refracted ray just short of total internal reflection leaves, and where eval comes closest to passing just beyond it.
    Returns (scene, list of (ior, step in degrees, vertex on the second face, its normal, wo there))."""
    s = _pkg().scenes
    b = s._Builder()
    up = np.array([0.0, 1.0, 0.0])
    to_eye = -LIGHT_C / np.linalg.norm(LIGHT_C)
    across = np.cross(to_eye, [1.0, 0.0, 0.0])  # the emitter's long side lies in the plane of incidence (y, z)
    across /= np.linalg.norm(across)
    P = lambda u, v: tuple(LIGHT_C + across * u + np.array([1.0, 0.0, 0.0]) * v)
    quad = (P(-1.5, -0.2), P(1.5, -0.2), P(1.5, 0.2), P(-1.5, 0.2))
    nl = np.cross(np.subtract(quad[1], quad[0]), np.subtract(quad[2], quad[0]))
    if nl @ to_eye < 0:  # the emitter faces the prisms
        quad = (quad[0], quad[3], quad[2], quad[1])
    b.add_mesh(_tris([quad]), b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(40, 35, 30))))
    b.add_mesh(_tris([((-12, -12, -9), (12, -12, -9), (12, 12, -9), (-12, 12, -9))]), b.material("rough_white_conductor", s.material_presets()["rough_white_conductor"]))
    items = []
    k = 0
    for ior in IORS:
        glass = b.material("glass%d" % int(ior * 10), s._mat(s.SMOOTH_DIELECTRIC, 0.01, iorA=ior, iorB=0.0))
        for step in STEPS_DEG:
            p = np.array([-1.2 + 0.3 * (k % 9), -0.45 + 0.3 * (k // 9), 0.0])
            d = (p - EYE) / np.linalg.norm(p - EYE)
            alpha = bound_angle(ior) + np.deg2rad(step)
            q = p + 0.07 * d
            eh = (LIGHT_C - q) / np.linalg.norm(LIGHT_C - q)
            g = eh - d * (eh @ d)
            g /= np.linalg.norm(g)
            n = np.cos(alpha) * d - np.sin(alpha) * g
            b.add_mesh(_tris([_square(p, -d, 0.04), _square(q, n, 0.09)]), glass)
            items.append((ior, step, q, n, -d))
            k += 1
    cam = s.make_camera(w, h, 3.2, tuple(EYE), (0.0, 0.0, 0.0))
    sd = s.SceneData(triangles=np.concatenate(b.tris).astype(s.TRI_DTYPE), materials=np.stack(b.mats).astype(s.MAT_DTYPE),
                     objects=np.stack(b.objs).astype(s.OBJ_DTYPE), background=np.float32([0.05, 0.05, 0.08]), camera=cam,
                     rr_rate=0.8, spp=16, name="tir")
    return sd, items, quad


def test_tir_scene_straddles_the_rule():
    """Per index of refraction, the prisms lie on both sides of the bound; the emitter is where it matters:
    for the prisms the rule with the lowered bound would claim, points of the emitter do pass eval (so the GPU's negative control has
    something to count), and for none of those the shipped rule claims."""
    sd, items, quad = tir_scene()
    rng = np.random.default_rng(5)
    uv = rng.random((4096, 2))
    a, b_, c, d_ = [np.asarray(v, np.float64) for v in quad]
    pts = a[None, :] + (b_ - a)[None, :] * uv[:, :1] + (d_ - a)[None, :] * uv[:, 1:]
    for ior in IORS:
        claimed = unclaimed = gate = lit_if_lowered = 0
        for i, step, q, n, wo in items:
            if i != ior:
                continue
            s2 = sin2_of(f32(n), f32(wo), ior)
            assert wo @ n < 0
            assert abs(np.sqrt(float(s2)) - ior * np.sin(bound_angle(ior) + np.deg2rad(step))) < 1e-4
            gate += int(s2 < f32(0.81))
            ws = pts - q[None, :]
            ws /= np.linalg.norm(ws, axis=1)[:, None]
            lit = bool(passes_eval_inside(ws, f32(n), f32(wo), ior).any())
            if s2 > tir_bound(ior):
                claimed += 1
                assert not lit
            else:
                unclaimed += 1
                lit_if_lowered += int(lit and s2 > tir_bound(ior, 1.001 * 0.85))
        print("\n[tir scene] ior %.1f: %d prisms claimed, %d not (%d within the gate), %d lit ones the lowered bound would claim"
              % (ior, claimed, unclaimed, gate, lit_if_lowered))
        assert claimed == 9 and unclaimed == 9 and lit_if_lowered >= 3
