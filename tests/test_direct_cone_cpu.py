"""direct_is_zero's cone rule (csrc/mcpt_kernels.hip), restated in numpy in float32 with the kernel's expressions,
swept over the indices of refraction mcpt_scene_create accepts, and the scene that tests/test_gpu_direct_cone.py renders.

The rule: a Dirac vertex skips direct lighting if the mirror direction (seen from outside) or the Snell direction (a dielectric seen
from inside, behind the gate sin2 < 0.81) is farther than a tolerance from the cone that holds every light sample: 0.06 rad for
reflection, 0.15 rad for refraction.  Material::eval passes a direction ws only if h.N >= 1 - EPSILON, and how far such a ws can lie
from the Snell direction grows with the index:  angle <= asin(0.9 + d) - asin(0.9),  d = 0.014212 (1 + ior)  (the proof stands above
direct_is_zero).  The constant 0.15 rad covers that bound up to ior 2.5, so the rule declines to claim a refraction vertex above
kConeMaxIor = 2.5.  Before that limit existed the rule claimed vertices at ior 4.75 and above that a light sample does reach.

This file draws directions around the Snell / mirror direction, keeps those that pass eval (passes_eval_inside of
test_direct_tir_cpu.py and its reflection twin), puts an emitter sphere around each and asserts that the rule claims none of them;
it prints, per index, how far a passing direction was found from the Snell direction; and it shows that the check fails without
the limit."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("mcpt_tir_cpu_for_cone", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_direct_tir_cpu.py"))
_tir = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tir)

f32 = np.float32
dot32, passes_eval_inside, EPS = _tir.dot32, _tir.passes_eval_inside, _tir.EPS

CONE_MAX_IOR = 2.5  # kConeMaxIor
_COS_SIN = {0.06: (f32(0.99820054), f32(0.05996400)), 0.15: (f32(0.98877108), f32(0.14943813))}  # the kernel's constants


def _tolerance(angle, scale):
    """cone_tolerance(): the constants, or cos / sin of the angle and the slack on the cosine scaled by the checking build's knob."""
    if scale == 1.0:
        return _COS_SIN[angle] + (f32(1e-3),)
    a = f32(f32(angle) * f32(scale))
    return f32(np.cos(a)), f32(np.sin(a)), f32(f32(1e-3) * f32(scale))


def proven_bound(ior):
    """The proven distance of a passing ws from the Snell direction (radians); None where 0.9 + d reaches 1."""
    d = 0.014212 * (1.0 + float(ior))
    return None if 0.9 + d >= 1.0 else float(np.arcsin(0.9 + d) - np.arcsin(0.9))


def cone_claims(n, wo, q, centres, R, ior, scale=1.0, max_ior=CONE_MAX_IOR):
    """direct_is_zero's cone branch in float32 for one Dirac dielectric vertex (q, n, wo) and rows of emitter bounding spheres
    (centres, R): True where the rule skips direct lighting.  wo.n >= 0: the reflection half; wo.n < 0: the refraction half.
    max_ior = None: the rule as it was before the index limit."""
    n, wo, q = np.asarray(n, f32), np.asarray(wo, f32), np.asarray(q, f32)
    L = (np.asarray(centres, f32) - q[None, :]).astype(f32)
    R = f32(R)
    no = np.zeros(len(L), bool)
    D2 = dot32(L, L)
    gate = D2 > f32(f32(R * R) * f32(1.0201))
    D = np.sqrt(D2)
    sl = (R / D).astype(f32)
    cl = np.sqrt(f32(1.0) - sl * sl)
    won = dot32(wo, n)
    if not won < 0:  # `inside` of k_shade
        r = (n * f32(f32(2) * dot32(n, wo)) - wo).astype(f32)
        cm, sm, slack = _tolerance(0.06, scale)
    else:
        ior = f32(ior)
        wot = (wo - n * won).astype(f32)
        sin2 = f32(f32(ior * ior) * dot32(wot, wot))
        if not sin2 < f32(0.81):
            return no  # (the total-internal-reflection rule's side of the gate)
        if max_ior is not None and not ior <= f32(max_ior):
            return no
        r = (wot * (-ior) + n * np.sqrt(f32(1.0) - sin2)).astype(f32)
        cm, sm, slack = _tolerance(0.15, scale)
    rl = np.sqrt(dot32(r, r))
    if not (rl > f32(0.5) and rl < f32(2.0)):
        return no
    cos_a = (dot32(r[None, :], L) / (rl * D)).astype(f32)
    return gate & (cos_a < (cl * cm - sl * sm) - slack)


def passes_eval_reflect(ws, n, wo):
    """Material::eval's test for a Dirac material with isReflect = true (mat_eval's Dirac reflect branch), float32, for rows of unit
    directions ws: True where a light sample in that direction could give a non-zero contribution."""
    ws = ws.astype(f32)
    n, wo = n.astype(f32)[None, :], wo.astype(f32)[None, :]
    hv = (ws + wo).astype(f32)
    h = (hv / np.sqrt(dot32(hv, hv))[:, None]).astype(f32)
    h = np.where((dot32(ws, n) > 0)[:, None], h, -h)
    return ~((dot32(ws, n) * dot32(wo, n) <= 0) | (dot32(h, n) < f32(1) - EPS))


# --------------------------------------------------------------------------- the sweep
IORS = (0.6, 0.8, 1.0001, 1.3, 1.91, 2.353, 3.0, 4.0, 4.5, 4.75, 5.0, 6.0)
SIN2S = (0.1, 0.5, 0.7, 0.78, 0.80, 0.809)
RDS = (0.01, 0.1, 0.5, 0.99)
N_DIRS = 100000
DIST = 6.0


def _perp(rng, v):
    """Rows of unit vectors perpendicular to the rows of v, at a random azimuth."""
    p = np.cross(v, rng.normal(size=v.shape))
    return p / np.linalg.norm(p, axis=1)[:, None]


def _around(rng, axis, angle):
    """Unit directions at `angle` (a row of radians) from the rows of `axis`, at random azimuths (float64)."""
    axis = np.broadcast_to(axis, (len(angle), 3))
    return axis * np.cos(angle)[:, None] + _perp(rng, axis) * np.sin(angle)[:, None]


def _offsets(rng, n):
    """Half of the draws uniform up to 0.3 rad, half log-uniform from 1e-8 to 0.3 rad: for an index close to one only directions within
    1e-6 rad of the Snell direction pass."""
    a = rng.uniform(0.0, 0.3, n)
    a[n // 2:] = 0.3 * 10.0 ** rng.uniform(-7.5, 0.0, n - n // 2)
    return a


def _frame(rng):
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    t = np.cross(n, rng.normal(size=3))
    t /= np.linalg.norm(t)
    return n, t


def _claimed(rng, n, wo, P, ior, **kw):
    """How many of the emitter spheres around the passing directions P, per R / D, the rule claims.  A sphere's centre lies up to 0.95 of
    its angular radius from its passing direction, so that the direction stays inside the exact emitters too (R = 1.001 r + 1e-3)."""
    out = 0
    for rd in RDS:
        c = _around(rng, P.astype(np.float64), rng.uniform(0.0, 0.95, len(P)) * np.arcsin(rd)) * DIST
        out += int(cone_claims(n, wo, np.zeros(3), c, rd * DIST, ior, **kw).sum())
    return out


def sweep_refraction(ior, seed=11, **kw):
    """(passing directions, emitter spheres claimed although they hold a passing direction, farthest passing direction from the Snell
    direction in radians) over SIN2S x RDS for one index."""
    rng = np.random.default_rng(seed)
    passing = claimed = 0
    farthest = 0.0
    for sin2 in SIN2S:
        s_wo = np.sqrt(sin2) / ior
        if s_wo >= 0.9999:  # (an index below one: no such incidence)
            continue
        nd, t = _frame(rng)
        n = nd.astype(f32)
        wo = (t * s_wo - nd * np.sqrt(1.0 - s_wo * s_wo)).astype(f32)
        won = float(np.dot(wo.astype(np.float64), n.astype(np.float64)))
        wot = wo.astype(np.float64) - n.astype(np.float64) * won
        s2 = ior * ior * (wot @ wot)
        snell = -ior * wot + n.astype(np.float64) * np.sqrt(1.0 - s2)
        snell /= np.linalg.norm(snell)
        ws = _around(rng, snell, _offsets(rng, N_DIRS)).astype(f32)
        ws = (ws / np.sqrt(dot32(ws, ws))[:, None]).astype(f32)
        P = ws[passes_eval_inside(ws, n, wo, f32(ior))]
        passing += len(P)
        if len(P):
            farthest = max(farthest, float(np.arccos(np.clip(P.astype(np.float64) @ snell, -1, 1)).max()))
            claimed += _claimed(rng, n, wo, P, ior, **kw)
    return passing, claimed, farthest


def sweep_reflection(seed=12, **kw):
    rng = np.random.default_rng(seed)
    passing = claimed = 0
    farthest = 0.0
    for cos_o in (0.02, 0.2, 0.6, 0.95, 1.0):
        nd, t = _frame(rng)
        n = nd.astype(f32)
        wo = (t * np.sqrt(1.0 - cos_o * cos_o) + nd * cos_o).astype(f32)
        mirror = 2.0 * (nd @ wo.astype(np.float64)) * nd - wo.astype(np.float64)
        mirror /= np.linalg.norm(mirror)
        ws = _around(rng, mirror, _offsets(rng, N_DIRS)).astype(f32)
        ws = (ws / np.sqrt(dot32(ws, ws))[:, None]).astype(f32)
        P = ws[passes_eval_reflect(ws, n, wo)]
        passing += len(P)
        farthest = max(farthest, float(np.arccos(np.clip(P.astype(np.float64) @ mirror, -1, 1)).max()))
        claimed += _claimed(rng, n, wo, P, 1.5, **kw)
    return passing, claimed, farthest


def test_cone_rule_claims_no_emitter_a_passing_direction_points_into():
    print("\n[cone rule, numpy] index: passing directions, farthest from the Snell direction (rad), proven bound, spheres claimed")
    for ior in IORS:
        passing, claimed, farthest = sweep_refraction(ior)
        bound = proven_bound(ior)
        print("  %-7g %7d   %.4f   %s   %d" % (ior, passing, farthest, "%.4f" % bound if bound else "  -   ", claimed))
        assert passing >= 1000, ior
        assert claimed == 0, ior
        if ior <= CONE_MAX_IOR:  # where the rule claims, the measurement stays within the proof and the proof within the tolerance
            assert farthest <= bound <= proven_bound(CONE_MAX_IOR) < 0.15 - 0.015
    passing, claimed, farthest = sweep_reflection()
    print("  mirror  %7d   %.4f   %.4f   %d" % (passing, farthest, 2 * np.arccos(1 - 1.01e-4), claimed))
    assert passing >= 1000 and claimed == 0 and farthest <= 2 * np.arccos(1 - 1.01e-4) < 0.06 / 1.5


def test_cone_restatement_can_fail():
    """The negative control: without the index limit (the constant 0.15 rad at every index) the same check reports emitters that the rule
    claims although a passing direction points into them, at index 5 and 6; so does a reflection tolerance of 0.2 x 0.06 rad."""
    for ior in (5.0, 6.0):
        passing, claimed, _ = sweep_refraction(ior, max_ior=None)
        print("\n[cone rule, numpy, no index limit] index %g: %d of %d x %d spheres claimed" % (ior, claimed, passing, len(RDS)))
        assert claimed > 0, ior
    assert sweep_reflection(scale=0.2)[1] > 0


# --------------------------------------------------------------------------- the scene of tests/test_gpu_direct_cone.py
EYE = np.array([0.0, 0.0, 60.0])
LIGHT_C = np.zeros(3)  # one emitter, 0.1 x 0.1, straight ahead of the camera and facing it
LIGHT_E = 0.05
CONE_IORS = (1.5, 2.353, 3.0, 4.0, 5.0, 6.0)
CONE_SIN2 = (0.7, 0.80)
CONE_MISS = (0.05, 0.10, 0.13, 0.16, 0.19, 0.22, 0.30)
FACE_E = 0.05  # half width of a prism's entry face; the second face is twice as wide, 0.2 / 6 = 0.033 rad as seen from the emitter


def light_sphere():
    """The emitters' bounding sphere as mcpt_scene.cpp computes it: the box's centre, its corner distance x 1.001 + 1e-3."""
    return LIGHT_C, float(np.sqrt(2.0) * LIGHT_E * 1.001 + 1e-3)


def cone_scene(w=240, h=160):
    """84 glass prisms around the camera's axis, each 6 away from one small emitter on that axis.  The camera's ray enters a prism
    through a face perpendicular to it and meets the second face from inside at sin2 = ior^2 sin^2(alpha) in CONE_SIN2.  Where the
    prism stands fixes the angle between that ray and the direction to the emitter; it is chosen so that the Snell exit direction
    misses the emitter's centre by CONE_MISS in the plane of incidence, on the grazing side, where a passing ws lies farthest.
    Returns (scene, list of (ior, sin2, miss, vertex on the second face, its normal, wo there))."""
    s = _tir._pkg().scenes
    b = s._Builder()
    e = LIGHT_E
    b.add_mesh(_tir._tris([((-e, -e, 0.0), (e, -e, 0.0), (e, e, 0.0), (-e, e, 0.0))]), b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(4000, 3500, 3000))))
    b.add_mesh(_tir._tris([((-14, -14, -3), (14, -14, -3), (14, 14, -3), (-14, 14, -3))]), b.material("rough_white_conductor", s.material_presets()["rough_white_conductor"]))
    conf = []
    for ior in CONE_IORS:
        for sin2 in CONE_SIN2:
            for miss in CONE_MISS:
                alpha = np.arcsin(np.sqrt(sin2) / ior)
                beta = (np.arcsin(np.sqrt(sin2)) - alpha) + miss  # between the ray inside the glass and the direction to the emitter
                conf.append((beta, ior, sin2, miss, alpha))
    conf.sort()
    items = []
    axis = (LIGHT_C - EYE) / np.linalg.norm(LIGHT_C - EYE)
    c = np.linalg.norm(LIGHT_C - EYE)
    for k, (beta, ior, sin2, miss, alpha) in enumerate(conf):
        psi = 2.399963 * k  # the golden angle: neighbours in beta, which stand at similar distances from the axis, get apart
        u = np.array([np.cos(psi), np.sin(psi), 0.0])
        omega = np.arcsin(DIST * np.sin(beta) / c)  # the triangle eye - vertex - emitter: angle beta outside at the vertex, omega at the eye
        q = LIGHT_C + DIST * (-np.cos(beta - omega) * axis + np.sin(beta - omega) * u)
        d = (q - EYE) / np.linalg.norm(q - EYE)
        eh = (LIGHT_C - q) / DIST
        g = eh - d * (eh @ d)
        g /= np.linalg.norm(g)
        n = np.cos(alpha) * d - np.sin(alpha) * g
        glass = b.material("glass%g" % ior, s._mat(s.SMOOTH_DIELECTRIC, 0.01, iorA=ior, iorB=0.0))
        b.add_mesh(_tir._tris([_tir._square(q - 0.08 * d, -d, FACE_E), _tir._square(q, n, 2 * FACE_E)]), glass)
        items.append((ior, sin2, miss, q, n, -d))
    cam = s.make_camera(w, h, 13.0, tuple(EYE), tuple(LIGHT_C))
    sd = s.SceneData(triangles=np.concatenate(b.tris).astype(s.TRI_DTYPE), materials=np.stack(b.mats).astype(s.MAT_DTYPE),
                     objects=np.stack(b.objs).astype(s.OBJ_DTYPE), background=np.float32([0.05, 0.05, 0.08]), camera=cam,
                     rr_rate=0.8, spp=16, name="cone")
    return sd, items


def scene_model(items, **kw):
    """Per prism, over a 7 x 7 grid of vertices on its second face as the camera sees them: (the rule claims a vertex that a point of
    the emitter lights, the rule claims a vertex)."""
    rng = np.random.default_rng(6)
    pts = np.zeros((256, 3))
    pts[:, :2] = rng.uniform(-LIGHT_E, LIGHT_E, (256, 2))
    centre, R = light_sphere()
    out = []
    for ior, sin2, miss, q, n, wo in items:
        t1 = np.cross(n, wo)
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(n, t1)
        wrong = claims = False
        for a in np.linspace(-1.8 * FACE_E, 1.8 * FACE_E, 7):
            for b_ in np.linspace(-1.8 * FACE_E, 1.8 * FACE_E, 7):
                v = q + a * t1 + b_ * t2
                w = (EYE - v) / np.linalg.norm(EYE - v)
                ws = pts - v[None, :]
                ws /= np.linalg.norm(ws, axis=1)[:, None]
                claim = bool(cone_claims(n, w, v, centre[None, :], R, ior, **kw)[0])
                claims |= claim
                wrong |= claim and bool(passes_eval_inside(ws, f32(n), f32(w), f32(ior)).any())
        out.append((wrong, claims))
    return out


def test_cone_scene_sits_on_the_tolerance():
    """The prisms' geometry is what the docstring says; the rule without the index limit claims at least 3 prisms that the emitter
    lights, all of them above the limit, and the shipped rule claims none of those; at the preset indices the shipped rule does claim
    prisms (it has work), none of them lit; the control's scale 0.2 claims a lit prism at a preset index, 0.05 rad off."""
    sd, items = cone_scene()
    centre, R = light_sphere()
    assert len(items) == len(CONE_IORS) * len(CONE_SIN2) * len(CONE_MISS)
    qs = np.array([it[3] for it in items])
    ds = np.array([-it[5] for it in items])
    # no prism stands in front of another as seen from the camera: directions at least two entry faces apart
    ang = np.arccos(np.clip(ds @ ds.T, -1, 1)) + 10.0 * np.eye(len(items))
    assert ang.min() > 2.0 * np.sqrt(2.0) * FACE_E / (EYE[2] - 6.0), ang.min()
    for ior, sin2, miss, q, n, wo in items:
        assert abs(np.linalg.norm(q - centre) - DIST) < 1e-9 and 0.011 < R / DIST < 0.013
        assert wo @ n < 0
        assert abs(float(_tir.sin2_of(f32(n), f32(wo), ior)) - sin2) < 1e-4
        wot = wo - n * (wo @ n)
        snell = -ior * wot + n * np.sqrt(1.0 - ior * ior * (wot @ wot))
        eh = (centre - q) / DIST
        assert abs(np.arccos(snell @ eh) - miss) < 1e-6
        assert np.arccos(eh @ n) > np.arccos(snell @ n)  # the emitter lies on the grazing side of the exit direction
        assert abs(np.linalg.det(np.stack([n, wo, eh]))) < 1e-9  # in the plane of incidence
    parent = scene_model(items, max_ior=None)
    fixed = scene_model(items)
    control = scene_model(items, scale=0.2)
    wrong = [it[:3] for it, (w, _) in zip(items, parent) if w]
    print("\n[cone scene] prisms with lit vertices that the rule without the index limit claims:", wrong)
    assert len(wrong) >= 3 and all(ior > CONE_MAX_IOR for ior, _, _ in wrong)
    assert not any(w for w, _ in fixed)
    assert sum(claims for it, (_, claims) in zip(items, fixed) if it[0] <= CONE_MAX_IOR) >= 4  # the shipped rule has work in this scene
    assert not any(claims for it, (_, claims) in zip(items, fixed) if it[0] > CONE_MAX_IOR)
    wrong = [it[:3] for it, (w, _) in zip(items, control) if w]
    print("[cone scene] prisms with lit vertices that the rule with its tolerances x 0.2 claims:", wrong)
    assert any(ior <= CONE_MAX_IOR and miss == 0.05 for ior, _, miss in wrong)
