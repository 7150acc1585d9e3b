"""direct_is_zero's half-space rule (csrc/mcpt_kernels.hip, DESIGN.md section 6 shortcut 8), restated in numpy, and the scene that
tests/test_gpu_direct_halfspace.py renders.

The rule: with c, R the emitters' bounding sphere (R = 1.001 r + 1e-3 for the exact radius r, mcpt_scene.cpp), L = fl(c - q) and
k = kHalfspaceSlack = 1e-5, a vertex (q, n) outside the distance gate |L|^2 > 1.0201 R^2 skips direct lighting if

    n.L < -(R + k (|c|_1 + R) + k |L|_1)                     (all in float32, in the kernel's order of operations)

because then the float value normalized(x_l - q).n that k_direct computes is negative for EVERY light sample x_l, and every branch
of Material::eval returns 0 at its first test.  The margin is derived from the unit roundoff u = 2^-24: x_l leaves the emitters' hull
by at most 6u (|c| + r), ws.n errs by 8u (|L| + r), the rule's own n.L by 4u |L|: 12u = 7.2e-7 relative to |c| + |L| + 2r covers them,
and k is more than ten times that.  This file checks that statement without a GPU: over random emitters, vertices and normals placed
on the rule's edge, whenever the rule accepts, all of 4096 light samples -- the corners of the emitter among them -- give a negative
float32 cosine; and with the margin removed AND the plane pushed into the emitter the same check fails (the check can fail)."""
import os

import numpy as np

f32 = np.float32
K_SLACK = f32(1e-5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bounding_sphere(points):
    """mcpt_scene.cpp: centre = float centroid of the emitters' box, r over the 8 corners in double, R = (float)(r * 1.001 + 1e-3)."""
    mn, mx = points.min(0).astype(f32), points.max(0).astype(f32)
    c = (f32(0.5) * mn + f32(0.5) * mx).astype(f32)
    r2 = max(float(((np.where(k, mx, mn).astype(np.float64) - c.astype(np.float64)) ** 2).sum())
             for k in [np.array([i & 1, i & 2, i & 4], bool) for i in range(8)])
    return c, f32(np.sqrt(r2) * 1.001 + 1e-3)


def plane_constants(c, R, scale=1.0):
    """DevScene::light_plane as mcpt_upload.hip fills it (scale: the checking build's MCPT_HALFSPACE_SLACK_SCALE)."""
    k = f32(K_SLACK * f32(scale))
    c1 = f32(f32(abs(c[0]) + abs(c[1])) + abs(c[2]))
    return f32(R + f32(k * f32(c1 + R))), k


def rule_h(q, n, c, R, plane):
    """emitters_behind behind the distance gate, float32, operation for operation (vectorised over rows of q, n)."""
    L = (c[None, :] - q).astype(f32)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])).astype(f32)
    gate = dot(L, L) > f32(f32(R * R) * f32(1.0201))
    l1 = (np.abs(L[:, 0]) + (np.abs(L[:, 1]) + np.abs(L[:, 2]))).astype(f32)
    return gate & (dot(n, L) < -(plane[0] + plane[1] * l1).astype(f32))


def sampled_cosines(tri, q, n, u2, u3):
    """k_direct's dot(normalized(x_l - q), n) for Triangle::Sample points of `tri` (sample_light's float32 expression)."""
    x, y = np.sqrt(u2).astype(f32), u3.astype(f32)
    v0, v1, v2 = tri[0][None, :], tri[1][None, :], tri[2][None, :]
    xl = ((v0 * (f32(1) - x)[:, None] + v1 * (x * (f32(1) - y))[:, None]).astype(f32) + v2 * (x * y)[:, None]).astype(f32)
    d = (xl - q[None, :]).astype(f32)
    z = (d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])).astype(f32)
    ws = (d / np.sqrt(z).astype(f32)[:, None]).astype(f32)
    return (ws[:, 0] * n[0] + (ws[:, 1] * n[1] + ws[:, 2] * n[2])).astype(f32)


def _configurations(rng, n_conf):
    """Random emitter triangles (sizes 1e-2 .. 1e2, offsets up to 1e4 from the origin), unit normals, and vertices whose tangent plane
    passes within +-(1e-7 .. 1) * (|c| + R) of the bounding sphere's surface."""
    for _ in range(n_conf):
        size = 10.0 ** rng.uniform(-2, 2)
        off = rng.normal(size=3) * 10.0 ** rng.uniform(-1, 4)
        tris = (off[None, None, :] + rng.uniform(-size, size, (int(rng.integers(1, 4)), 3, 3))).astype(f32)
        c, R = bounding_sphere(tris.reshape(-1, 3))
        n = rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(f32)
        t = rng.normal(size=3)
        t -= n.astype(np.float64) * (t @ n)
        t /= np.linalg.norm(t)
        depth = float(rng.choice([-1, 1])) * 10.0 ** rng.uniform(-7, 0) * (np.abs(c).sum() + float(R))
        q = (c.astype(np.float64) + n.astype(np.float64) * (float(R) - depth) + t * float(R) * rng.uniform(0.2, 3.0)).astype(f32)
        # (n.L = -(R - depth): depth < 0 moves the plane away from the sphere, depth > 0 into it)
        yield tris, c, R, q, n


def _edge_uniforms(rng, m):
    u2, u3 = rng.random(m).astype(f32), rng.random(m).astype(f32)
    one = f32(1) - f32(2.0 ** -24)
    for i, (a, b) in enumerate([(0, 0), (one, 0), (one, one), (0, one), (one, 0.5), (0.5, one)]):
        u2[i], u3[i] = a, b
    return u2, u3


def test_rule_h_accepts_only_vertices_whose_every_light_sample_is_back_facing():
    rng = np.random.default_rng(7)
    accepted = rejected = 0
    for tris, c, R, q, n in _configurations(rng, 1500):
        plane = plane_constants(c, R)
        if not rule_h(q[None, :], n[None, :], c, R, plane)[0]:
            rejected += 1
            continue
        accepted += 1
        u2, u3 = _edge_uniforms(rng, 4096)
        for tri in tris:
            cos = sampled_cosines(tri, q, n, u2, u3)
            assert (cos < 0).all(), (c, R, q, n, float(cos.max()))
    print("\n[rule H, numpy] %d configurations accepted, %d rejected" % (accepted, rejected))
    assert accepted > 300 and rejected > 300  # the configurations sit on both sides of the rule


def test_rule_h_restatement_can_fail():
    """The negative control of the check above: a margin scaled by -3000 (the value the GPU test uses) accepts planes that cut the
    emitters' sphere, and for some of them a light sample has a positive cosine."""
    rng = np.random.default_rng(7)
    bad = 0
    for tris, c, R, q, n in _configurations(rng, 1500):
        if not rule_h(q[None, :], n[None, :], c, R, plane_constants(c, R, -3000.0))[0]:
            continue
        u2, u3 = _edge_uniforms(rng, 4096)
        bad += int(any((sampled_cosines(tri, q, n, u2, u3) >= 0).any() for tri in tris))
    assert bad > 0


# --------------------------------------------------------------------------- the scene of tests/test_gpu_direct_halfspace.py
DEPTHS = [-0.3, -0.1, -0.03, -0.01, -3e-3, -1e-3, -5e-4, -3e-4, -2e-4, -1e-4, -3e-5, 0.0, 3e-5, 1e-4, 2e-4, 3e-4, 1e-3, 3e-3, 5e-3,
          1e-2, 3e-2, 0.1, 0.3]
TILTS = [0.0, 5e-3, -2e-2]


def _quad(pkg, a, b, c, d):
    t = np.zeros(2, pkg.scenes.TRI_DTYPE)
    t["v0"], t["v1"], t["v2"] = [a, a], [b, c], [c, d]
    return t


def halfspace_scene(pkg, w=120, h=80):
    """Two 1 x 1 and 0.6 x 0.6 emitters 4.4 apart (bounding sphere R = 2.6, mostly empty), and beyond the corner P of the first one
    that lies on the sphere's box a ladder of 0.16-wide quads facing AWAY from the emitters, alternately rough conductor and rough
    dielectric: quad (depth, tilt) has its tangent plane at n.L = -(R - depth), i.e. `depth` inside the sphere (negative: outside),
    from -0.3 through 0 to +0.3 with steps down to 3e-5 around the rule's margin (1e-4 here), and its normal tilted by 0, 5e-3 and
    -2e-2 rad from the direction centre -> P.  For depth > R - r + r (1 - cos tilt) = 3.6e-3 .. 4.1e-3 the corner P of the emitter lies in front of the
    plane, so those quads DO receive light: a rule that claimed them would be caught.  Each quad is pushed sideways just beyond
    the distance gate D > 1.01 R; one (depth -0.01) is centred ON the gate.  A `clear_rough_plastic` sphere sits 0.4 from the second
    emitter, beyond it as seen from the centre (rough refraction from inside, with the emitters behind part of its surface); a rough
    floor sends paths at the quads from everywhere.  Returns (scene, centre, R, list of (depth, tilt, quad centre, normal))."""
    s = pkg.scenes
    P = s.material_presets()
    b = s._Builder()
    light = s._mat(s.ROUGH_CONDUCTOR, emission=(40, 35, 30))
    la = _quad(pkg, (-2.5, 3.0, -0.5), (-1.5, 3.0, -0.5), (-1.5, 3.0, 0.5), (-2.5, 3.0, 0.5))
    lb = _quad(pkg, (1.7, 3.4, 0.7), (2.3, 3.4, 0.7), (2.3, 3.4, 1.3), (1.7, 3.4, 1.3))
    b.add_mesh(la, b.material("light_a", light))
    b.add_mesh(lb, b.material("light_b", s._mat(s.ROUGH_CONDUCTOR, emission=(20, 25, 30))))
    pts = np.concatenate([np.concatenate([t["v0"], t["v1"], t["v2"]]) for t in (la, lb)]).astype(f32)
    c, R = bounding_sphere(pts)
    c64, R64 = c.astype(np.float64), float(R)
    corner = np.array([-2.5, 3.0, -0.5])
    m = (corner - c64) / np.linalg.norm(corner - c64)  # centre -> corner: the normal of the untilted quads
    down = np.array([0.0, -1.0, 0.0]) - m * (np.array([0.0, -1.0, 0.0]) @ m)
    down /= np.linalg.norm(down)
    side = np.cross(m, down)
    b.add_mesh(_quad(pkg, (-12, 0, -12), (-12, 0, 12), (12, 0, 12), (12, 0, -12)), b.material("rough_white_conductor", P["rough_white_conductor"]))
    mats = [("rough_white_conductor", P["rough_white_conductor"]), ("rough_plastic", P["rough_plastic"])]
    quads = []
    e = 0.08
    k = 0
    for depth in DEPTHS:
        for tilt in TILTS:
            n = np.cos(tilt) * m + np.sin(tilt) * side
            ta = np.cross(n, down)
            ta /= np.linalg.norm(ta)
            tb = np.cross(n, ta)  # (points down-ish)
            tau_gate = np.sqrt(max(1.0201 * R64 * R64 - (R64 - depth) ** 2, 0.0))
            on_gate = depth == -0.01 and tilt == 0.0
            tau = tau_gate if on_gate else tau_gate * 1.02 + 0.25 + 0.2 * (k % 4)
            phi = np.deg2rad(-70 + 140.0 * ((k * 7) % 23) / 22.0)
            p0 = c64 + n * (R64 - depth) + tau * (np.cos(phi) * tb + np.sin(phi) * ta)
            key, mat = mats[k % 2]
            b.add_mesh(_quad(pkg, p0 - e * ta - e * tb, p0 + e * ta - e * tb, p0 + e * ta + e * tb, p0 - e * ta + e * tb), b.material(key, mat))
            quads.append((depth, tilt, p0, n))
            k += 1
    sc = np.array([2.0, 3.4, 1.0]) - c64
    b.add_sphere(tuple(np.array([2.0, 3.0, 1.0]) + 0.75 * sc / np.linalg.norm(sc)), 0.35, b.material("clear_rough_plastic", P["clear_rough_plastic"]))
    eye = corner + m * 7.0 + down * 1.2
    cam = s.make_camera(w, h, 40, tuple(eye), tuple(corner + m * 0.5 + down * 1.2))
    sd = s.SceneData(triangles=np.concatenate(b.tris).astype(s.TRI_DTYPE), materials=np.stack(b.mats).astype(s.MAT_DTYPE),
                     objects=np.stack(b.objs).astype(s.OBJ_DTYPE), background=np.float32([0.05, 0.05, 0.08]), camera=cam,
                     rr_rate=0.8, spp=16, name="halfspace")
    return sd, c, R, quads


def test_halfspace_scene_straddles_the_rule():
    """The ladder really lies on both sides of the rule and of its margin, every quad but one lies beyond the distance gate, the quads
    face the right way (cross(v1 - v0, v2 - v0) is the normal the library computes), and some quads that a rule without margin
    would wrongly claim have the emitter's corner in front of them."""
    import mcpt_loader
    pkg = mcpt_loader.load()
    sd, c, R, quads = halfspace_scene(pkg)
    plane = plane_constants(c, R)
    tris = sd.triangles[6:6 + 2 * len(quads)]  # (two emitters and the floor come first)
    corner = np.array([-2.5, 3.0, -0.5])
    claimed = lit_if_claimed = 0
    for (depth, tilt, p0, n), t0 in zip(quads, tris[::2]):
        nn = np.cross(t0["v1"].astype(np.float64) - t0["v0"], t0["v2"].astype(np.float64) - t0["v0"])
        assert np.allclose(nn / np.linalg.norm(nn), n, atol=1e-5)
        q = np.float32(p0)[None, :]
        h = bool(rule_h(q, np.float32(n)[None, :], c, R, plane)[0])
        if depth == -0.01 and tilt == 0.0:  # the quad centred on the distance gate: the gate cuts it
            d = np.linalg.norm(c - p0) / float(R)
            assert abs(d - 1.01) < 1e-4
            continue
        claimed += h
        slack = float(plane[0] - R) + float(plane[1]) * float(np.abs(c - q[0]).sum())
        assert h == (depth < -slack) or abs(depth + slack) < 2e-5, (depth, tilt, slack)
        if depth > 5e-3:
            lit_if_claimed += int(n @ (corner - p0) > 0)
            assert rule_h(q, np.float32(n)[None, :], c, R, plane_constants(c, R, -3000.0))[0] or depth > 0.25
    assert 25 <= claimed <= 33 and lit_if_claimed >= 12
