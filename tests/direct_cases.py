"""The sampled direct term of include/mcpt.h (mcpt_query_direct) restated in numpy float32, its Philox keys, and the host composition
the GPU tests compare against.  Every product and sum below is one float32 operation in the written order, as csrc/mcpt_direct.h has it."""
import numpy as np

f32 = np.float32
EPS = f32(1e-4)
PI = f32(3.141592653589793)
FLT_MAX = f32(3.4028234663852886e38)
DIRECT_STREAM = 5
SAMPLE_COUNTS = (1, 3, 4, 32)


def dot3(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def samples(points, normals, rows):
    """points (n, 3), normals (n, 3), light rows (n, N, 10) -> q, ws (n, N, 3), dist (n, N), live (n, N) bool, contrib (n, N, 3)."""
    p = np.asarray(points, f32)[:, None, :]
    nf = np.asarray(normals, f32)[:, None, :]
    r = np.asarray(rows, f32)
    N = r.shape[1]
    with np.errstate(all="ignore"):
        q = np.broadcast_to(p + nf * EPS, r.shape[:2] + (3,)).astype(f32)
        w = r[..., 0:3] - q
        z = dot3(w, w)
        dist = np.sqrt(z)
        ws = np.where((z > 0)[..., None], w / np.sqrt(z)[..., None], w).astype(f32)
        cs, cl = dot3(ws, np.broadcast_to(nf, ws.shape)), dot3(-ws, r[..., 3:6])
        g = ((cs * cl) / (dist * dist)) / r[..., 9]
        live = (cs > 0) & (cl > 0) & (g <= FLT_MAX)
        contrib = np.where(live[..., None], (r[..., 6:9] * g[..., None]) / f32(N), f32(0)).astype(f32)
    return q, ws, dist.astype(f32), live, contrib


def fold(contrib, visible):
    """contrib (n, N, 3), visible (n, N) -> D (n, 3): the sum in sample order, then / pi."""
    c = np.asarray(contrib, f32)
    v = np.asarray(visible) != 0
    acc = np.zeros((c.shape[0], 3), f32)
    for j in range(c.shape[1]):
        acc = np.where(v[:, j, None], acc + c[:, j], acc).astype(f32)
    return (acc / PI).astype(f32)


def philox_uniforms(oracle, seed, pixel, sample, depth, block, stream):
    """One block through the oracle's Philox: key (seed, pixel), counter (sample, depth, block, stream) -> 4 uniforms."""
    o = oracle.philox([sample, depth, block, stream], [seed, pixel])
    return ((o >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


def special_rows():
    """(name, point, normal, light row) of the rows a sample must not survive, and one it must."""
    up = (0.0, 1.0, 0.0)
    down = (0.0, -1.0, 0.0)
    emit = (17.0, 12.0, 4.0)

    def row(x, n=down, e=emit, pdf=0.25):
        return tuple(x) + tuple(n) + tuple(e) + (pdf,)

    nan = float("nan")
    return [("live", (0, 0, 0), up, row((0.1, 1.0, 0.2))),
            ("cs <= 0", (0, 0, 0), down, row((0.1, 1.0, 0.2))),           # the point faces away
            ("cs == 0", (0, 0, 0), up, row((1.0, 1e-4, 0.0))),            # exactly in the tangent plane of q
            ("cl <= 0", (0, 0, 0), up, row((0.1, 1.0, 0.2), n=up)),       # the light faces away
            ("dist == 0", (0, 0, 0), up, row((0.0, 1e-4, 0.0))),          # x_l == q
            ("pdf == 0", (0, 0, 0), up, row((0.1, 1.0, 0.2), pdf=0.0)),
            ("no light", (0, 0, 0), up, (0.0,) * 10),                     # the row of an empty light table
            ("NaN normal", (0, 0, 0), (nan, 1.0, 0.0), row((0.1, 1.0, 0.2))),
            ("NaN light normal", (0, 0, 0), up, row((0.1, 1.0, 0.2), n=(0.0, nan, 0.0))),
            ("tiny pdf", (0, 0, 0), up, row((0.0, 1e-3, 0.0), e=(1e30, 1e30, 1e30), pdf=1e-38))]  # g overflows


def random_case(n, N, seed):
    """Points below a patch of light samples, a third of them facing away."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)).astype(f32)
    nf = rng.normal(size=(n, 3))
    nf = (nf / np.linalg.norm(nf, axis=1, keepdims=True)).astype(f32)
    rows = np.zeros((n, N, 10), f32)
    rows[..., 0:3] = rng.uniform(-1, 1, (n, N, 3))
    rows[..., 1] += 2.0
    nl = rng.normal(size=(n, N, 3))
    rows[..., 3:6] = nl / np.linalg.norm(nl, axis=2, keepdims=True)
    rows[..., 6:9] = rng.uniform(0, 20, (n, N, 3))
    rows[..., 9] = rng.uniform(0.1, 4, (n, N))
    return p, nf, rows


def host_direct(hip, hs, points, normals, N, seed=1, key_sample=0, pixels=None, key_samples=None):
    """The host composition of D at points (n, 3): rng_uniforms, then sample_light, then direct_samples, then intersect, then direct_fold.
    pixels / key_samples: per-point key words (default: the point's index and key_sample).  Returns (D (n, 3), the parts)."""
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    nf = np.ascontiguousarray(normals, f32).reshape(-1, 3)
    n = len(p)
    pixels = np.arange(n) if pixels is None else np.asarray(pixels)
    key_samples = np.full(n, key_sample) if key_samples is None else np.asarray(key_samples)
    if hs.info()["n_lights"] == 0:
        z = np.zeros((n, N), np.uint8)
        return np.zeros((n, 3), f32), {"live": z, "visible": z, "contrib": np.zeros((n, N, 3), f32)}
    u = np.zeros((n, N, 4), f32)
    blocks = np.arange(N)
    for i in range(n):
        u[i] = hip.rng_uniforms(seed, int(pixels[i]), int(key_samples[i]), 0, blocks, DIRECT_STREAM)
    rows = hs.sample_light(u.reshape(-1, 4)).reshape(n, N, 10)
    parts = hip.direct_samples(p, nf, rows)
    live = parts["live"].reshape(-1) != 0
    visible = np.zeros(n * N, bool)
    if live.any():
        t, prim = hs.intersect(parts["q"].reshape(-1, 3)[live], parts["ws"].reshape(-1, 3)[live])[:2]
        d = parts["dist"].reshape(-1)[live]
        visible[live] = (np.asarray(prim) >= 0) & (np.abs(np.asarray(t, np.float64) - d.astype(np.float64)) < np.float64(EPS))
    parts["visible"] = visible.reshape(n, N)
    parts["rows"] = rows
    return hip.direct_fold(parts["contrib"], parts["visible"]), parts


# ---------------------------------------------------------------- scenes and the closed form
def _quad(pkg, a, b, c, d):
    t = np.zeros(2, pkg.scenes.TRI_DTYPE)
    t["v0"], t["v1"], t["v2"] = [a, a], [b, c], [c, d]
    return t


TRIANGLE = np.array([(-0.5, 2.0, -0.4), (0.7, 2.0, -0.3), (0.1, 2.0, 0.8)], np.float64)  # normal (0, -1, 0)
TRIANGLE_EMISSION = (17.0, 12.0, 4.0)
BLOCKED, OPEN = (0.1, 0.0, 0.3), (3.0, 0.0, 3.0)  # floor points: every segment from BLOCKED to the triangle crosses y = 1 inside the blocker


def one_triangle_scene(pkg, blocker=False):
    """A floor at y = 0 facing up and ONE emitting triangle at y = 2 facing down: a mesh light of one triangle, so the biased pick of
    BVH.cpp:132 has nothing to choose.  blocker: a 0.7 x 0.7 quad at y = 1, facing up, that hides the whole triangle from BLOCKED."""
    s = pkg.scenes
    b = s._Builder()
    t = np.zeros(1, s.TRI_DTYPE)
    t["v0"][0], t["v1"][0], t["v2"][0] = TRIANGLE[0], TRIANGLE[1], TRIANGLE[2]
    b.add_mesh(t, b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=TRIANGLE_EMISSION)))
    white = b.material("floor", s.material_presets()["rough_white_conductor"])
    b.add_mesh(_quad(pkg, (-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6)), white)
    if blocker:
        b.add_mesh(_quad(pkg, (-0.25, 1, -0.1), (-0.25, 1, 0.6), (0.45, 1, 0.6), (0.45, 1, -0.1)), white)
    cam = s.make_camera(32, 24, 55, (0.3, 1.3, -4.5), (0.2, 0.2, 0.0))
    return b.finish(background=np.zeros(3, f32), camera=cam, rr_rate=0.8, spp=1, name="one_triangle")


def floor_points(n_side=4, half=1.5):
    """n_side^2 points of the floor with the normal (0, 1, 0)."""
    a = np.linspace(-half, half, n_side)
    x, z = np.meshgrid(a, a)
    p = np.stack([x.reshape(-1), np.zeros(x.size), z.reshape(-1)], axis=1).astype(f32)
    return p, np.tile(f32([0, 1, 0]), (len(p), 1))


def polygon_D(q, n, verts, emission):
    """Lambert's formula for the irradiance a uniform diffuse polygon sends to the point q with unit normal n, in float64, as
    D = E / pi:  E = L / 2 * |sum_k gamma_k (n . Gamma_k)|, gamma_k the angle the edge k subtends at q, Gamma_k the unit normal of
    the plane through q and the edge.  The polygon lies wholly above the tangent plane here, so no clipping is needed."""
    q, n, v = np.asarray(q, np.float64), np.asarray(n, np.float64), np.asarray(verts, np.float64)
    r = v - q
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    assert (r @ n > 0).all()
    s = 0.0
    for k in range(len(v)):
        a, b = r[k], r[(k + 1) % len(v)]
        c = np.cross(a, b)
        s += np.arccos(np.clip(a @ b, -1, 1)) * (n @ (c / np.linalg.norm(c)))
    return np.asarray(emission, np.float64) * abs(s) / 2 / np.pi


def closed_form_check(D, parts, p, nf, N):
    """Per point and channel the deviation of D from polygon_D in standard errors of the point's own mean, the errors computed from
    the per-sample contributions of the host composition (every sample of the open scene is visible, or contributes 0)."""
    x = parts["contrib"].astype(np.float64) * N * parts["visible"][..., None]  # per-sample estimates of E (emit * g), before / pi
    se = x.std(axis=1, ddof=1) / np.sqrt(N) / np.pi
    q = p.astype(np.float64) + nf.astype(np.float64) * float(EPS)
    want = np.array([polygon_D(q[i], nf[i], TRIANGLE, TRIANGLE_EMISSION) for i in range(len(p))])
    return np.abs(D.astype(np.float64) - want) / se, want, se
