"""The shadow-visibility query of the render loop, ray by ray (mcpt_debug_shadow: the product's own launch of k_trace_shadow, with
k_retrace_shadow behind it for trees that use the retry flavour of the traversal stack, on a queue the call fills as k_direct would).

Reference: the rule of Scene.cpp:74-75 -- a light sample is visible iff the CLOSEST hit of the ray lies within EPSILON of the light
distance.  The oracle's closest hit t is a double the device reproduces bit for bit (tests/test_gpu_parity.py), so the expectation is
plain float64 arithmetic with no tolerance on the decision:

    visible_ref = (prim >= 0) & (abs(t - float64(dist)) < float64(float32(1e-4)))

`found` hints are truthful: an oracle scene of the emitting objects alone gives t_L for the same ray, and found = |t_L - dist| < EPSILON
restates k_direct's own test of the sampled light primitive.  Wherever visible_ref holds the hint is truthful too (the closest hit is
in the window).

Bounds: with the reference's tree and float nodes not one ray may differ.  Under every other tree a ray that grazes a box face within
float rounding can take another branch; the project's bound for such rays (test_cast_rays_parity) is max(3, n // 10000) and is used
here as it stands.  Every case prints its count, and every differing ray.
"""
import numpy as np
import pytest
from conftest import TREES
from chain_scene import chain_scene as _chain

pytestmark = pytest.mark.gpu

EPS = np.float64(np.float32(1e-4))
N = 20000


def visible_ref(t, prim, dist):
    return (prim >= 0) & (np.abs(t - np.asarray(dist, np.float32).astype(np.float64)) < EPS)


def _scene(pkg, name):
    return pkg.scenes.cornell_demo(64, 64, 4) if name == "cornell_demo" else pkg.scenes.chess_scene(width=160, height=90, spp=4)


def lights_only(pkg, sd):
    """The description of sd's emitting objects alone."""
    emits = (sd.materials["emission"] > 0).any(axis=1)
    tris, objs, first = [], [], 0
    for o in sd.objects:
        if not emits[o["material"]]:
            continue
        o = o.copy()
        if o["kind"] == 0:
            tris.append(sd.triangles[int(o["first_tri"]):int(o["first_tri"]) + int(o["n_tri"])])
            o["first_tri"] = first
            first += int(o["n_tri"])
        objs.append(o)
    return pkg.scenes.SceneData(triangles=np.concatenate(tris), materials=sd.materials.copy(), objects=np.stack(objs),
                                background=sd.background, env_pixels=None, camera=sd.camera, rr_rate=sd.rr_rate)


def _unit(v):
    """float32 direction and float32 length of v, as k_direct forms them (normalized(x_l - q), norm(x_l - q))."""
    v = v.astype(np.float32)
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(np.float32)).astype(np.float32)
    return (v / n[:, None]).astype(np.float32), n


def first_hits(os_, sd, n, seed):
    """n camera rays that hit something: (o, d, t) with t the oracle's closest hit."""
    rng = np.random.default_rng(seed)
    W, H = int(sd.camera["width"]), int(sd.camera["height"])
    pix = rng.integers(0, W * H, size=4 * n).astype(np.uint32)
    smp = rng.integers(0, 64, size=4 * n).astype(np.uint32)
    o, d = os_.camera_rays(pix, smp, seed=7)
    t, prim = os_.intersect(o, d)
    k = np.flatnonzero(prim >= 0)[:n]
    assert len(k) == n
    return o[k], d[k], t[k]


def rays_production(fh, light_points):
    """Set a: from camera-ray first hits, pulled back along the camera ray by 1 - 1e-3, to sampled light points."""
    o, d, t = fh
    q = (o + d * (t * (1.0 - 1e-3))[:, None].astype(np.float32)).astype(np.float32)
    ws, dist = _unit(light_points - q)
    return q, ws, dist


def rays_window_edges(os_, fh, seed):
    """Set b: dist swept across the window around the closest hit t_c of 1350 rays: float32(t_c) + k EPSILON, and the float32 neighbours
    of float32(t_c +- EPSILON)."""
    rng = np.random.default_rng(seed)
    o, d, t = (a[:900] for a in fh)
    d2 = rng.normal(size=(450, 3)).astype(np.float32)  # second-bounce-like rays from the hit points
    d2, _ = _unit(d2)
    p = (o[:450] + d[:450] * (t[:450] * (1.0 - 1e-3))[:, None].astype(np.float32)).astype(np.float32)
    o, d = np.concatenate([o, p]), np.concatenate([d, d2])
    t, prim = os_.intersect(o, d)
    k = np.flatnonzero((prim >= 0) & (t > 1.0))
    o, d, t = o[k], d[k], t[k]
    tc = t.astype(np.float32)
    eps = np.float32(1e-4)
    cols = [(tc + np.float32(m) * eps).astype(np.float32) for m in (0, 0.5, -0.5, 0.9, -0.9, 1.1, -1.1, 2, -2, 100, -100)]
    for edge in ((t + EPS).astype(np.float32), (t - EPS).astype(np.float32)):
        cols += [np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))]
    m = len(cols)
    return np.repeat(o, m, axis=0), np.repeat(d, m, axis=0), np.stack(cols, axis=1).reshape(-1).astype(np.float32)


def degenerate_dirs(rng, n):
    """n directions of four kinds in turn: one zero component, two (an axis), all zero, a -0.0 component."""
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d, _ = _unit(d)
    kind = np.arange(n) % 4
    one = np.flatnonzero(kind == 0)
    d[one, rng.integers(0, 3, size=len(one))] = 0.0  # (not renormalised: the reference never normalises inside intersect)
    two = np.flatnonzero(kind == 1)
    d[two] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=len(two))] * rng.choice([-1, 1], size=(len(two), 1)).astype(np.float32)
    d[kind == 2] = 0.0
    neg = np.flatnonzero(kind == 3)
    d[neg, rng.integers(0, 3, size=len(neg))] = -0.0
    return d


def rays_degenerate(os_, sd, fh, seed):
    """Set c: zero direction components (the NaN-faithful slab chain in window and occluder mode), in runs of 100 -- whole waves of them
    -- in the first half and scattered among plain rays in the second.  Even origins as test_intersect_degenerate_directions: in and
    around the scene, some exactly on its bounding planes; odd origins just off the surfaces the camera sees."""
    rng = np.random.default_rng(seed)
    n = len(fh[2])
    lo = np.minimum(sd.triangles["v0"].min(axis=0), np.minimum(sd.triangles["v1"].min(axis=0), sd.triangles["v2"].min(axis=0)))
    hi = np.maximum(sd.triangles["v0"].max(axis=0), np.maximum(sd.triangles["v1"].max(axis=0), sd.triangles["v2"].max(axis=0)))
    o = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3)).astype(np.float32)
    for a in range(3):
        o[a::11, a] = lo[a]
        o[a + 3::11, a] = hi[a]
    o[1::2] = (fh[0] + fh[1] * (fh[2] * (1.0 - 1e-3))[:, None].astype(np.float32)).astype(np.float32)[1::2]
    d, _ = _unit(rng.uniform(lo, hi, size=(n, 3)).astype(np.float32) - o)  # the plain rays: aimed at points inside the scene's box
    half = n // 2
    runs = np.flatnonzero((np.arange(half) // 100) % 2 == 0)  # runs of 100 degenerate rays, 100 plain ones between them
    d[runs] = degenerate_dirs(rng, len(runs))
    scattered = half + np.flatnonzero(rng.random(n - half) < 0.15)
    d[scattered] = degenerate_dirs(rng, len(scattered))
    t, prim = os_.intersect(o, d)
    hit = prim >= 0
    tc = np.where(hit, t, 0.0)
    u = rng.random(n)
    # a third at the closest hit (visible), a third beyond it (occluded), the rest anywhere
    dist = np.where(hit & (u < 1 / 3), tc, np.where(hit & (u < 2 / 3), tc * 1.5, rng.uniform(1.0, float(np.linalg.norm(hi - lo)), size=n)))
    dist = np.maximum(dist, 1e-3).astype(np.float32)
    return o, d, dist


def rays_leaving_and_long(os_, sd, fh, seed):
    """Set d: rays that leave the scene (nothing in the window: invisible), and rays whose dist is 10^3 scene extents, whose pruning
    margin is dominated by dist * 1e-4."""
    rng = np.random.default_rng(seed)
    o, d, t = fh
    n = len(t)
    p = (o + d * (t * (1.0 - 1e-3))[:, None].astype(np.float32)).astype(np.float32)
    lo = np.minimum(sd.triangles["v0"].min(axis=0), np.minimum(sd.triangles["v1"].min(axis=0), sd.triangles["v2"].min(axis=0)))
    hi = np.maximum(sd.triangles["v0"].max(axis=0), np.maximum(sd.triangles["v1"].max(axis=0), sd.triangles["v2"].max(axis=0)))
    extent = float(np.linalg.norm(hi - lo))
    half = n // 2
    # leaving: back towards the camera side, from where every first hit was seen (straight back where the scattered direction hits)
    out_d, _ = _unit((-d[:half] + rng.normal(0, 0.2, size=(half, 3))).astype(np.float32))
    out_d = np.where((os_.intersect(p[:half], out_d)[1] >= 0)[:, None], -d[:half], out_d).astype(np.float32)
    out_dist = rng.uniform(0.05 * extent, 3.0 * extent, size=half).astype(np.float32)
    # long: from the same kind of point towards a light sample 10^3 extents away, in any direction (the origin stays at scene scale, as
    # every origin of the render loop does)
    far_o = p[half:]
    far_d, _ = _unit(rng.normal(size=(n - half, 3)).astype(np.float32))
    far_dist = (np.float32(1e3 * extent) * rng.uniform(1.0, 2.0, size=n - half)).astype(np.float32)
    return np.concatenate([p[:half], far_o]), np.concatenate([out_d, far_d]), np.concatenate([out_dist, far_dist]), half, extent


_SETS = {}


def ray_sets(pkg, oracle, hs, name):
    """The four ray sets of a scene with their expectations, computed once per scene and shared (read-only) by every tree and flavour:
    {set: (o, d, dist, found hints, visible_ref)}.  hs: any HipScene of the scene (for sample_light, which does not depend on the tree)."""
    if name in _SETS:
        return _SETS[name]
    sd = _scene(pkg, name)
    os_, ol = oracle.OracleScene(sd), oracle.OracleScene(lights_only(pkg, sd))
    x_l = hs.sample_light(np.random.default_rng(101).random((N, 4)).astype(np.float32))[:, :3]
    fh = first_hits(os_, sd, N, 31)
    sets = {}

    def add(key, o, d, dist, hints):
        t, prim = os_.intersect(o, d)
        ref = visible_ref(t, prim, dist)
        if hints == "lights":
            t_l, p_l = ol.intersect(o, d)
            found = visible_ref(t_l, p_l, dist)
        else:
            found = ref.copy()
        for a in (o, d, dist, found, ref, t, prim):
            a.setflags(write=False)
        sets[key] = (o, d, dist, found, ref, t, prim)

    add("a", *rays_production(fh, x_l), hints="lights")
    add("b", *rays_window_edges(os_, fh, 32), hints="ref")
    add("c", *rays_degenerate(os_, sd, fh, 33), hints="ref")
    o, d, dist, half, extent = rays_leaving_and_long(os_, sd, fh, 34)
    add("d", o, d, dist, hints="ref")
    sets["d_half"], sets["extent"] = half, extent
    _check_set_properties(sets, name)
    _SETS[name] = sets
    return sets


def class_shares(found, ref):
    """Shares of the three classes of set a: found and visible, found and occluded, not found."""
    return (found & ref).mean(), (found & ~ref).mean(), (~found).mean()


def _compare(capsys, label, got, s, found, bound):
    o, d, dist, _, ref, t, prim = s
    bad = np.flatnonzero(got != ref)
    with capsys.disabled():
        print("\n[shadow query] %s: %d of %d rays differ from the oracle (visible %.3f)" % (label, len(bad), len(ref), ref.mean()))
        for i in bad[:20]:
            print("    ray %d: o %s d %s dist %r t_c %r prim %d found %d: device %d, oracle %d"
                  % (i, o[i].tolist(), d[i].tolist(), float(dist[i]), float(t[i]), int(prim[i]), int(found[i]), int(got[i]), int(ref[i])))
    assert len(bad) <= bound, (label, len(bad), bound)


def _run_sets(capsys, pkg, oracle, hs, name, label, exact):
    sets = ray_sets(pkg, oracle, hs, name)
    for key in "abcd":
        s = sets[key]
        o, d, dist, found, ref = s[:5]
        bound = 0 if exact else max(3, len(ref) // 10000)
        zeros = np.zeros(len(ref), np.uint8)
        _compare(capsys, "%s %s set %s, no hints" % (name, label, key), hs.shadow_visible(o, d, dist), s, zeros, bound)
        _compare(capsys, "%s %s set %s, truthful hints" % (name, label, key), hs.shadow_visible(o, d, dist, found=found), s, found, bound)
    return sets


def _check_set_properties(sets, name):
    """What the sets must contain to test anything (all from the oracle alone)."""
    _, _, _, found, ref = sets["a"][:5]
    shares = class_shares(found, ref)
    assert min(shares) >= 0.05, (name, shares)
    o, d, dist, _, ref_b = sets["b"][:5]
    assert 0.3 < ref_b.mean() < 0.7  # the sweep straddles the window: about half inside
    assert (sets["d"][6][:sets["d_half"]] < 0).all() and not sets["d"][4][:sets["d_half"]].any()  # rays that leave the scene: nothing in any window
    assert (sets["d"][2][sets["d_half"]:] > 900 * sets["extent"]).all()
    dc = sets["c"][1]
    assert ((dc == 0).sum(axis=1) == 1).sum() > 500 and ((dc == 0).sum(axis=1) == 2).sum() > 500 and ((dc == 0).all(axis=1)).sum() > 500
    assert np.signbit(dc[dc == 0]).any()
    deg, ref_c, hit_c = (dc == 0).any(axis=1), sets["c"][4], sets["c"][6] >= 0
    assert (deg & ref_c).sum() > 200 and (deg & hit_c & ~ref_c).sum() > 200 and (~deg & ref_c).sum() > 200  # both outcomes, both kinds


@pytest.mark.parametrize("tree", TREES, ids=lambda t: "%s-q%s" % (t[0], t[1] or "auto"))
@pytest.mark.parametrize("name", ["cornell_demo", "chess"])
def test_shadow_query_under_every_tree(pkg, oracle, hip, name, tree, tree_env, capsys):
    tree_env(*tree)
    hs = hip.HipScene(_scene(pkg, name))
    _run_sets(capsys, pkg, oracle, hs, name, "%s/q%s" % (tree[0], tree[1] or "auto"), exact=tree == ("reference", "0"))


@pytest.mark.parametrize("quantise", [0, 1])
def test_shadow_query_instanced(pkg, oracle, hip, quantise, capsys):
    hs = hip.HipScene(_scene(pkg, "chess"), builder="sah", quantise=quantise, instancing=True)
    info = hs.info()
    assert info["n_instances"] > 0 and info["quantised"] == quantise
    _run_sets(capsys, pkg, oracle, hs, "chess", "sah instanced q%d" % quantise, exact=False)


@pytest.mark.parametrize("small", [True, False])
def test_shadow_query_lds_resident_and_not(pkg, oracle, hip, small, monkeypatch, capsys):
    if not small:
        monkeypatch.setenv("MCPT_SMALL_SCENE", "0")
    hs = hip.HipScene(_scene(pkg, "cornell_demo"))
    assert hs.info()["lds_resident"] == int(small)
    _run_sets(capsys, pkg, oracle, hs, "cornell_demo", "LDS-resident %d" % small, exact=False)


@pytest.mark.parametrize("name", ["cornell_demo", "chess"])
def test_shadow_query_retrace_in_the_checking_build(pkg, oracle, hip, hip_check, name, capsys):
    """The checking build runs the retry flavour with 4 LDS entries for every tree: most rays are decided by k_retrace_shadow."""
    hs = hip.HipScene(_scene(pkg, name), library=hip_check)
    assert b"checking build" in hs.L.mcpt_version()
    _run_sets(capsys, pkg, oracle, hs, name, "checking build", exact=False)


def test_shadow_query_deep_chain_product_retry(pkg, oracle, hip, capsys):
    """The product's own retry flavour (16 LDS entries, trees deeper than 24 levels): the chain scene of tests/test_gpu_lbvh.py under the
    linear BVH, rays along +z through the square, started between planes in the middle of the chain, with dist at the closest plane
    (visible), at planes behind it (occluded) and between planes (nothing in the window)."""
    n_tri = 36
    sd = _chain(pkg, n_tri)
    hs = hip.HipScene(sd, builder="lbvh")
    assert 24 < hs.info()["bvh_height"] <= 48
    rng = np.random.default_rng(41)
    planes = np.float64([0.01 * k for k in range(n_tri) if k % 3 < 2])  # (the triangles with k % 3 == 2 lie far away in z)
    start = rng.integers(0, len(planes) - 1, size=N)
    o = np.concatenate([rng.uniform(-0.9, -0.1, (N, 2)), (planes[start] - 0.004)[:, None]], axis=1).astype(np.float32)
    d = np.concatenate([rng.normal(0, 0.02, (N, 2)), np.ones((N, 1))], axis=1).astype(np.float32)
    d, _ = _unit(d)
    t, prim = oracle.OracleScene(sd).intersect(o, d)
    assert (prim >= 0).all()
    behind = (planes[np.minimum(start + rng.integers(1, 6, size=N), len(planes) - 1)] - o[:, 2].astype(np.float64)) / d[:, 2].astype(np.float64)
    u = rng.random(N)
    dist = np.where(u < 0.4, t, np.where(u < 0.8, behind, t + 0.005)).astype(np.float32)
    ref = visible_ref(t, prim, dist)
    assert 0.3 < ref.mean() < 0.5
    s = (o, d, dist, ref, ref, t, prim)
    bound = max(3, N // 10000)
    _compare(capsys, "chain lbvh (retry flavour), no hints", hs.shadow_visible(o, d, dist), s, np.zeros(N, np.uint8), bound)
    # a hit in the window exists wherever dist sits on a plane (first two classes): truthful hints beyond visible_ref
    found = ref | (u >= 0.4) & (u < 0.8)
    _compare(capsys, "chain lbvh (retry flavour), truthful hints", hs.shadow_visible(o, d, dist, found=found), s, found, bound)


def _placements(n, rng):
    return {"default": None, "one shard": np.full(n, 7, np.int32), "odd shards": (2 * (np.arange(n) % 16) + 1).astype(np.int32),
            "last shard": np.full(n, 31, np.int32), "random": rng.integers(0, 32, size=n).astype(np.int32)}


def test_queue_layout_does_not_matter(pkg, oracle, hip, tree_env, capsys):
    """Set e: the same rays under every placement in the sharded queue -- one shard, odd shards only, the last shard, random shards; found
    entries only, window entries only, both meeting in the middle of a region filled to exactly R entries (n = 64 and 2048 in one shard:
    the capacity is the smallest that holds the fullest shard); list 0 and 1 -- give the same array, and it equals the oracle's."""
    tree_env("reference", "0")
    hs = hip.HipScene(_scene(pkg, "cornell_demo"))
    o, d, dist, found, ref, t, prim = ray_sets(pkg, oracle, hs, "cornell_demo")["a"]
    rng = np.random.default_rng(51)
    calls = 0
    for n in (1, 63, 64, 65, 2047, 2048, 2049):
        k = rng.permutation(N)[:n]
        for hints, sel in (("mixed", k), ("found only", k[found[k]]), ("window only", k)):
            f = np.zeros(len(sel), np.uint8) if hints == "window only" else found[sel].astype(np.uint8)
            if len(sel) == 0:
                continue
            for label, shard in _placements(len(sel), rng).items():
                for lst in (0, 1):
                    got = hs.shadow_visible(o[sel], d[sel], dist[sel], found=f, shard=shard, list=lst)
                    assert np.array_equal(got, ref[sel]), (n, hints, label, lst, int((got != ref[sel]).sum()))
                    calls += 1
    with capsys.disabled():
        print("\n[shadow query] queue layout: %d placements of up to 2049 rays, 0 rays differ" % calls)


def test_queue_is_strided_with_one_workgroup_per_cu(pkg, oracle, hip, tree_env, monkeypatch, capsys):
    """MCPT_SHADOW_GRID_PER_CU=1 caps the grid at 256 workgroups of 256 lanes: a queue of 80 000 entries makes them stride."""
    tree_env("reference", "0")
    monkeypatch.setenv("MCPT_SHADOW_GRID_PER_CU", "1")
    hs = hip.HipScene(_scene(pkg, "cornell_demo"))
    o, d, dist, found, ref, t, prim = ray_sets(pkg, oracle, hs, "cornell_demo")["a"]
    o4, d4, dist4, found4, ref4 = np.tile(o, (4, 1)), np.tile(d, (4, 1)), np.tile(dist, 4), np.tile(found, 4), np.tile(ref, 4)
    assert len(ref4) > 256 * 256
    rng = np.random.default_rng(52)
    for label, shard in (("default", None), ("random", rng.integers(0, 32, size=len(ref4)).astype(np.int32))):
        got = hs.shadow_visible(o4, d4, dist4, found=found4, shard=shard, list=1)
        bad = int((got != ref4).sum())
        with capsys.disabled():
            print("\n[shadow query] strided queue, %s placement: %d of %d rays differ" % (label, bad, len(ref4)))
        assert bad == 0


def test_argument_checks(pkg, hip):
    import ctypes as C
    hs = hip.HipScene(pkg.scenes.cornell_rc(32, 32, 1))
    L = hs.L
    n = 4
    o, d = np.zeros((n, 3), np.float32), np.tile(np.float32([0, 0, 1]), (n, 1))
    dist, found, shard, vis = np.ones(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(h=hs.h, lst=0, n=n, o=o, d=d, dist=dist, found=found, shard=shard, vis=vis):
        return L.mcpt_debug_shadow(h, lst, n, *[None if a is None else p(a) for a in (o, d, dist, found, shard, vis)])

    assert call() == 0 and call(shard=None) == 0 and call(lst=1) == 0
    assert call(n=0) == 0 and call(n=0, o=None, d=None, dist=None, found=None, shard=None, vis=None) == 0
    for kw in (dict(h=None), dict(o=None), dict(d=None), dict(dist=None), dict(found=None), dict(vis=None), dict(lst=-1), dict(lst=2), dict(n=-1),
               dict(n=(1 << 22) + 1), dict(shard=np.int32([0, 32, 0, 0])), dict(shard=np.int32([0, 0, -1, 0])), dict(found=np.uint8([0, 1, 2, 0])),
               dict(dist=np.float32([1, 0, 1, 1])), dict(dist=np.float32([1, 1, -1, 1])), dict(dist=np.float32([1, 1, 1, np.inf])),
               dict(dist=np.float32([np.nan, 1, 1, 1]))):
        assert call(**kw) == 1, kw
        assert b"mcpt_debug_shadow" in L.mcpt_last_error()
    with pytest.raises(hip.McptError):
        hs.shadow_visible(o, d, dist, list=3)
