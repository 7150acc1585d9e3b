"""A plain restatement of the two device tree builders of csrc/mcpt_lbvh.hip (numpy and python loops), and the scenes it is compared on.

build_model(sd, "lbvh" | "ploc") returns what HipScene.dump_bvh() returns for a scene created with that builder -- (info, boxes[n-1,12],
children[n-1,2], None) -- with the device's node numbering, so trees are compared with array_equal, not up to isomorphism:

  primitive boxes  k_prim_boxes: slot i < n_tri is triangle i (box = min / max of the stored vertices); the slots after them are the
                   spheres in object order, box c -+ r, primitive id n_tri + OBJECT index (not the sphere's ordinal)
  Morton codes     k_morton, in float32: c = 0.5f*mn + 0.5f*mx, inv = 1.0f / (cmax - cmin) or 0 for a zero extent,
                   q = trunc(min(u * 2^21, 2^21 - 1)), 21 bits per axis spread to every third bit, x in the highest position
  sort             stable by code (the radix sort of (code, slot) pairs keeps equal codes in slot order)
  lbvh             k_hierarchy (Karras 2012: delta with the 64 + clz(i ^ j) rule for equal codes, range and split search); inner node i is
                   node i, the root is node 0; child boxes are exact min / max unions; a leaf below d inner nodes has depth d + 1
  ploc             k_ploc_nn / k_ploc_flags / scan / k_ploc_emit round by round: radius = clamp(MCPT_PLOC_RADIUS, 1, 64), node index =
                   node_base + exclusive-scan rank, left = the smaller-index cluster, levels = 1 + max.  Only the case without a host-built
                   top (n / 16 < 64) is modelled.  info["rounds"] is the number of rounds (not part of the ABI: the model's figure only).

Exactness.  The only arithmetic of the builders whose result could depend on what the device compiler contracts into FMAs is
union_half_area = dx*dy + (dy*dz + dz*dx).  Every vertex, centre and radius of the scenes below lies on the integer grid in [0, 1024):
extents stay below 2^10, their products below 2^20 and the sum below 2^22, all exact in float32 whether fused or not; centroids are
half-integers (exact); (c - cmin) is exact, and the one rounding of (c - cmin) * inv is the same IEEE multiplication on both sides.  So
the model equals the device bit for bit on these scenes, and only on such scenes is that claimed."""
import numpy as np

f32 = np.float32
KMAX_RADIUS = 64


# --------------------------------------------------------------------------- primitives, codes, order
def prim_boxes(sd):
    """-> (pmin[n,3], pmax[n,3], prim_id[n]) in slot order (k_prim_boxes)."""
    tri = sd.triangles
    n_tri = len(tri)
    v = np.stack([tri["v0"], tri["v1"], tri["v2"]], axis=1).astype(f32).reshape(n_tri, 3, 3)
    mn, mx, ids = [v.min(axis=1)], [v.max(axis=1)], list(range(n_tri))
    for oi, o in enumerate(sd.objects):
        if int(o["kind"]) == 1:
            c, r = o["center"].astype(f32), f32(o["radius"])
            mn.append((c - r)[None])
            mx.append((c + r)[None])
            ids.append(n_tri + oi)
    return np.concatenate(mn).astype(f32), np.concatenate(mx).astype(f32), np.array(ids, np.int32)


def spread21(x):
    """21 bits -> every third bit (the device's mask ladder), on python ints."""
    x &= 0x1fffff
    x = (x | x << 32) & 0x1f00000000ffff
    x = (x | x << 16) & 0x1f0000ff0000ff
    x = (x | x << 8) & 0x100f00f00f00f00f
    x = (x | x << 4) & 0x10c30c30c30c30c3
    x = (x | x << 2) & 0x1249249249249249
    return x


def morton_codes(pmin, pmax):
    """-> list of python ints (63-bit codes), float32 arithmetic as in k_prim_boxes / build_lbvh_device / k_morton."""
    c = f32(0.5) * pmin + f32(0.5) * pmax
    cmin, cmax = c.min(axis=0), c.max(axis=0)
    ext = (cmax - cmin).astype(f32)
    inv = np.zeros(3, f32)
    inv[ext > 0] = f32(1.0) / ext[ext > 0]
    u = ((c - cmin).astype(f32) * inv).astype(f32)
    u = np.minimum(np.maximum(u, f32(0)), f32(1))
    q = np.minimum(u * f32(2097152.0), f32(2097151.0)).astype(f32)
    q = np.trunc(q).astype(np.int64)
    return [(spread21(int(x)) << 2) | (spread21(int(y)) << 1) | spread21(int(z)) for x, y, z in q]


def sorted_order(codes):
    return np.argsort(np.array(codes, dtype=np.uint64), kind="stable")


# --------------------------------------------------------------------------- LBVH
def _delta(keys, n, i, j):
    if j < 0 or j >= n:
        return -1
    a, b = keys[i], keys[j]
    if a == b:
        return 64 + (32 - (i ^ j).bit_length())
    return 64 - (a ^ b).bit_length()


def lbvh_hierarchy(keys):
    """k_hierarchy: -> child[n-1][2] in sorted-leaf numbering (>= 0 inner node, < 0: ~sorted position)."""
    n = len(keys)
    child = []
    for i in range(n - 1):
        d = 1 if _delta(keys, n, i, i + 1) - _delta(keys, n, i, i - 1) >= 0 else -1
        dmin = _delta(keys, n, i, i - d)
        lmax = 2
        while _delta(keys, n, i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if _delta(keys, n, i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = _delta(keys, n, i, j)
        s, t = 0, l
        while True:
            t = (t + 1) >> 1
            if _delta(keys, n, i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + (-1 if d < 0 else 0)
        lo, hi = min(i, j), max(i, j)
        child.append((~gamma if lo == gamma else gamma, ~(gamma + 1) if hi == gamma + 1 else gamma + 1))
    return child


def _lbvh(pmin, pmax, prim_id, order, keys):
    n = len(order)
    child = lbvh_hierarchy(keys)
    boxes, children = np.zeros((n - 1, 12), f32), np.zeros((n - 1, 2), np.int32)
    nmin, nmax, done = np.zeros((n - 1, 3), f32), np.zeros((n - 1, 3), f32), [False] * (n - 1)
    height, stack = 0, [(0, 1)]  # (inner node, number of inner nodes from the root down to it)
    while stack:
        node, depth = stack[-1]
        pending = [c for c in child[node] if c >= 0 and not done[c]]
        if pending:
            stack.extend((c, depth + 1) for c in pending)
            continue
        stack.pop()
        for side, c in enumerate(child[node]):
            if c < 0:
                p = order[~c]
                mn, mx = pmin[p], pmax[p]
                children[node, side] = ~int(prim_id[p])
                height = max(height, depth + 1)
            else:
                mn, mx = nmin[c], nmax[c]
                children[node, side] = c
            boxes[node, 6 * side:6 * side + 3], boxes[node, 6 * side + 3:6 * side + 6] = mn, mx
        nmin[node] = np.minimum(boxes[node, 0:3], boxes[node, 6:9])
        nmax[node] = np.maximum(boxes[node, 3:6], boxes[node, 9:12])
        done[node] = True
    assert all(done), "the hierarchy does not reach every inner node from node 0"
    return {"root": 0, "stack_entries": height, "root_min": nmin[0].tolist(), "root_max": nmax[0].tolist()}, boxes, children


# --------------------------------------------------------------------------- PLOC
def union_half_area(amin, amax, bmin, bmax):
    d = (np.maximum(amax, bmax) - np.minimum(amin, bmin)).astype(f32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dy + (dy * dz + dz * dx)).astype(f32)


def ploc_nearest(bmin, bmax, radius, tie="paired"):
    """k_ploc_nn: the neighbour of every cluster within +-radius whose union has the smallest half area.  Equal areas (tie="paired", the
    device's rule): the smaller |i - j|, then the pair whose smaller index is even, then the smaller min(i, j) -- a key of the unordered
    pair, so the best pair of the array is mutual, and clusters with equal boxes pair up (2k, 2k+1).  tie="smaller": the rule the kernel
    had before (the smaller index), kept to state what it did to coincident primitives."""
    m = len(bmin)
    idx = np.arange(m)
    best, bj, btie = np.full(m, np.inf, f32), np.full(m, -1, np.int64), np.zeros(m, np.int64)
    for d in range(-radius, radius + 1):  # ascending j, as on the device
        if d == 0:
            continue
        j = idx + d
        valid = (j >= 0) & (j < m)
        jc = np.clip(j, 0, m - 1)
        a = union_half_area(bmin, bmax, bmin[jc], bmax[jc])
        lo = np.minimum(idx, jc)
        t = (np.int64(abs(d)) << 33) | ((lo & 1).astype(np.int64) << 32) | lo.astype(np.int64)
        better = (bj < 0) | (a < best)
        if tie == "paired":
            better |= (a == best) & (t < btie)
        better &= valid
        best, bj, btie = np.where(better, a, best), np.where(better, j, bj), np.where(better, t, btie)
    return bj


def _ploc(pmin, pmax, prim_id, order, radius, tie):
    n = len(order)
    assert n // 16 < 64, "only the case without a host-built top is modelled"
    radius = min(max(int(radius), 1), KMAX_RADIUS)
    bmin, bmax = pmin[order].copy(), pmax[order].copy()
    ref, lev = [~int(prim_id[p]) for p in order], [1] * n
    boxes, children = np.zeros((n - 1, 12), f32), np.zeros((n - 1, 2), np.int32)
    m, node_base, rounds = n, 0, 0
    while m > 1:
        nn = ploc_nearest(bmin, bmax, radius, tie)
        idx = np.arange(m)
        mutual = (nn >= 0) & (nn[np.clip(nn, 0, m - 1)] == idx)
        stays, creates = ~(mutual & (idx > nn)), mutual & (idx < nn)
        pos, rank = np.cumsum(stays) - stays, np.cumsum(creates) - creates  # exclusive scans
        m2, made = int(stays.sum()), int(creates.sum())
        assert m2 < m and made > 0, "no mutual pair: the tie rule is not a function of the unordered pair"
        nbmin, nbmax, nref, nlev = np.zeros((m2, 3), f32), np.zeros((m2, 3), f32), [0] * m2, [0] * m2
        for i in range(m):
            if not stays[i]:
                continue
            mn, mx, r, lv = bmin[i], bmax[i], ref[i], lev[i]
            if creates[i]:
                j = int(nn[i])
                node = node_base + int(rank[i])
                boxes[node] = np.concatenate([mn, mx, bmin[j], bmax[j]])
                children[node] = (r, ref[j])
                mn, mx, r, lv = np.minimum(mn, bmin[j]), np.maximum(mx, bmax[j]), node, 1 + max(lv, lev[j])
            nbmin[pos[i]], nbmax[pos[i]], nref[pos[i]], nlev[pos[i]] = mn, mx, r, lv
        bmin, bmax, ref, lev, m = nbmin, nbmax, nref, nlev, m2
        node_base += made
        rounds += 1
    assert node_base == n - 1
    return {"root": ref[0], "stack_entries": lev[0], "root_min": bmin[0].tolist(), "root_max": bmax[0].tolist(), "rounds": rounds}, boxes, children


def build_model(sd, builder, ploc_radius=16, tie="paired"):
    """-> (info, boxes, children, None) as HipScene(sd, builder=builder).dump_bvh() returns them (no quantised boxes: check_tree covers those)."""
    pmin, pmax, prim_id = prim_boxes(sd)
    assert len(prim_id) >= 2
    keys = morton_codes(pmin, pmax)
    order = sorted_order(keys)
    keys = [keys[p] for p in order]
    if builder == "lbvh":
        info, boxes, children = _lbvh(pmin, pmax, prim_id, order, keys)
    elif builder == "ploc":
        info, boxes, children = _ploc(pmin, pmax, prim_id, order, ploc_radius, tie)
    else:
        raise ValueError(builder)
    info["n_nodes"] = len(prim_id) - 1
    return info, boxes, children, None


# --------------------------------------------------------------------------- scenes on the integer grid in [0, 1024)
def _scene(pkg, meshes_and_spheres):
    """meshes_and_spheres: a list of [k,3,3] vertex arrays (a mesh) and (centre, radius) tuples (a sphere), in object order."""
    base = pkg.scenes.cornell_rc(32, 32, 1)
    tris, objs = [], []
    for item in meshes_and_spheres:
        o = np.zeros((), dtype=base.objects.dtype)
        if isinstance(item, tuple):
            o["kind"], o["material"], o["center"], o["radius"] = 1, 0, np.asarray(item[0], f32), f32(item[1])
        else:
            v = np.asarray(item, f32)
            o["kind"], o["material"], o["first_tri"], o["n_tri"] = 0, 0, sum(len(t) for t in tris), len(v)
            tris.append(v)
        objs.append(o)
    v = np.concatenate(tris)
    assert (v == np.round(v)).all() and v.min() >= 0 and v.max() < 1024
    tri = np.zeros(len(v), dtype=base.triangles.dtype)
    tri["v0"], tri["v1"], tri["v2"] = v[:, 0], v[:, 1], v[:, 2]
    return pkg.scenes.SceneData(triangles=tri, materials=base.materials[:1].copy(), objects=np.stack(objs), background=base.background,
                                env_pixels=None, camera=base.camera, rr_rate=base.rr_rate)


def _random_triangles(n, seed, lo=8, hi=1016, planar_y=None):
    """n triangles with integer vertices within 4 cells of an integer corner, none of zero area."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 3, 3), f32)
    for k in range(n):
        while True:
            v0 = rng.integers(lo, hi, 3)
            v = np.stack([v0, v0 + rng.integers(-4, 5, 3), v0 + rng.integers(-4, 5, 3)])
            if planar_y is not None:
                v[:, 1] = planar_y
            if np.cross(v[1] - v[0], v[2] - v[0]).any():
                break
        out[k] = v
    return out


def _box_triangle(lo, size):
    """A triangle whose box is exactly lo .. lo + size on every axis."""
    x, y, z = lo
    s = size
    return [[x, y, z], [x + s, y, z + s], [x, y + s, z + s]]


SIZES = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)
IDENTICAL = (8, 49, 64, 300)


def case_scene(pkg, name):
    kind, _, arg = name.partition("-")
    if kind == "random":      # n random small triangles
        return _scene(pkg, [_random_triangles(int(arg), seed=100 + int(arg))])
    if kind in ("nested", "nestedsorted"):  # one centroid, different boxes: triangle k has the box centre -+ k, in its own plane
        # "nested": in a fixed shuffled order.  In order of size ("nestedsorted": the model only, never given to the device) every cluster's
        # smallest union is with the next smaller one, only the two smallest are mutual, and PLOC's tree is a chain of n levels whatever the
        # tie rule -- deeper than the traversal stack from n = 49 on.  Shuffled, n = 65 gives 43 levels (the retry flavour of the stack).
        ks = np.arange(1, int(arg) + 1)
        if kind == "nested":
            ks = np.random.default_rng(2).permutation(ks)
        return _scene(pkg, [[_box_triangle((512 - int(k),) * 3, 2 * int(k)) for k in ks]])
    if kind == "identical":   # one triangle, n times: every box, centroid and code equal
        return _scene(pkg, [[[[500, 500, 500], [520, 500, 510], [500, 520, 510]]] * int(arg)])
    if kind == "planar":      # every vertex in the plane y = 7: the centroids have no extent on y
        return _scene(pkg, [_random_triangles(int(arg), seed=7, planar_y=7)])
    if kind == "row":         # equal tiles side by side along x
        return _scene(pkg, [[_box_triangle((16 + 8 * i, 40, 40), 8) for i in range(int(arg))]])
    if kind == "grid":        # equal tiles, arg x arg of them
        return _scene(pkg, [[_box_triangle((16 + 8 * i, 16 + 8 * j, 40), 8) for j in range(int(arg)) for i in range(int(arg))]])
    if kind == "mixed":       # mesh, sphere, mesh, sphere: sphere ids are n_tri + 1 and n_tri + 3; each sphere shares its box with a triangle
        a = np.concatenate([_random_triangles(5, seed=31, lo=80, hi=140), np.array([_box_triangle((96, 96, 96), 8)], f32)])
        b = np.concatenate([_random_triangles(3, seed=32, lo=80, hi=140), np.array([_box_triangle((120, 100, 90), 12)], f32)])
        return _scene(pkg, [a, ((100, 100, 100), 4), b, ((126, 106, 96), 6)])
    raise ValueError(name)


CASES = (["random-%d" % n for n in SIZES] + ["nested-65"] + ["identical-%d" % n for n in IDENTICAL]
         + ["planar-100", "row-64", "grid-16", "mixed"])
