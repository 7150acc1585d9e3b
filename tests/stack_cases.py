"""Shared by tests/test_stack_model_cpu.py, tests/test_gpu_stack_classes.py and tests/test_gpu_stack_live.py: scenes and rays that hold a
traversal stack at its LAST entry, and a float64 model of the walk that says so (no tests in this file).

Why.  A traversal kernel gets its per-lane stack by tree height (MCPT_STACK_DISPATCH, csrc/mcpt_stack_dispatch.h): 8 entries for
LDS-resident scenes (height <= 9), 16 up to height 17, kStkB = 20 up to 20, 24 up to 24, then the retry flavour (16 LDS entries, a
retrace with the 48-entry scratch stack), and nothing beyond 48.  A ray holds at most height - 1 entries, and in the plain classes a push
onto a full stack is dropped without a word.  tests/chain_scene.py fills such a stack, but the hit its +z rays return (triangle 0) is
tested from the parked leaf and never sits on the stack: with one entry too few the answer is the same.  Here the answer is the entry
pushed last.

flipped_chain(pkg, n, keep): chain_scene(pkg, n) with every triangle not in `keep` mirrored inside its own footprint (the right angle
moves to the opposite corner), so that every primitive box, Morton code and tree node is unchanged while a ray near (-0.9, -0.9) along +z
misses every flipped triangle and still passes through every box.  last_entry_case() walks the all-flipped scene, which nothing hits,
notes from which stack position every leaf was popped, and un-flips the leaf popped from position height - 2.

walk() restates descend / leaf_step / closest_update of csrc/mcpt_traverse.h over a dumped tree: the near child first, the far child
pushed, ties left first, pruning by `lim` with the margin |t| 1e-4 + 1e-2, the occluder rule t <= dist - kEps with its own limit.  It
walks the boxes the flavour under test traverses: the float boxes, or for quantised trees the dequantised ones of dump_bvh() as
tests/test_bvh_host.py::check_tree reads them (near / far is then decided by the quantised boxes and can differ from the float order,
which is why `keep` is chosen per flavour).  It visits a leaf when it reaches it, where the kernels park it and go on speculatively;
while nothing has been hit -- the case here until the very last leaf -- both test the same leaves from the same stack positions.

The slack (the one free number of these tests).  A ray COUNTS only if the model holds height - 1 entries, takes its answer from position
height - 2, and every decision on the way has slack:
  box decisions   every slab value t = (c - o) * inv carries the error bound REL * |c - o| * |inv| (quantised boxes, evaluated on the device
                  as q * (cell * inv) + (origin - o) * inv: REL * (|c - origin| + |origin - o|) * |inv|), REL = 2e-5.  Float32 rounding of the
                  two or three operations behind a slab value is at most 3 * 2^-24 = 1.8e-7 relative to those magnitudes, so the bound is over
                  100 times the rounding at whatever coordinate the value was computed, near the square or 4e5 away.  Entry and exit
                  distances are intervals under that bound; "the box is hit", "it is entered beyond lim", "it ends before the window" and
                  "the right child is nearer" must come out the same way over the whole interval.  Two values that the device computes
                  from the very same operands (the flat box of a planar triangle: tmin == tmax; two children that start at the same
                  plane: a tie, left first) are equal on the device bit for bit and count as decided.
  triangles       u, v, u + v stay BARY = 1e-3 away from 0 and 1 (a hit: all of them; a miss: at least one condition fails by that much),
                  |det| stays 1e-3 away from kEps and t 1e-3 away from 0 and from dist - kEps.  The float32 numerators of a triangle that
                  reaches 4e5 units carry a relative error of a few 1e-7 of the determinant: BARY is over 1000 times that.
The flipped chain meets this with the rays of ray_sets(): every one of them counts under the float boxes, and at least half must."""
import dataclasses
import math

import numpy as np
from bvh_model import build_model, prim_boxes
from chain_scene import chain_scene

f32, f64 = np.float32, np.float64
K_EPS = float(f32(1e-4))                    # kEps (csrc/mcpt_internal.h), a float widened to double
REL, BARY, T_ABS = 2e-5, 1e-3, 1e-3         # the slack: see the module docstring
NS = (10, 11, 18, 19, 21, 22, 25, 26, 49, 50)  # heights 9 | 10, 17 | 18, 20 | 21, 24 | 25, 48 | 49: both sides of every class border
BACKGROUND = (0.25, 0.5, 0.75)              # the chain scene is black and unlit: with a sky a path that hits differs from one that misses
FAR = float(2 ** 21)                        # a distance beyond every box of every chain here (the longest reaches 3 * 2^17)
INF = float("inf")


def lit(sd):
    """The same geometry under a constant sky, so that cast_rays, render and the sensors see whether a first hit was found."""
    return dataclasses.replace(sd, background=np.array(BACKGROUND, f32))


def flipped_chain(pkg, n, keep=()):
    """chain_scene(pkg, n) with the right angle of every triangle not in `keep` at the opposite corner of its footprint: (max x, max y),
    (min x, max y), (max x, min y), same z and the same winding.  No primitive box changes, which is asserted on the model's boxes."""
    sd = chain_scene(pkg, n)
    tri = sd.triangles.copy()
    for k in range(n):
        if k in keep:
            continue
        v = np.stack([tri["v0"][k], tri["v1"][k], tri["v2"][k]])
        mn, mx = v.min(0), v.max(0)
        assert mn[2] == mx[2]
        tri["v0"][k], tri["v1"][k], tri["v2"][k] = (mx[0], mx[1], mn[2]), (mn[0], mx[1], mn[2]), (mx[0], mn[1], mn[2])
    out = dataclasses.replace(sd, triangles=tri)
    a, b = prim_boxes(sd), prim_boxes(out)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "flipping a triangle changed a primitive box"
    return out


# --------------------------------------------------------------------------- quantised boxes
def dequantised(info, qboxes):
    """The float boxes the quantised flavour traverses: origin + q * cell in float32, as check_tree reads a dump.  -> (boxes[n,12], grid)"""
    o, c = np.array(info["q_origin"], f32), np.array(info["q_cell"], f32)
    deq = (o + qboxes.astype(f32).reshape(-1, 4, 3) * c).astype(f32)
    return deq.reshape(-1, 12), (o.astype(f64), c.astype(f64))


def quantise_model(info, boxes):
    """What the device builders make of float boxes (csrc/mcpt_lbvh.hip, k_quantise and the grid of build_lbvh_device): the grid spans the
    root box padded by ext * 1e-3 + 1e-6 with 65535 cells per axis, minima go down to floor(.) - 1, maxima up to ceil(.) + 1.  For the
    CPU runs of the model only: on the GPU the dumped boxes are walked.  -> (info with the grid, qboxes[n,12] uint16)"""
    rmn, rmx = np.array(info["root_min"], f32).astype(f64), np.array(info["root_max"], f32).astype(f64)
    ext = rmx - rmn
    pad = ext * 1e-3 + 1e-6
    origin, cell = (rmn - pad).astype(f32), ((ext + 2 * pad) / 65535.0).astype(f32)
    b = boxes.astype(f64).reshape(-1, 4, 3)
    rel = (b - origin.astype(f64)) / cell.astype(f64)
    q = np.where(np.arange(4)[None, :, None] % 2 == 0, np.floor(rel) - 1.0, np.ceil(rel) + 1.0)
    out = dict(info)
    out["q_origin"], out["q_cell"], out["quantised"] = origin.tolist(), cell.tolist(), 1
    return out, np.clip(q, 0, 65535).astype(np.uint16).reshape(-1, 12)


# --------------------------------------------------------------------------- the walk
@dataclasses.dataclass
class WalkResult:
    prim: int = -1          # closest: the primitive hit; occluder / window: the leaf that proved occlusion
    t: float = INF
    occluded: bool = False
    found: bool = False     # window: a hit within kEps of dist
    held: int = 0           # the largest number of entries on the stack
    pos: int = -1           # the stack position the deciding leaf was popped from (-1: it never was on the stack, or nothing decided)
    ok: bool = True         # every decision had slack
    dropped: int = 0        # pushes lost to `cap`
    tests: list = dataclasses.field(default_factory=list)  # (primitive, position it was popped from), in the order tested


def _triangle(sd, prim, o, d, res):
    """Triangle::getIntersection in float64 on the float32 edges of TriGeom -> t or None; clears res.ok without slack."""
    T = sd.triangles[prim]
    v0 = T["v0"].astype(f64)
    e1, e2 = (T["v1"] - T["v0"]).astype(f64), (T["v2"] - T["v0"]).astype(f64)
    pvec = np.cross(d, e2)
    det = float(e1 @ pvec)
    if abs(abs(det) - K_EPS) <= T_ABS:
        res.ok = False
    if abs(det) < K_EPS:
        return None
    tvec = o - v0
    qvec = np.cross(tvec, e1)
    u, v, t = float(tvec @ pvec) / det, float(d @ qvec) / det, float(e2 @ qvec) / det
    bary = (u, 1 - u, v, 1 - (u + v))
    if min(bary) >= 0 and t >= 0:
        if min(bary) <= BARY or t <= T_ABS:
            res.ok = False
        return t
    if not (min(bary) < -BARY or t < -T_ABS):
        res.ok = False
    return None


class _Box:
    """Entry and exit distance of one box as intervals under the slab error bound."""

    def __init__(self, mn, mx, o, inv, grid):
        self.nan = False
        lo, hi = [], []
        for a in range(3):
            pair = []
            for c in (mn[a], mx[a]):
                if math.isinf(inv[a]):
                    if c == o[a]:
                        self.nan = True  # 0 * inf: the NaN-faithful chain decides, not this model
                    t, e = (INF if (c > o[a]) == (inv[a] > 0) else -INF), 0.0
                else:
                    t = (c - o[a]) * inv[a]
                    mag = abs(c - o[a]) if grid is None else abs(c - grid[0][a]) + abs(grid[0][a] - o[a])
                    e = REL * mag * abs(inv[a])
                pair.append((t, e, (a, float(c))))
            pair.sort(key=lambda p: p[0])
            lo.append(pair[0])
            hi.append(pair[1])
        self.tmin, self.tmin_lo, self.tmin_hi, self.kmin = self._pick(lo, max)
        self.tmax, self.tmax_lo, self.tmax_hi, self.kmax = self._pick(hi, min)

    @staticmethod
    def _pick(vals, sel):
        t = sel(v[0] for v in vals)
        a = [v[0] for v in vals].index(t)
        lo, hi = sel(v[0] - v[1] for v in vals), sel(v[0] + v[1] for v in vals)
        if sel is max:
            alone = all(vals[a][0] - vals[a][1] > v[0] + v[1] for k, v in enumerate(vals) if k != a)
        else:
            alone = all(vals[a][0] + vals[a][1] < v[0] - v[1] for k, v in enumerate(vals) if k != a)
        return t, lo, hi, (vals[a][2] if alone else None)  # the operands that alone decide it, or None

    def hit(self, res):
        if self.nan:
            res.ok = False
        if self.tmin_hi - K_EPS <= self.tmax_lo:
            h = True
        elif self.tmin_lo - K_EPS > self.tmax_hi:
            h = False
        else:
            h = self.tmin - K_EPS <= self.tmax
            if not (self.kmin is not None and self.kmin == self.kmax):  # (a flat box: tmin and tmax are one value on the device)
                res.ok = False
        if self.tmax_lo >= -K_EPS:
            return h
        if self.tmax_hi >= -K_EPS:
            res.ok = False
        return h and self.tmax >= -K_EPS


def _beyond(lo, hi, t, bound, res):
    """t > bound, decided over the interval [lo, hi]; `bound` is a float32 the device computed with a rounding of its own."""
    e = REL * abs(bound)
    if lo > bound + e:
        return True
    if hi <= bound - e:
        return False
    res.ok = False
    return t > bound


def walk(sd, boxes, children, o, d, mode, dist=None, cap=None, root=0, grid=None, root_box=None):
    """One ray through a dumped tree.  mode: "closest", "occluder" or "window" (the two walks of a shadow query, dist the light's distance).
    cap: a stack of that many entries whose pushes onto a full stack are dropped, as the plain flavour would drop them.
    grid: (q_origin, q_cell) when `boxes` are dequantised ones.  root_box: (min, max) of the root, tested first as walk_start does."""
    assert len(sd.triangles) == len(children) + 1 and not (sd.objects["kind"] == 1).any(), "triangles only"
    o32, d32 = np.asarray(o, f32), np.asarray(d, f32)
    with np.errstate(divide="ignore"):
        inv = [float(x) for x in (f32(1.0) / d32)]  # make_ray: the float32 reciprocal
    o64, d64 = o32.astype(f64), d32.astype(f64)
    of = [float(x) for x in o64]
    res = WalkResult()
    lim, lo = INF, -INF
    if mode != "closest":
        margin = f32(f32(dist) * f32(1e-4) + f32(1e-2))
        lim, lo = float(f32(dist) + margin), float(f32(dist) - margin)
        dist = float(f32(dist))
    if root_box is not None and not _Box([float(x) for x in root_box[0]], [float(x) for x in root_box[1]], of, inv, None).hit(res):
        return res
    B = boxes.astype(f64)
    stack = []
    cur, cur_pos = int(root), -1

    def push(v):
        if cap is not None and len(stack) >= cap:
            res.dropped += 1
            return
        stack.append(v)
        res.held = max(res.held, len(stack))

    def pop():
        if not stack:
            return None, -1
        return stack.pop(), len(stack)

    while cur is not None:
        if cur >= 0:
            b = B[cur]
            sides = []
            for s in (0, 1):
                bx = _Box([float(x) for x in b[6 * s:6 * s + 3]], [float(x) for x in b[6 * s + 3:6 * s + 6]], of, inv, grid)
                h = bx.hit(res)
                if h and lim != INF:
                    h = not _beyond(bx.tmin_lo, bx.tmin_hi, bx.tmin, lim, res)
                if h and mode == "window":  # the child ends before the window: txl < lo
                    h = _beyond(bx.tmax_lo, bx.tmax_hi, bx.tmax, lo, res) or bx.tmax == lo
                sides.append((h, bx))
            (hl, bl), (hr, br) = sides
            left, right = int(children[cur][0]), int(children[cur][1])
            if hl and hr:
                if br.tmin_hi < bl.tmin_lo:
                    swap = True
                elif br.tmin_lo > bl.tmin_hi:
                    swap = False
                else:
                    swap = br.tmin < bl.tmin
                    if not (bl.kmin is not None and bl.kmin == br.kmin):  # (a tie of identical operands goes left on the device too)
                        res.ok = False
                push(left if swap else right)
                cur, cur_pos = (right if swap else left), -1
            elif hl:
                cur, cur_pos = left, -1
            elif hr:
                cur, cur_pos = right, -1
            else:
                cur, cur_pos = pop()
            continue
        prim = ~cur
        res.tests.append((prim, cur_pos))
        t = _triangle(sd, prim, o64, d64, res)
        if t is not None:
            if mode == "closest":
                if abs(t - res.t) <= T_ABS:
                    res.ok = False  # two hits this close: the tie rule or rounding decides
                if t < res.t:
                    res.t, res.prim, res.pos = t, prim, cur_pos
                    lim = float(f32(t + (abs(t) * 1e-4 + 1e-2)))
            else:
                dd = t - dist
                if abs(dd + K_EPS) <= T_ABS or abs(abs(dd) - K_EPS) <= K_EPS / 10:
                    res.ok = False
                if dd <= -K_EPS:
                    res.occluded, res.prim, res.t, res.pos = True, prim, t, cur_pos
                    return res
                if abs(dd) < K_EPS:
                    res.found = True
        cur, cur_pos = pop()
    return res


# --------------------------------------------------------------------------- cases
HOME_O, HOME_D = (-0.9, -0.9, -5.0), (0.0, 0.0, 1.0)  # the ray `keep` is chosen on


@dataclasses.dataclass
class Tree:
    """A tree as walk() takes it."""
    info: dict
    boxes: np.ndarray     # the boxes the flavour traverses (float, or dequantised)
    children: np.ndarray
    grid: tuple = None

    @property
    def height(self):
        return int(self.info["stack_entries"])

    def walk(self, sd, o, d, mode="closest", dist=None, cap=None):
        return walk(sd, self.boxes, self.children, o, d, mode, dist=dist, cap=cap, root=self.info["root"], grid=self.grid,
                    root_box=(self.info["root_min"], self.info["root_max"]))


def model_tree(sd, quantised=False, builder="lbvh"):
    info, boxes, children, _ = build_model(sd, builder)
    if not quantised:
        return Tree(info, boxes, children)
    qinfo, q = quantise_model(info, boxes)
    deq, grid = dequantised(qinfo, q)
    return Tree(qinfo, deq, children, grid)


def dumped_tree(dump):
    """From HipScene.dump_bvh(): the float boxes, or the dequantised ones when the scene traverses quantised nodes."""
    info, boxes, children, q = dump
    if q is None:
        return Tree(info, boxes, children)
    deq, grid = dequantised(info, q)
    return Tree(info, deq, children, grid)


def last_entry_case(pkg, n, tree):
    """-> keep: the one triangle to leave un-flipped so that the home ray's only hit is the leaf popped from position height - 2 of `tree`
    (the tree of chain_scene(pkg, n), which flipping leaves unchanged)."""
    r = tree.walk(flipped_chain(pkg, n), HOME_O, HOME_D)
    assert r.prim == -1 and r.ok, "the all-flipped chain is hit, or the home ray has no slack"
    assert r.held == tree.height - 1, "the home ray holds %d entries of height - 1 = %d" % (r.held, tree.height - 1)
    last = [p for p, pos in r.tests if pos == tree.height - 2]
    assert len(last) == 1, last
    return frozenset(last)


def tilt_of(n):
    """The slope of the tilted rays for the chain of n triangles, whose farthest one lies at z = 3 * 2^((n - 1) // 3 + 1)."""
    return min(1e-4, 0.04 / (3.0 * 2.0 ** ((n - 1) // 3 + 1)))


def ray_sets(n, large=2100):
    """The rays for the chain of n triangles: name -> (origins, dirs) float32.  16 origins on a grid around (-0.9, -0.9, -5); "axis": along
    +z (a zero direction component: the NaN-faithful slab chain, the generic loop); "tilt": all three components non-zero (the max3 /
    min3 chain and, with quantised nodes, the loop of k_trace_closest_refill), tilted by 1e-4 or, in long chains, by as much as keeps the
    ray within 0.04 of its origin's x and y where it meets the farthest triangle (whose footprint is the small one).  1 ray; 257 rays: a
    wave's chunk of 256, which its lanes refill three times, and one ray for the next wave; `large`: three workgroups of the refill kernel
    (1024 rays each), the last one partial.  "mixed": runs of 50 axis rays inside chunks of tilted ones, traced by the generic path
    before the refill loop starts."""
    xy = [(x, y) for x in (-0.93, -0.91, -0.89, -0.87) for y in (-0.93, -0.91, -0.89, -0.87)]
    O = np.array([(x, y, -5.0) for x, y in xy], f32)
    s = tilt_of(n)
    tilts = np.array([(s, s, 1), (-s, s / 2, 1), (s / 2, -s, 1), (-s / 2, -s / 2, 1)], f64)
    tilts = (tilts / np.linalg.norm(tilts, axis=1, keepdims=True)).astype(f32)
    assert (tilts != 0).all()
    out = {}
    for m in (1, 257, large):
        k = np.arange(m)
        out["axis-%d" % m] = (O[k % 16], np.tile(np.array(HOME_D, f32), (m, 1)))
        out["tilt-%d" % m] = (O[k % 16], tilts[(k // 16) % 4])
    k = np.arange(large)
    axis = (k % 300) < 50
    d = tilts[(k // 16) % 4].copy()
    d[axis] = HOME_D
    out["mixed-%d" % large] = (O[k % 16], d)
    return {name: (np.ascontiguousarray(o), np.ascontiguousarray(d)) for name, (o, d) in out.items()}


class Counter:
    """Model answers per distinct ray of one scene and tree, computed once."""

    def __init__(self, sd, tree, keep):
        self.sd, self.tree, self.keep, self.memo = sd, tree, keep, {}

    def one(self, o, d, mode, dist, cap=None):
        key = (np.asarray(o, f32).tobytes(), np.asarray(d, f32).tobytes(), mode, dist, cap)
        if key not in self.memo:
            self.memo[key] = self.tree.walk(self.sd, o, d, mode, dist, cap)
        return self.memo[key]

    def counts(self, r):
        """The three conditions: height - 1 entries, the answer from the last one, slack everywhere."""
        h = self.tree.height
        return r.ok and r.held == h - 1 and r.pos == h - 2 and r.prim in self.keep

    def counting(self, o, d, mode="closest", dist=None):
        """-> (mask of the rays that count, the model's results)"""
        rs = [self.one(o[i], d[i], mode, dist) for i in range(len(o))]
        return np.array([self.counts(r) for r in rs]), rs


# --------------------------------------------------------------------------- the entry points (GPU tests)
def narrow_camera(pkg, n, size=8):
    """A camera at the home ray's origin looking along +z, its field of view as narrow as the tilt of ray_sets(n): its rays are tilted ones."""
    return pkg.scenes.make_camera(size, size, math.degrees(tilt_of(n)), HOME_O, (HOME_O[0], HOME_O[1], 0.0))


def path_ids(n):
    """(pixel, sample, channel) of n paths for cast_rays: every ray its own random stream, the three channels in turn."""
    k = np.arange(n)
    return (k % 4096).astype(np.uint32), (k // 4096).astype(np.uint32), (k % 3).astype(np.int32)


def entry_points(hs, o, d, n_sensors=200):
    """Every entry point that walks the tree, on one ray set -> dict of numpy arrays.  tmax and dist are FAR, beyond every box, so that
    the occluder walk enters every box the ray meets; `shadow_found` passes found = 1 (the occluder walk alone, as k_direct's found light
    samples run it), `shadow` passes no hint: its window walk comes first, enters nothing and holds no entry (the model's figure,
    tests/test_stack_model_cpu.py), so nothing is found and the occluder walk never starts."""
    from ray_query_cases import Rays, closest, occluded
    from sensor_query_cases import cast_values, fold, radiance
    n = len(o)
    out = {}
    out["t"], out["prim"] = hs.intersect(o, d)
    res, _ = closest(hs, Rays(o, d))
    out["query_t"], out["query_prim"] = res["t"], res["prim"]
    far = np.full(n, FAR, f32)
    out["occluded"], _ = occluded(hs, Rays(o, d, far))
    out["shadow_found"] = hs.shadow_visible(o, d, far, found=np.ones(n, np.uint8))
    out["shadow"] = hs.shadow_visible(o, d, far)
    out["cast"] = hs.cast_rays(o, d, *path_ids(n), seed=9)
    m = min(n, n_sensors)
    out["sensor"], _, _ = radiance(hs, o[:m], d[:m], spp=2, seed=4)
    out["sensor_want"] = fold(cast_values(hs, o[:m], d[:m], 2, seed=4))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """Equal bits (NaN equals NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    return a == b


class Expect:
    """What the entry points must return for one description and the tree the device built for it: the model's verdict on every ray
    (which ones count) and the oracle's answers, computed once per ray set."""

    def __init__(self, oracle, sd, tree, keep, n):
        self.sd, self.tree, self.keep, self.n = sd, tree, keep, n
        self.model = Counter(sd, tree, keep)
        self.osc = oracle.OracleScene(sd)
        self.sets = ray_sets(n)
        self.memo = {}

    def close(self):
        self.osc.close()

    def want(self, name):
        """(counting mask for the closest walk, for the occluder walk, oracle t, oracle prim, oracle cast_rays)"""
        if name not in self.memo:
            o, d = self.sets[name]
            closest, _ = self.model.counting(o, d)
            occluder, _ = self.model.counting(o, d, "occluder", FAR)
            t, prim = self.osc.intersect(o, d)
            self.memo[name] = (closest, occluder, t, prim, self.osc.cast_rays(o, d, *path_ids(len(o)), seed=9))
        return self.memo[name]

    def check(self, name, got):
        """`got`, the entry_points of a handle on set `name`, against the oracle on the rays that count; nothing is asserted on the others."""
        from ray_query_cases import expected_occluded
        o, d = self.sets[name]
        n = len(o)
        closest, occluder, t, prim, cast = self.want(name)
        print("\nn %d, height %d, %s: %d rays, %d count for the closest walk, %d for the occluder walk; keep %s"
              % (self.n, self.tree.height, name, n, closest.sum(), occluder.sum(), sorted(self.keep)))
        assert closest.mean() >= 0.5 and occluder.mean() >= 0.5
        assert np.isin(prim[closest], sorted(self.keep)).all(), "the oracle and the model disagree"
        # intersect (k_trace_closest / k_trace_closest_refill) and query_closest (the same kernels on the staged chunk)
        for tk, pk in (("t", "prim"), ("query_t", "query_prim")):
            bad = closest & ((got[pk] != prim) | (bits(got[tk]) != bits(t)))
            first = int(np.argmax(bad))
            assert not bad.any(), "%s: %d of %d counting rays differ from the oracle, e.g. ray %d: primitive %d (oracle %d)" % (
                pk, bad.sum(), closest.sum(), first, got[pk][first], prim[first])
        # query_occluded (k_query_occluded) and the render loop's shadow query with the light sample found (k_trace_shadow): the occluder walk
        want_occ = expected_occluded(t, prim, np.full(n, FAR, f32))
        assert (want_occ[occluder] == 1).all()
        bad = occluder & (got["occluded"] != want_occ)
        assert not bad.any(), "query_occluded: %d of %d counting rays are reported visible" % (bad.sum(), occluder.sum())
        bad = occluder & (got["shadow_found"] != (want_occ == 0))
        assert not bad.any(), "shadow_visible(found=1): %d of %d counting rays are reported visible" % (bad.sum(), occluder.sum())
        assert not got["shadow"][occluder].any()  # no hint: the window walk finds nothing at FAR, whatever the stack holds
        # cast_rays: the wavefront loop (first rays through launch_trace_closest), every path value the oracle's
        bad = closest & ~same(got["cast"], cast)
        assert not bad.any(), "cast_rays: %d of %d counting paths differ from the oracle" % (bad.sum(), closest.sum())
        # ray sensors (k_sensor_primary): the float32 fold of cast_rays, as tests/test_gpu_sensor_query.py compares them
        m = len(got["sensor"])
        bad = closest[:m, None] & ~same(got["sensor"], got["sensor_want"])
        assert not bad.any(), "query_radiance: %d sensor values differ from the fold of cast_rays" % bad.sum()
        sky = (got["sensor"] == np.array(self.sd.background, f32)).all(axis=1)
        assert not (closest[:m] & sky).any(), "a counting sensor sees the sky"


# --------------------------------------------------------------------------- live scenes
def split_chain(sd):
    """The same triangles as two objects: all but the last one, and the last one on its own (no box, code or primitive id changes)."""
    n = len(sd.triangles)
    obj = np.zeros(2, sd.objects.dtype)
    obj[0] = obj[1] = sd.objects[0]
    obj["n_tri"][0], obj["first_tri"][1], obj["n_tri"][1] = n - 1, n - 1, 1
    return dataclasses.replace(sd, objects=obj)


def first_part(sd):
    """Object 0 of a split chain alone, and (objects, triangles) as add_objects takes them to bring the last triangle back."""
    n = len(sd.triangles)
    objs = sd.objects[1:2].copy()
    objs["first_tri"][0] = 0
    return dataclasses.replace(sd, objects=sd.objects[:1].copy(), triangles=sd.triangles[:n - 1].copy()), (objs, sd.triangles[n - 1:].copy())


def pulled_in(sd, k):
    """-> (factor, positions[1,3,3]): triangle k of a flipped chain with its far edge pulled in along its long axis, by the first factor for
    which the builder model gives a tree one level lower (its centroid then shares the leading Morton bit of an earlier triangle)."""
    a = k % 3
    assert a < 2, "the triangles far away in z have no long axis"
    L = f32(3.0 * 2.0 ** (k // 3 + 1))
    h = build_model(sd, "lbvh")[0]["stack_entries"]
    for factor in (0.5, 0.25, 0.75):
        tri = sd.triangles.copy()
        P = np.stack([tri["v0"][k], tri["v1"][k], tri["v2"][k]]).astype(f32)
        assert (P[:, a] == L).sum() == 2  # (flipped: the far edge)
        P[P[:, a] == L, a] = f32(L * f32(factor))
        tri["v0"][k], tri["v1"][k], tri["v2"][k] = P
        if build_model(dataclasses.replace(sd, triangles=tri), "lbvh")[0]["stack_entries"] == h - 1:
            return factor, P[None]
    raise AssertionError("no factor lowers the tree")
