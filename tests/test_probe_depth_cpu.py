"""The probe-visibility rule without a GPU (include/mcpt.h: mcpt_probe_depth_dirs_host, mcpt_probe_depth_texel_host,
mcpt_probe_depth_fold_host, mcpt_probe_shade_visible_host): csrc/mcpt_probe_depth.h compiled for the CPU against the numpy float32
restatements of tests/probe_depth_cases.py, bit for bit, and against what the text says at its edges."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_cases as pc  # noqa: E402
import probe_depth_cases as pdc  # noqa: E402
from test_probes_cpu import GRIDS, lookup_points, unit  # noqa: E402

f32, f64 = np.float32, np.float64
U = 2.0 ** -24  # the unit roundoff of float32


def assert_bits(got, want, what=""):
    bad = ~pc.same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


# ---------------------------------------------------------------- texels
def test_texel_round_trip(hip):
    """texel(c_j) == j, and |c_j| = 1 within 3.5 u: the squared norm is three products (u each) and two additions of positive terms
    (u each), at most 3 u relative; the square root halves that and rounds once (2.5 u); each component's division rounds once more."""
    c = hip.probe_depth_dirs()
    assert c.shape == (64, 3) and c.dtype == f32
    assert_bits(c, pdc.texel_dirs(), "host against the restatement")
    assert np.array_equal(hip.probe_depth_texel(c), np.arange(64))
    assert np.array_equal(pdc.texel_of(c), np.arange(64))
    err = np.abs(np.linalg.norm(c.astype(f64), axis=1) - 1)
    print("\n[probe depth] max ||c_j| - 1| = %.3g (bound %.3g)" % (err.max(), 4 * U))
    assert err.max() <= 4 * U
    # scaled copies keep their texel: the vector need not be unit
    assert np.array_equal(hip.probe_depth_texel(c * f32(1000)), np.arange(64))
    assert np.array_equal(hip.probe_depth_texel(c * f32(1e-3)), np.arange(64))
    # both hemispheres are covered: |ox| + |oy| > 1 folds to z < 0
    assert (c[:, 2] < 0).sum() == 24 and (c[:, 2] == 0).sum() == 16 and (c[:, 2] > 0).sum() == 24


def test_direction_edge_cases(hip):
    """What the text gives by hand: px = 1 lands on the clamp (floor(8) -> 7); the fold of -z is (sgn(0), sgn(0)) = (1, 1); vz = 0 and
    vz = -0 are not folded, and a vector just below the seam folds onto the same texel; zero and non-finite vectors have texel 0."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                  [0.3, 0.7, 0.0], [0.3, 0.7, -0.0], [0.3, 0.7, -1e-30], [-0.3, 0.7, 0.0], [30, 70, 0],
                  [0, 0, 0], [np.nan, 1, 0], [np.inf, 1, 0], [3e38, 3e38, 3e38], [0.1, 0.1, 0.8], [0.1, 0.1, -0.8]], f32)
    want = np.array([39, 32, 60, 4, 36, 63, 53, 53, 53, 50, 53, 0, 0, 0, 0, 36, 63], np.int32)
    assert np.array_equal(hip.probe_depth_texel(v), want)
    assert np.array_equal(pdc.texel_of(v), want)
    rng = np.random.default_rng(5)
    r = np.concatenate([unit(rng, 2000), (rng.normal(size=(500, 3)) * 100).astype(f32)])
    r[::7, 2] = 0
    r[::11, 0] = 0
    got = hip.probe_depth_texel(r)
    assert np.array_equal(got, pdc.texel_of(r)) and got.min() >= 0 and got.max() <= 63
    # the nearest texel: no other texel direction is closer than the chosen one by more than the map's distortion allows -- the chosen
    # direction is within the largest angle between neighbouring texel centres (a loose sanity check of the orientation, not of bits)
    c = hip.probe_depth_dirs().astype(f64)
    u = r[:2000].astype(f64)
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    assert (np.einsum("ij,ij->i", c[got[:2000]], u) > 0.8).all()


# ---------------------------------------------------------------- fold
def synthetic(rng, n, spp, max_distance=4.0):
    d = unit(rng, n * spp).reshape(n, spp, 3)
    r = np.minimum(rng.uniform(0.05, 6.0, (n, spp)), max_distance).astype(f32)
    bf = rng.uniform(size=(n, spp)) < 0.3
    return d, r, bf


@pytest.mark.parametrize("spp", [1, 5, 64, 70, 130])
def test_fold_against_the_restatement(hip, spp):
    rng = np.random.default_rng(100 + spp)
    n = 3
    d, r, bf = synthetic(rng, n, spp)
    m, c = hip.probe_depth_fold(d, r, bf)
    wm, wc = pdc.fold(d, r, bf)
    assert m.shape == (n, 192) and m.dtype == f32 and c.shape == (n, 2) and c.dtype == np.int32
    assert_bits(m, wm, "spp %d" % spp)
    assert np.array_equal(c, wc) and (c[:, 0] == spp).all() and np.array_equal(c[:, 1], bf.sum(1))
    assert (m.reshape(n, 64, 3)[:, :, 0] >= 0).all()
    # accumulate: onto arbitrary earlier sums and counts
    m0 = rng.uniform(0, 3, (n, 192)).astype(f32)
    c0 = rng.integers(0, 1000, (n, 2)).astype(np.int32)
    m1, c1 = hip.probe_depth_fold(d, r, bf, m0, c0)
    wm1, wc1 = pdc.fold(d, r, bf, m0, c0)
    assert_bits(m1, wm1, "spp %d, accumulate" % spp)
    assert np.array_equal(c1, wc1) and np.array_equal(c1[:, 0], c0[:, 0] + spp)
    # a split call equals one call
    for a in sorted({1, spp // 2, 64} & set(range(1, spp))):
        ma, ca = hip.probe_depth_fold(d[:, :a], r[:, :a], bf[:, :a])
        mb, cb = hip.probe_depth_fold(d[:, a:], r[:, a:], bf[:, a:], ma, ca)
        assert_bits(mb, m, "spp %d = %d + %d" % (spp, a, spp - a))
        assert np.array_equal(cb, c)


def test_fold_weight_is_cos32(hip):
    """One sample along a texel's own direction: W = fl(dot)^32 by five squarings, S1 = W r, S2 = W (r r); a sample in the opposite
    hemisphere of a texel adds exactly zero to it."""
    c = hip.probe_depth_dirs()
    d = c[36][None, None, :]
    m, _ = hip.probe_depth_fold(d, [[2.5]], [[0]])
    m = m.reshape(64, 3)
    w = pdc.dot3(c[36], c[36])
    for _ in range(5):
        w = w * w
    assert m[36, 0] == w and m[36, 1] == w * f32(2.5) and m[36, 2] == w * (f32(2.5) * f32(2.5))
    away = pdc.dot3(c, c[36][None, :]) <= 0
    assert away.sum() >= 10 and not m[away].any()
    # |c|^2 is within 10 u of 1 (3.5 u per factor, 3 u for the sum); 32nd power and 31 roundings of the squarings: below 400 u
    assert abs(float(m[36, 0]) - 1) <= 400 * U


# ---------------------------------------------------------------- lookup
def volume(rng, origin, spacing, dims, spp=96):
    """Coefficients, depth moments of synthetic samples at the scale of the grid, and counts; one probe in four has a W == 0 texel row
    (all of its texels) or single zeroed texels."""
    m = dims[0] * dims[1] * dims[2]
    sh = rng.normal(size=(m, 27)).astype(f32)
    scale = float(np.mean(spacing))
    d = unit(rng, m * spp).reshape(m, spp, 3)
    r = (rng.uniform(0.2, 2.5, (m, spp)) * scale).astype(f32)
    bf = rng.uniform(size=(m, spp)) < 0.15
    mom, cnt = pdc.fold(d, r, bf)
    mom = mom.reshape(m, 64, 3)
    mom[::4, ::3, :] = 0  # W == 0 texels
    return sh, mom.reshape(m, 192), cnt


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_lookup_against_the_restatement(hip, name):
    origin, spacing, dims = GRIDS[name]
    rng = np.random.default_rng(7)
    m = dims[0] * dims[1] * dims[2]
    sh, mom, cnt = volume(rng, origin, spacing, dims)
    p = lookup_points(rng, origin, spacing, dims, 100)
    n = unit(rng, len(p))
    for nb, bm in ((0.0, 0.25), (0.2, 0.25), (0.05, 0.0), (0.0, 1.0)):
        got, wt = hip.probe_shade_visible(origin, spacing, dims, sh, mom, cnt, p, n, normal_bias=nb, backface_max=bm, weight=True)
        want, wa = pdc.shade_visible(origin, spacing, dims, sh, mom, cnt, p, n, nb, bm)
        assert_bits(got, want, "%s, bias %g, backface_max %g" % (name, nb, bm))
        assert_bits(wt, wa, "%s, weights" % name)
    plain = hip.probe_shade(origin, spacing, dims, sh, p, n)
    assert (got != plain).any() or m == 1
    # dead probes: every second probe buried
    dead = cnt.copy()
    dead[::2] = (24, 24)
    killed = np.nonzero((dead[:, 0] > 0) & (dead[:, 1].astype(f32) > f32(0.25) * dead[:, 0].astype(f32)))[0]
    got, wt = hip.probe_shade_visible(origin, spacing, dims, sh, mom, dead, p, n, weight=True)
    want, wa = pdc.shade_visible(origin, spacing, dims, sh, mom, dead, p, n, 0.0, 0.25)
    assert_bits(got, want, name + ", dead probes")
    assert_bits(wt, wa, name + ", dead probes, weights")
    assert_bits(got, pdc.shade_visible(origin, spacing, dims, sh, mom, cnt * 0, p, n, 0.0, 0.25, kill=killed)[0], name + ", dead = weight 0")
    # every probe dead: the plain lookup, equal bits
    dead[:] = (10, 9)
    got, wt = hip.probe_shade_visible(origin, spacing, dims, sh, mom, dead, p, n, weight=True)
    assert not wt.any()
    assert_bits(got, plain, name + ", all dead")
    # a probe without samples is alive whatever backface_max; exactly at the threshold it is alive too (strictly greater kills)
    edge = cnt.copy()
    edge[:] = (8, 2)
    a = hip.probe_shade_visible(origin, spacing, dims, sh, mom, edge, p, n, backface_max=0.25)
    b = hip.probe_shade_visible(origin, spacing, dims, sh, mom, cnt * 0, p, n, backface_max=0.0)
    assert_bits(a, b, name + ", threshold")
    # no depth information at all (W == 0 everywhere): trilinear x backface weights only, ch = 1
    got0, wt0 = hip.probe_shade_visible(origin, spacing, dims, sh, mom * 0, cnt, p, n, weight=True)
    want0, wa0 = pdc.shade_visible(origin, spacing, dims, sh, mom * 0, cnt, p, n, 0.0, 0.25)
    assert_bits(got0, want0, name + ", W == 0")
    assert (wt0 > 0).all()


def test_identical_probes_give_their_own_irradiance(hip):
    """With the same coefficients L at every probe the weights cancel: out = sh_irradiance(L, n) up to rounding.  Against the float
    sh_irradiance(L, n), with M = sum_j |A(j) L_j Y_j(n)| (the terms may cancel, so M and not the result is the scale) and S the exact sum
    of the weights: a blended coefficient is one product and seven additions of terms of one sign, b_j = S L_j (1 + 8 u); its irradiance
    sum makes two products and eight additions per term, 10 u M S, so 18 u M S in all; A = S (1 + 7 u) from its seven additions and the
    quotient rounds once: 26 u M.  The reference's own sum is another 10 u M: 36 u M to first order, asserted as 40 u M.  Points whose
    A is below 1e-3 are left out, so that no product a * L gets near the subnormals."""
    origin, spacing, dims = GRIDS["3x2x4"]
    rng = np.random.default_rng(9)
    m = 24
    _, mom, cnt = volume(rng, origin, spacing, dims, spp=256)
    cnt[5] = (24, 20)  # one dead probe among them
    L = rng.normal(size=27).astype(f32)
    sh = np.ascontiguousarray(np.broadcast_to(L, (m, 27)))
    p = lookup_points(rng, origin, spacing, dims, 200)
    n = unit(rng, len(p))
    got, wt = hip.probe_shade_visible(origin, spacing, dims, sh, mom, cnt, p, n, normal_bias=0.1, weight=True)
    want = hip.sh_irradiance(L, n).astype(f64)
    Y = hip.sh_basis(n).astype(f64)
    M = (np.abs(pc.BAND.astype(f64)[None, :, None] * L.astype(f64).reshape(1, 9, 3)) * np.abs(Y)[:, :, None]).sum(axis=1)
    keep = wt > 1e-3
    assert keep.sum() >= 100 and np.unique(wt[keep]).size >= 100  # the weights do differ from point to point
    err = (np.abs(got.astype(f64) - want) / M)[keep]
    print("\n[probe depth] identical probes: largest error %.3g M (bound %.3g)" % (err.max(), 40 * U))
    assert err.max() <= 40 * U
