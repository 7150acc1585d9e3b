"""Pixel-centre feature rays on the GPU (include/mcpt.h: mcpt_feature_opts, mcpt_centre_rays, mcpt_render_aovs_features,
mcpt_render_motion_features, mcpt_sequence_create_features): k_centre_rays gives the bits of the numpy restatement; the switch off is the
_ex call and mcpt_sequence_create_moments; centre records do not depend on the seed; centre AOVs follow their definition on the oracle's
hits and centre motion the float64 restatement of tests/test_gpu_temporal.py; a static one-sample sequence under depth of field keeps its
whole history on every covered pixel, which sampled features do not; a centre sequence is the composition of the separate _features
calls, plain, through mirror chains and adaptive, with the host builder and with PLOC; refusals leave the history alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirror_scene as ms  # noqa: E402
from centre_cases import cameras, centre_rays_f32, small_camera  # noqa: E402
from conftest import TREES  # noqa: E402
from test_gpu_adaptive import _mid_threshold  # noqa: E402
from test_gpu_sequence import ALL, SHORT, translate  # noqa: E402
from test_gpu_temporal import GLASS_SPHERE, MOVE, assert_motion_close, prims_of, scene_geometry  # noqa: E402
from test_temporal_cpu import bits_equal, project_f64  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
CAMERAS = ["cornell", "cornell_dof", "chess_dof"]


@pytest.fixture(scope="module")
def tiny(pkg, hip):
    hs = hip.HipScene(pkg.scenes.cornell_demo(8, 8, 4))
    yield hs
    hs.close()


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("name", CAMERAS)
def test_centre_rays_equal_the_restatement(pkg, hip, tiny, name):
    _, cam = cameras(pkg)[name]
    n = int(cam["width"]) * int(cam["height"])
    o, d = tiny.centre_rays(np.arange(n), camera=cam)
    wo, wd = centre_rays_f32(cam)
    assert bits_equal(o, wo), int((o.view(np.uint32) != wo.view(np.uint32)).sum())
    assert bits_equal(d, wd), int((d.view(np.uint32) != wd.view(np.uint32)).sum())
    # pixels in any order, with repeats and runs (one launch per run of consecutive pixels)
    pick = np.array([n - 1, 0, 1, 2, 700, 5, 6, 5, n // 2, n // 2 + 1], np.uint32)
    o2, d2 = tiny.centre_rays(pick, camera=cam)
    assert bits_equal(o2, wo[pick]) and bits_equal(d2, wd[pick])


@pytest.mark.parametrize("shape", [(1, 1), (3, 5)])
@pytest.mark.parametrize("dof", [False, True])
def test_centre_rays_of_small_frames(pkg, hip, tiny, shape, dof):
    H, W = shape
    cam = small_camera(pkg, W, H, dof)
    o, d = tiny.centre_rays(np.arange(W * H), camera=cam)
    wo, wd = centre_rays_f32(cam)
    assert bits_equal(o, wo) and bits_equal(d, wd)
    assert np.array_equal(o, np.broadcast_to(np.asarray(cam["position"], f32), o.shape))  # the centre of the lens is the eye


# ---------------------------------------------------------------- 2. the switch off changes nothing
@pytest.mark.parametrize("depth", [0, 2])
def test_null_or_zeroed_options_are_the_ex_calls(pkg, hip, depth):
    sd = ms.mirror_scene(pkg)
    hs = hip.HipScene(sd)
    hs.snapshot()
    hs.update([(ms.BOX, ms.translate(2.5, 0, 0))])
    aov = hs.render_aovs(aov_spp=4, seed=5, specular_depth=depth)
    motion = hs.render_motion(seed=5, aov_spp=4, specular_depth=depth)
    assert (motion[..., 0:2] != 0).any()
    for f in ("null", hip.FeatureOpts()):
        assert bits_equal(hs.render_aovs(aov_spp=4, seed=5, specular_depth=depth, features=f), aov)
        assert bits_equal(hs.render_motion(seed=5, aov_spp=4, specular_depth=depth, features=f), motion)
        assert bits_equal(hs.render_aovs(seed=5, specular_depth=depth, features=f), aov)  # aov_spp 0 still means 4
    hs.close()


def test_null_or_zeroed_options_are_sequence_create_moments(pkg, hip):
    sd = pkg.scenes.cornell_demo(48, 32, 4)
    scenes = [hip.HipScene(sd) for _ in range(3)]
    kw = dict(filter=True, normal_test=True, color_clamp=True, moments=True)
    seqs = [hip.HipSequence(scenes[0], **kw), hip.HipSequence(scenes[1], features="null", **kw), hip.HipSequence(scenes[2], features=hip.FeatureOpts(), **kw)]
    for k in range(4):
        rs = []
        for hs, s in zip(scenes, seqs):
            hs.update([(SHORT, translate(-32.0 * k, 0, 0))])
            rs.append(s.frame(want=ALL, spp=1, seed=k + 1))
        for r in rs[1:]:
            for key in ALL:
                assert np.array_equal(r[key].view(np.uint8), rs[0][key].view(np.uint8)), (k, key)
        for s in seqs[1:]:
            assert np.array_equal(s.flags(), seqs[0].flags()) and bits_equal(s.moments(), seqs[0].moments())
    assert rs[0]["len"].max() == 4 and (rs[0]["motion"][..., 0:2] != 0).any()
    for x in seqs + scenes:
        x.close()


# ---------------------------------------------------------------- 3. seed independence
@pytest.mark.parametrize("depth", [0, 2])
def test_centre_records_do_not_depend_on_the_seed(pkg, hip, depth):
    sd = ms.mirror_scene(pkg)
    hs = hip.HipScene(sd)
    hs.snapshot()
    hs.update([(ms.BOX, ms.translate(2.5, 0, 0))])
    a1, a77 = (hs.render_aovs(seed=s, specular_depth=depth, centre=True) for s in (1, 77))
    m1, m77 = (hs.render_motion(seed=s, specular_depth=depth, centre=True) for s in (1, 77))
    assert bits_equal(a1, a77) and bits_equal(m1, m77)
    assert bits_equal(hs.render_aovs(seed=1, aov_spp=1, specular_depth=depth, centre=True), a1)  # aov_spp 0 means 1
    assert set(np.unique(a1[..., 7])) == {0.0, 1.0} and set(np.unique(m1[..., 3])) <= {0.0, 1.0}
    assert (m1[..., 0:2] != 0).any()
    # the sampled features do depend on it (the control)
    assert not bits_equal(hs.render_aovs(seed=1, aov_spp=1, specular_depth=depth), hs.render_aovs(seed=77, aov_spp=1, specular_depth=depth))
    hs.close()


# ---------------------------------------------------------------- 4. centre AOVs against the oracle
def _tri_normals(sd):
    t = sd.triangles
    v0, v1, v2 = (t[k].astype(np.float64) for k in ("v0", "v1", "v2"))
    n = np.cross(v1 - v0, v2 - v0)
    with np.errstate(invalid="ignore"):  # (degenerate triangles: never hit)
        return n / np.linalg.norm(n, axis=1, keepdims=True)


_oracle_ref = {}


def oracle_aovs(pkg, oracle, hs, name):
    """The float64 restatement of test_gpu_denoise.test_aovs_against_the_oracle at one sample per pixel, on the oracle's hits of the device's
    centre rays: (ref[n, 8] float32 without the normal, normal[n, 3] float64, textured[n], prim[n]); computed once per scene."""
    if name in _oracle_ref:
        return _oracle_ref[name]
    sd, cam = cameras(pkg)[name]
    n_px = int(cam["width"]) * int(cam["height"])
    o, d = hs.centre_rays(np.arange(n_px), camera=cam)
    t, prim = oracle.OracleScene(sd).intersect(o, d)
    n_tri = len(sd.triangles)
    obj = sd.objects
    tri_mat = np.zeros(n_tri, np.int32)
    for ob in obj:
        if ob["kind"] == 0:
            tri_mat[ob["first_tri"]:ob["first_tri"] + ob["n_tri"]] = ob["material"]
    mats = sd.materials
    nrm_tri = _tri_normals(sd)
    hit = prim >= 0
    mat = np.where(hit, np.where(prim < n_tri, tri_mat[np.clip(prim, 0, n_tri - 1)], obj["material"][np.clip(prim - n_tri, 0, len(obj) - 1)]), -1)
    nrm = np.zeros((n_px, 3))
    tri = hit & (prim < n_tri)
    nrm[tri] = nrm_tri[prim[tri]]
    sph = hit & (prim >= n_tri)
    if sph.any():
        ob = obj[prim[sph] - n_tri]
        p = o[sph] + d[sph] * t[sph].astype(f32)[:, None]
        dv = p.astype(np.float64) - ob["center"]
        nrm[sph] = dv / np.linalg.norm(dv, axis=1, keepdims=True)
    flip = (nrm * d).sum(1) > 0
    nrm[flip] = -nrm[flip]
    alb = np.ones((n_px, 3), f32)
    textured = np.zeros(n_px, bool)
    for i in np.nonzero(hit)[0]:
        m = mats[mat[i]]
        if np.any(m["emission"] > 0) or m["type"] >= 2:
            continue
        if m["textured"] and prim[i] < n_tri:
            textured[i] = True
            tr = sd.triangles[prim[i]]
            P = o[i].astype(np.float64) + d[i].astype(np.float64) * t[i]
            A, B, Cc = (tr[k].astype(np.float64) for k in ("v0", "v1", "v2"))
            M = np.stack([B - A, Cc - A], 1)
            u, v = np.linalg.lstsq(M, P - A, rcond=None)[0]
            uv = (1 - u - v) * tr["t0"] + u * tr["t1"] + v * tr["t2"]
            col, row = int((f32(uv[0]) - f32(0.05)) * 10), int(f32(uv[1]) * 12)
            alb[i] = 0.9 if (3 <= col <= 5 and row <= 7 and (col + row) % 2 == 1) else 0.1
        else:
            alb[i] = m["base_reflectance"]
    ref = np.zeros((n_px, 8), f32)
    ref[:, 0:3] = alb  # (the fold of one record: 0 + x / 1)
    ref[:, 6] = np.where(hit, t, 0.0).astype(f32)  # (a miss carries DBL_MAX)
    ref[:, 7] = hit.astype(f32)
    _oracle_ref[name] = (ref, nrm, textured, prim)
    return _oracle_ref[name]


@pytest.mark.parametrize("name,tree", [("cornell_dof", t) for t in TREES] + [("chess_dof", None)],
                         ids=["cornell-%s-%s" % t for t in TREES] + ["chess-default"])
def test_centre_aovs_against_the_oracle(pkg, hip, oracle, tree_env, name, tree):
    if tree is not None:
        tree_env(*tree)
    sd, cam = cameras(pkg)[name]
    hs = hip.HipScene(sd)
    ref, nrm, textured, prim = oracle_aovs(pkg, oracle, hs, name)
    got = hs.render_aovs(seed=9, camera=cam, centre=True).reshape(-1, 8)
    assert np.array_equal(got[:, 7], (prim >= 0).astype(f32))  # coverage is exactly prim >= 0
    assert np.array_equal(got[:, 7], ref[:, 7])
    assert np.array_equal(got[:, 6], ref[:, 6])
    np.testing.assert_allclose(got[:, 3:6], nrm, rtol=0, atol=1e-6)
    bad = (got[:, 0:3] != ref[:, 0:3]).any(1)
    assert not (bad & ~textured).any(), "albedo differs off the textured floor"
    assert bad.sum() <= 0.005 * textured.sum(), (int(bad.sum()), int(textured.sum()))
    for m_ in np.nonzero(bad)[0]:
        assert all(float(x) in (float(f32(0.1)), float(f32(0.9))) for x in got[m_, 0:3]), (m_, got[m_, 0:3], ref[m_, 0:3])
    assert (got[:, 7] == 0).any() and (got[:, 7] == 1).any()
    if name == "chess_dof":
        assert textured.sum() > 100
    hs.close()


# ---------------------------------------------------------------- 5. centre motion
def centre_motion_f64(pkg, hip, hs, sd, cam, prev_cam, cur_xf, prev_xf):
    """test_gpu_temporal.motion_f64 on the centre rays, one per pixel: the motion records of include/mcpt.h in float64 from mcpt_centre_rays +
    mcpt_intersect on the live scene (whose transforms are cur_xf; the snapshot was taken under prev_xf).  (motion[H, W, 4], prim[H, W])."""
    W, H = int(cam["width"]), int(cam["height"])
    n_px = W * H
    o, d = hs.centre_rays(np.arange(n_px), camera=cam)
    t, prim = hs.intersect(o, d)
    hit = prim >= 0
    n_tri = len(sd.triangles)
    p_cur = o.astype(np.float64) + d.astype(np.float64) * np.where(hit, t, 0.0)[:, None]
    p_prev = p_cur.copy()
    Vc, Cc = scene_geometry(pkg, hip, sd, cur_xf)
    Vp, Cp = scene_geometry(pkg, hip, sd, prev_xf)
    tr = hit & (prim < n_tri)
    k = prim[tr]
    v0, e1, e2 = Vc[k, 0], Vc[k, 1] - Vc[k, 0], Vc[k, 2] - Vc[k, 0]
    r = p_cur[tr] - v0
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    d1, d2 = (r * e1).sum(1), (r * e2).sum(1)
    det = a * c - b * b
    u, v = (c * d1 - b * d2) / det, (a * d2 - b * d1) / det
    p_prev[tr] = Vp[k, 0] + (Vp[k, 1] - Vp[k, 0]) * u[:, None] + (Vp[k, 2] - Vp[k, 0]) * v[:, None]
    sp = hit & (prim >= n_tri)
    p_prev[sp] = p_cur[sp] + (Cp[prim[sp] - n_tri] - Cc[prim[sp] - n_tri])
    xy_c, z_c = project_f64(cam, p_cur)
    xy_p, z_p = project_f64(prev_cam, p_prev)
    valid = hit & (z_c > 0) & (z_p > 0)
    rec = np.zeros((n_px, 4))
    rec[valid, 0:2] = (xy_p - xy_c)[valid]
    rec[valid, 2] = np.linalg.norm(p_prev - np.asarray(prev_cam["position"], np.float64).reshape(3), axis=1)[valid]
    rec[valid, 3] = 1
    return rec.reshape(H, W, 4), prim.reshape(H, W)


def test_static_scene_under_depth_of_field_has_zero_centre_motion(pkg, hip):
    sd, cam = cameras(pkg)["cornell_dof"]
    hs = hip.HipScene(sd)
    aov = hs.render_aovs(camera=cam, centre=True)
    assert (aov[..., 7] == 1).any() and (aov[..., 7] == 0).any()
    for snap in (False, True):
        if snap:
            hs.snapshot()
        m = hs.render_motion(camera=cam, seed=3, centre=True)
        assert (m[..., 0] == 0).all() and (m[..., 1] == 0).all(), snap
        assert bits_equal(m[..., 3], aov[..., 7]), snap
    hs.close()


@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("obj", [SHORT, GLASS_SPHERE], ids=["short_box", "glass_sphere"])
def test_one_moved_object_centre(pkg, hip, obj, builder):
    sd, cam = cameras(pkg)["cornell_dof"]
    hs = hip.HipScene(sd, builder=builder)
    hs.snapshot()
    info = hs.update([(obj, MOVE)])
    assert info["path"] == (1 if builder == "ploc" else 0)
    got = hs.render_motion(camera=cam, seed=1, centre=True)
    want, prim = centre_motion_f64(pkg, hip, hs, sd, cam, cam, {obj: MOVE}, {})
    assert_motion_close(got, want, "centre, object %d, %s" % (obj, builder))
    on_moved = np.isin(prim, prims_of(sd, [obj]))
    assert on_moved.sum() > 50
    assert (got[..., 0:2][~on_moved] == 0).all()  # an unmoved primitive (or nothing) seen: exactly zero
    assert (got[..., 0][on_moved] > 1).all()      # the object went towards smaller i: its pixels came from larger i
    hs.close()


def test_camera_pan_centre(pkg, hip):
    sd, cam = cameras(pkg)["cornell_dof"]
    hs = hip.HipScene(sd)
    a = np.radians(2.0)
    eye = np.array([278, 273, -800.0])
    fwd = np.array([np.sin(a), 0, np.cos(a)]) * 800
    prev = pkg.scenes.make_camera(64, 64, 40, eye, eye + fwd, (0, 1, 0), use_dof=True, focal_distance=900, aperture_radius=40)
    got = hs.render_motion(camera=cam, prev_camera=prev, seed=1, centre=True)
    want, _ = centre_motion_f64(pkg, hip, hs, sd, cam, prev, {}, {})
    assert_motion_close(got, want, "centre, 2 degree pan")
    assert bits_equal(got[..., 3], hs.render_aovs(camera=cam, centre=True)[..., 7])
    assert np.abs(got[..., 0][got[..., 3] > 0]).min() > 1  # 2 degrees of a 40 degree field at 64 px: a few pixels everywhere
    hs.close()


# ---------------------------------------------------------------- 6. the point of it all
@pytest.mark.parametrize("normal_test", [False, True])
def test_static_sequence_under_depth_of_field_keeps_its_history(pkg, hip, normal_test):
    """Static Cornell 64 x 64 under depth of field, a moments sequence of six one-sample frames, seeds 1..6.  With centre features every
    covered pixel keeps its whole history -- len counts the frames and the colour is the plain running mean of the six mcpt_render
    frames -- and every other pixel restarts; with sampled features strictly fewer pixels get there."""
    sd, cam = cameras(pkg)["cornell_dof"]
    hs = hip.HipScene(sd)
    H = W = 64
    frames = [hs.render(spp=1, seed=k + 1, camera=cam)[0] for k in range(6)]
    for k, c in enumerate(frames):
        assert np.isfinite(c).all(), k
    cov = hs.render_aovs(camera=cam, centre=True)[..., 7]
    assert set(np.unique(cov)) == {0.0, 1.0}
    covered = cov == 1
    seq = hs.sequence(filter=False, moments=True, centre_features=True, normal_test=normal_test)
    ref = None
    for k in range(6):
        r = seq.frame(camera=cam, want=("fb", "accumulated", "len"), spp=1, seed=k + 1)
        assert bits_equal(r["fb"], frames[k]), k
        ref = frames[k].copy() if k == 0 else ref + (frames[k] - ref) * (f32(1) / f32(k + 1))
        assert ref.dtype == f32
        assert (r["len"][covered] == k + 1).all(), (k, np.unique(r["len"][covered]))
        assert (r["len"][~covered] == 1).all(), k
        assert bits_equal(r["accumulated"][covered], ref[covered]), k
    n_centre = int((r["len"] == 6).sum())
    seq.close()
    seq = hs.sequence(filter=False, moments=True, centre_features=False, normal_test=normal_test)
    for k in range(6):
        r = seq.frame(camera=cam, want=("len",), spp=1, seed=k + 1)
    n_sampled = int((r["len"] == 6).sum())
    print("static DoF Cornell, 6 x 1 spp, normal_test %s: len == 6 on %d pixels with centre features (all %d covered), on %d with sampled ones"
          % (normal_test, n_centre, int(covered.sum()), n_sampled))
    assert n_centre == covered.sum() and n_sampled < n_centre
    seq.close()
    hs.close()


# ---------------------------------------------------------------- 7. the sequence is the composition of the _features calls
@pytest.mark.parametrize("builder", ["sah", "ploc"])
@pytest.mark.parametrize("kind", ["plain", "specular_motion", "adaptive_guided"])
def test_centre_sequence_is_the_composition_of_the_calls(pkg, hip, kind, builder):
    """Six frames with a box moved before each.  With the host builder the separate calls run on a second handle, with PLOC on the
    sequence's own handle before its frame (tests/test_gpu_sequence.py).
      plain            Cornell 64 x 64, 4 spp, specular depth 1 without specular motion: the chain AOVs feed the filter, and the history's
                       depth, normal and motion come from the extra first-hit pass -- all three passes on the centre rays;
      specular_motion  the mirror scene at depth 2, the normal test and the colour clamp on, one sample per pixel with moments;
      adaptive_guided  Cornell 64 x 64, min_spp 2, cap 8: the features come first and guide the rounds."""
    mirror = kind == "specular_motion"
    sd = ms.mirror_scene(pkg) if mirror else pkg.scenes.cornell_demo(64, 64, 8)
    H, W = (ms.H, ms.W) if mirror else (64, 64)
    a = hip.HipScene(sd, builder=builder)
    b = a if builder == "ploc" else hip.HipScene(sd, builder=builder)
    S0, CAP = 2, 8
    if kind == "plain":
        depth, rej, spp = 1, {}, 4
        seq = a.sequence(filter=True, specular_depth=depth, centre_features=True)
    elif mirror:
        depth, rej, spp = 2, dict(normal_test=True, color_clamp=True), 1
        seq = a.sequence(filter=True, specular_depth=depth, specular_motion=True, moments=True, centre_features=True, **rej)
    else:
        depth, rej, spp = 0, {}, CAP
        thr = _mid_threshold(b.render_adaptive(S0, 1e30, spp=S0, seed=1)[2], 0.5)
        seq = a.sequence(filter=True, adaptive=dict(min_spp=S0, threshold=thr, dilate=1, guided=1), centre_features=True)
    hist, length, mom = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W, 2), f32)
    hist_var, prev_depth, prev_normal = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    moved = False
    for k in range(6):
        b.snapshot()
        move = [(ms.BOX, ms.translate(-6.0 + 2.5 * k, 0, 0))] if mirror else [(SHORT, translate(-32.0 * k, 0, 0))]
        info = b.update(move)
        assert info["path"] == (1 if builder == "ploc" else 0)
        if a is not b:
            a.update(move)
        aov = b.render_aovs(seed=k + 1, specular_depth=depth, centre=True)
        # what the history is validated against: the chain AOVs with specular motion, the first hits otherwise
        first = aov if mirror or depth == 0 else b.render_aovs(seed=k + 1, centre=True)
        motion = b.render_motion(seed=k + 1, specular_depth=depth if mirror else 0, centre=True)
        normal = np.ascontiguousarray(first[..., 3:6])
        if kind == "plain":
            rd = b.render_denoised(spp=spp, seed=k + 1, specular_depth=depth)
            fb = rd["fb"]
            acc, acc_var, acc_len = b.temporal_accumulate(fb, rd["variance"], motion, hist, hist_var, prev_depth, length)
        elif mirror:
            fb, _ = b.render(spp=spp, seed=k + 1)
            acc, acc_len, flags, mom = b.temporal_accumulate_moments(fb, motion, normal, hist, prev_depth, length, prev_normal, mom, **rej)
            acc_var = b.moments_variance(mom, acc_len, aov, flags=flags)
        else:
            guide = b.history_len(motion, hist, prev_depth, length)
            fb, cnt, err, var, ainfo, st = b.render_adaptive_guided(S0, thr, guide, dilate=1, spp=CAP, seed=k + 1)
            acc, acc_var, acc_len, _ = b.temporal_accumulate_ex(fb, var, motion, normal, hist, hist_var, prev_depth, length, prev_normal)
        den = b.denoise(acc, acc_var, aov)
        r = seq.frame(want=ALL, spp=spp, seed=k + 1)
        assert r["info"]["frame_index"] == k
        assert bits_equal(r["aov"], aov), k
        assert bits_equal(r["motion"], motion), k
        assert bits_equal(r["fb"], fb), k
        assert bits_equal(r["accumulated"], acc) and bits_equal(r["len"], acc_len), k
        assert bits_equal(r["variance"], acc_var), k
        assert bits_equal(r["denoised"], den), k
        assert np.array_equal(r["rgba"], b.tonemap(den)), k
        if mirror:
            assert np.array_equal(seq.flags(), flags) and bits_equal(seq.moments(), mom), k
        if kind == "adaptive_guided":
            cn = seq.counts()
            assert np.array_equal(cn["spp"], cnt) and bits_equal(cn["err"], err) and bits_equal(cn["guide"], guide), k
            assert cn["info"]["rounds"] == ainfo["rounds"] and cn["info"]["active_pixels"] == ainfo["active_pixels"], k
            assert r["stats"].samples == int(cnt.sum()) == st.samples, k
        moved |= bool((motion[..., 0:2] != 0).any())
        hist, length, hist_var, prev_depth, prev_normal = acc, acc_len, acc_var, first[..., 6].copy(), normal
    assert moved and length.max() == 6
    seq.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 8. errors leave the history as it was
def test_refusals_leave_the_history(pkg, hip, tiny):
    for call in (tiny.render_aovs, tiny.render_motion):
        for kw in (dict(aov_spp=2, centre=True), dict(features=hip.FeatureOpts(centre=2)), dict(aov_spp=-1, centre=True)):
            with pytest.raises(hip.McptError) as e:
                call(**kw)
            assert e.value.code == 1 and "_features" in str(e.value), kw
    bad = hip.FeatureOpts(centre=1)
    bad.reserved[6] = 1
    for kw in (dict(features=bad), dict(features=hip.FeatureOpts(centre=3)), dict(features=hip.FeatureOpts(centre=1), aov_spp=2)):
        with pytest.raises(hip.McptError) as e:
            hip.HipSequence(tiny, filter=False, moments=True, **kw)
        assert e.value.code == 1 and "mcpt_sequence_create" in str(e.value), kw
    seq = tiny.sequence(filter=False, moments=True, centre_features=True)  # the refused creations left the scene usable
    seq.frame(want=("len",), spp=1, seed=1)
    r = seq.frame(want=("len", "accumulated"), spp=1, seed=2)
    m = seq.moments()
    assert r["len"].max() == 2 and r["info"]["frame_index"] == 1
    other = pkg.scenes.make_camera(9, 8, 40, (278, 273, -800), (278, 273, 0))
    for kw in (dict(spp=0), dict(camera=other, spp=1), dict(spp=1, nranks=2), dict(spp=1, spp_total=4), dict(spp=1, accumulate=1), dict(spp=1, sample_offset=1)):
        with pytest.raises(hip.McptError) as e:
            seq.frame(want=("len",), seed=3, **kw)
        assert e.value.code == 1 and "mcpt_sequence_frame" in str(e.value), kw
        assert bits_equal(seq.moments(), m)
    r3 = seq.frame(want=("len", "accumulated"), spp=1, seed=3)
    assert r3["info"]["frame_index"] == 2  # the history went on from where it was
    cov = tiny.render_aovs(centre=True)[..., 7] == 1
    assert (r3["len"][cov] == 3).all() and (r3["len"][~cov] == 1).all()
    # the running mean of three frames on the covered pixels: the second frame's history was not lost
    c3, _ = tiny.render(spp=1, seed=3)
    fin = cov & np.isfinite(c3).all(-1) & np.isfinite(r["accumulated"]).all(-1)
    want = r["accumulated"] + (c3 - r["accumulated"]) * (f32(1) / f32(3))
    assert bits_equal(r3["accumulated"][fin], want[fin])
    seq.close()
