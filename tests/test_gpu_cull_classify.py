"""The sky cull's classifier on the device (k_classify, csrc/mcpt_cull.hip) and the candidate-list path of k_primary it feeds:
  (d) mcpt_debug_classify equals the numpy restatement of tests/cull_cases.py exactly -- flags and candidate lists in walk order -- on
      every case of the shared table, over the dump of the live scene's tree; its bound equals mcpt_cull_bound bit for bit;
  (e) 32-spp frames and work counters are identical with the culling on and off; at most 3 values differ from the oracle under SAH;
  (f) equal hit distances go to the larger primitive id through the candidate list as they do through the tree and in the oracle;
  (g) negative control: with rho scaled to 0 (checking build) the conservativeness checker of tests/test_cull_cpu.py does report
      violations."""
import numpy as np
import pytest

import cull_cases as cc

pytestmark = pytest.mark.gpu

f32 = np.float32
SPP = 32


def _live(pkg, hip, monkeypatch, case, cull=True, library=None):
    """The case's scene on the device under the case's tree -> (HipScene, camera, dumped tree)."""
    cc.set_tree(monkeypatch, case)
    if cull:
        monkeypatch.delenv("MCPT_SKY_CULL", raising=False)
    else:
        monkeypatch.setenv("MCPT_SKY_CULL", "0")
    hs = hip.HipScene(cc.scene(pkg, case.scene), library=library)
    bvh = hs.dump_bvh()
    return hs, cc.camera(pkg, case.cam, bvh[0]["root_min"], bvh[0]["root_max"]), bvh


def _same_bits(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.id)
def test_kernel_equals_the_restatement(pkg, hip, oracle, monkeypatch, case):
    hs, cam, bvh = _live(pkg, hip, monkeypatch, case)
    may_hit, cand, info = hs.classify(cam)
    assert _same_bits(info, hip.cull_bound(cam, bvh[0]["root_min"], bvh[0]["root_max"])), info
    assert bvh[0]["n_instances"] == (14 if case.instancing else 0)
    if case.scene == "chain":
        assert hs.info()["bvh_height"] >= 30  # a deep tree: the walk's stack is used to its depth
    ref_hit, ref_cand = cc.classify(bvh, cam, info)
    assert np.array_equal(may_hit, ref_hit), int((may_hit != ref_hit).sum())
    assert np.array_equal(cand, ref_cand), (int((cand != ref_cand).any(axis=1).sum()), cand[(cand != ref_cand).any(axis=1)][:4],
                                            ref_cand[(cand != ref_cand).any(axis=1)][:4])
    cc.check_non_vacuous(case, may_hit, cand)
    if not case.host_tree:  # the trees only the device builds: their classification is checked against the oracle here
        pix, prim = cc.oracle_rays(pkg, oracle, case, cam)
        bad = cc.violations(may_hit, cand, pix, prim)
        assert not bad.any(), (int(bad.sum()), pix[bad][:8], prim[bad][:8], cand[pix[bad][:8]])


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.id)
def test_frames_identical_through_lists_and_through_the_tree(pkg, hip, oracle, monkeypatch, case):
    hs, cam, _ = _live(pkg, hip, monkeypatch, case, cull=True)
    a, sa = hs.render(camera=cam, spp=SPP, seed=3)
    hs.close()
    hs, cam, _ = _live(pkg, hip, monkeypatch, case, cull=False)
    b, sb = hs.render(camera=cam, spp=SPP, seed=3)
    assert np.array_equal(a, b, equal_nan=True), int((a != b).sum())
    assert (sa.samples, sa.vertices, sa.shaded, sa.ref_scene_rays, sa.shadow_rays) == (sb.samples, sb.vertices, sb.shaded, sb.ref_scene_rays, sb.shadow_rays)
    assert sa.closest_rays <= sb.closest_rays
    if case.tree[0] == "sah":
        ref, _ = oracle.OracleScene(cc.scene(pkg, case.scene)).render(camera=cam, spp=SPP, seed=3, n_threads=8)
        same = (a == ref) | (np.isnan(a) & np.isnan(ref))
        assert (~same).sum() <= 3, int((~same).sum())  # (a ray that grazes a box face within float rounding)


def _two_quads(pkg, order):
    """Two coincident quads (two meshes with identical vertex data), emitters of different colours; `order` swaps which comes second."""
    s = pkg.scenes
    b = s._Builder()
    quad = np.zeros(2, s.TRI_DTYPE)
    quad["v0"], quad["v1"], quad["v2"] = [(-10, -10, 0)] * 2, [(10, -10, 0), (10, 10, 0)], [(10, 10, 0), (-10, 10, 0)]
    emit = [(0.9, 0.2, 0.1), (0.1, 0.3, 0.8)]
    for k in (order, 1 - order):
        b.add_mesh(quad.copy(), b.material("emitter%d" % k, s._mat(s.ROUGH_CONDUCTOR, emission=emit[k])))
    cam = s.make_camera(37, 19, 50, (1.5, 0.7, -40), (0, 0, 0), (0, 1, 0), False, 40.0, 1.0)
    return b.finish(camera=cam, rr_rate=0.5, spp=SPP, background=np.float32([0.05, 0.6, 0.25]), name="two_quads"), emit[1 - order]


@pytest.mark.parametrize("order", [0, 1])
def test_equal_distances_go_to_the_larger_primitive_id(pkg, hip, oracle, monkeypatch, order):
    sd, winner = _two_quads(pkg, order)
    monkeypatch.setenv("MCPT_BVH", "sah")
    monkeypatch.delenv("MCPT_QUANT_NODES", raising=False)
    monkeypatch.delenv("MCPT_SKY_CULL", raising=False)
    os_ = oracle.OracleScene(sd)
    hits = os_.primary_hits(SPP, seed=3).reshape(-1, SPP)
    covered, missed = (hits >= 0).all(axis=1), (hits < 0).all(axis=1)
    assert covered.sum() > 50 and missed.sum() > 50 and np.isin(hits[covered], (2, 3)).all()  # the second mesh wins every tie
    hs = hip.HipScene(sd)
    may_hit, cand, info = hs.classify()
    assert info["classified"] == 1 and may_hit[covered].all()
    assert (np.sort(cand[covered], axis=1) == (0, 1, 2, 3)).all()  # the list path decides: all four triangles are candidates
    a, _ = hs.render(spp=SPP, seed=3)
    monkeypatch.setenv("MCPT_SKY_CULL", "0")
    b, _ = hip.HipScene(sd).render(spp=SPP, seed=3)
    assert np.array_equal(a, b), int((a != b).sum())
    ref, _ = os_.render(spp=SPP, seed=3, n_threads=8)
    diff = (a != ref).any(axis=2).reshape(-1)
    assert not diff[covered | missed].any() and (a != ref).sum() <= 3, (int(diff.sum()), int((a != ref).sum()))
    # a depth-0 emitter returns clamp(emission * |cos|): the covered pixels have the winner's hue
    px = a.reshape(-1, 3)[covered].astype(np.float64)
    assert np.allclose(px[:, 0] / px[:, 1], winner[0] / winner[1], rtol=1e-4) and np.allclose(px[:, 2] / px[:, 1], winner[2] / winner[1], rtol=1e-4)


def test_a_bound_scaled_to_zero_is_caught(pkg, hip, hip_check, oracle, monkeypatch):
    """(g) The checking build with MCPT_CULL_RHO_SCALE=0 classifies with unwidened boxes: the checker must object (a tight bound only
    misclassifies; nothing is rendered with it).  The same library without the hook passes."""
    case = next(c for c in cc.CASES if c.cam == "thin_dof" and c.tree == ("sah", None))
    counts = {}
    for scale in (None, "0"):
        if scale is None:
            monkeypatch.delenv("MCPT_CULL_RHO_SCALE", raising=False)
        else:
            monkeypatch.setenv("MCPT_CULL_RHO_SCALE", scale)
        hs, cam, bvh = _live(pkg, hip, monkeypatch, case, library=hip_check)
        may_hit, cand, info = hs.classify(cam)
        assert info["classified"] == 1 and (info["rho"] == 0) == (scale == "0")
        assert np.array_equal(cc.classify(bvh, cam, info)[1], cand)  # the restatement follows the kernel with the wrong bound too
        pix, prim = cc.oracle_rays(pkg, oracle, case, cam)
        counts[scale] = int(cc.violations(may_hit, cand, pix, prim).sum())
        hs.close()
    print("\n[cull negative control] violations: %d with the bound as it is, %d with rho scaled to 0 (%d rays)" % (counts[None], counts["0"], len(pix)))
    assert counts[None] == 0 and counts["0"] >= 1
