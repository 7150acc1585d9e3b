"""Paths and frames through materials outside the nine presets (tests/material_zoo.py): every type with roughness 0 ... 1, indices of
refraction from 0.75 over 1 (index-matched) to 6, texture flags on all types, emission on Dirac and dielectric materials and on either
side of the hasEmission threshold.  Scene::castRay per path and Renderer::Render per frame against the oracle, bit for bit with the
reference's tree, on a cut of the scene that is LDS-resident and on the whole of it, which is not; and the checking build's count of
non-zero light samples at the vertices direct_is_zero skips."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import material_zoo as zoo  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = {"small": zoo.zoo_scene_small, "full": zoo.zoo_scene_full}


def _same_bits(a, b):
    """Element-wise: identical float32 bit patterns, or both NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _first_hit_material(sd, objmat, prim):
    """The material index of the object each primitive id belongs to (-1: background).  Triangle ids are positions in the triangle
    array, a sphere's id is the number of triangles plus its object index."""
    nt = len(sd.triangles)
    m = np.full(len(prim), -1)
    for oi, ob in enumerate(sd.objects):
        if int(ob["kind"]) == 0:
            m[(prim >= int(ob["first_tri"])) & (prim < int(ob["first_tri"]) + int(ob["n_tri"])) & (prim < nt)] = objmat[oi]
        else:
            m[prim == nt + oi] = objmat[oi]
    return m


@pytest.mark.parametrize("cut", ["small", "full"])
def test_zoo_cast_rays_parity(pkg, oracle, hip, cut, tree_env, monkeypatch, capsys):
    """Scene::castRay per path: bit-identical with the reference's tree (the small cut with and without the LDS-resident flavour);
    mismatches under the SAH and the LBVH tree are counted and bounded as in test_cast_rays_parity."""
    monkeypatch.delenv("MCPT_SMALL_SCENE", raising=False)
    sd, objmat = SCENES[cut](96, 64, 4)
    assert len(sd.materials) == (12 if cut == "small" else len(zoo.zoo_materials()[1]) + 2)
    os_ = oracle.OracleScene(sd)
    rng = np.random.default_rng(17)
    W, H = int(sd.camera["width"]), int(sd.camera["height"])
    n = 30000
    pix = rng.integers(0, W * H, size=n).astype(np.uint32)
    smp = rng.integers(0, 1000, size=n).astype(np.uint32)
    ch = rng.integers(0, 3, size=n).astype(np.int32)
    o, d = os_.camera_rays(pix, smp, seed=9)
    # every zoo material is what at least 50 of the rays see first (materials 0 and 1 are the floor and the emitter)
    _, prim = os_.intersect(o, d)
    seen = np.bincount(_first_hit_material(sd, objmat, prim) + 1, minlength=len(sd.materials) + 1)[1:]
    assert seen[2:].min() >= 50, seen
    ref = os_.cast_rays(o, d, pix, smp, ch, seed=9)
    tree_env("reference", "0")
    hs = hip.HipScene(sd)
    assert hs.info()["lds_resident"] == (1 if cut == "small" else 0)
    exact = hs.cast_rays(o, d, pix, smp, ch, seed=9)
    bad = ~_same_bits(ref, exact)
    assert not bad.any(), "reference tree: %d of %d paths differ, e.g. %s vs %s" % (bad.sum(), n, ref[bad][:4], exact[bad][:4])
    if cut == "small":
        monkeypatch.setenv("MCPT_SMALL_SCENE", "0")
        hs = hip.HipScene(sd)
        assert hs.info()["lds_resident"] == 0
        bad = ~_same_bits(ref, hs.cast_rays(o, d, pix, smp, ch, seed=9))
        assert not bad.any(), "reference tree, not LDS-resident: %d of %d paths differ" % (bad.sum(), n)
        monkeypatch.delenv("MCPT_SMALL_SCENE")
    for tree in [("sah", None), ("lbvh", None)]:
        tree_env(*tree)
        gpu = hip.HipScene(sd).cast_rays(o, d, pix, smp, ch, seed=9)
        bad = ~_same_bits(ref, gpu)
        with capsys.disabled():
            print("\n[zoo parity] %s, tree %s: %d of %d paths differ from the oracle (box-grazing rays)" % (cut, tree[0], bad.sum(), n))
        assert bad.sum() <= max(3, n // 10000), (tree, int(bad.sum()))


@pytest.mark.parametrize("cut", ["small", "full"])
def test_zoo_render_is_bit_identical_with_the_reference_tree(pkg, oracle, hip, cut, tree_env, monkeypatch):
    """Renderer::Render end to end, as test_render_is_bit_identical_with_the_reference_tree."""
    monkeypatch.delenv("MCPT_SMALL_SCENE", raising=False)
    sd, _ = SCENES[cut](96, 64, 4)
    tree_env("reference", "0")
    fb_ref, st_ref = oracle.OracleScene(sd).render(spp=4, seed=1)
    fb_gpu, st_gpu = hip.HipScene(sd).render(spp=4, seed=1, spp_per_pass=3)
    bad = ~_same_bits(fb_ref, fb_gpu)
    assert not bad.any(), "%d of %d framebuffer values differ" % (bad.sum(), bad.size)
    assert st_gpu.vertices == st_ref.vertices and st_gpu.ref_scene_rays == st_ref.scene_rays


@pytest.mark.parametrize("cut", ["small", "full"])
def test_zoo_direct_skips_lose_no_light(pkg, hip, hip_check, cut, monkeypatch):
    """The checking build evaluates the vertices direct_is_zero skips anyway: mcpt_debug_counters 14 / 15 count the light samples there
    and the non-zero ones among them, 10 / 11 the same for the total-internal-reflection rule.  The product frame is the checking frame."""
    for k in ("MCPT_SMALL_SCENE", "MCPT_TIR_BOUND_SCALE", "MCPT_CONE_TOL_SCALE", "MCPT_HALFSPACE_SLACK_SCALE"):
        monkeypatch.delenv(k, raising=False)
    sd, _ = SCENES[cut](96, 64, 16)
    hc = hip.HipScene(sd, library=hip_check)
    assert b"checking build" in hc.L.mcpt_version()
    fb_check, _ = hc.render(spp=16, seed=5)
    c = [int(v) for v in hc.debug_counters()]
    hc.close()
    print("\n[zoo check] %s: %d light samples at skipped vertices (%d non-zero), of which the total-internal-reflection rule claims %d (%d non-zero)"
          % (cut, c[14], c[15], c[10], c[11]))
    assert c[15] == 0 and c[11] == 0
    assert c[14] > 1000
    fb, _ = hip.HipScene(sd).render(spp=16, seed=5)
    assert np.array_equal(fb, fb_check, equal_nan=True)
