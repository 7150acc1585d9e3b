"""One ray set through every instantiation of the shared traversal pieces (csrc/mcpt_traverse.h: node visit, descend step, stack, leaf
test, closest update): float / quantised / prepared nodes, instanced or not, plain / retry / scratch stacks, k_trace_closest and its
lane-refill form.  Every flavour must return the oracle's hits: the same primitive for every ray, a bit-equal t wherever there is one.
Ray counts straddle the refill kernel's 256-ray chunk of a wave and 1024-ray chunk of a workgroup; the first tenth of every set has a
zero direction component (the NaN-faithful slab chain, traced by the generic loop before the refill loop starts)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (1, 255, 257, 1023, 1025, 5000)
SCENES = {"chess": lambda s: s.chess_scene(width=160, height=90, spp=1), "cornell": lambda s: s.cornell_demo(64, 64, 1)}
# flavour -> (HipScene keywords, checking library, MCPT_SMALL_SCENE=0)
FLAVOURS = {"default": ({}, False, False), "float_nodes": (dict(quantise=0), False, False), "check": ({}, True, False),
            "instanced_float": (dict(instancing=True, quantise=0), False, False), "instanced_quantised": (dict(instancing=True, quantise=1), False, False),
            "not_lds_resident": ({}, False, True)}
CASES = [("chess", f) for f in ("default", "float_nodes", "instanced_float", "instanced_quantised", "check")] + \
        [("cornell", f) for f in ("default", "float_nodes", "not_lds_resident", "check")]
_cache = {}


def _rays_and_reference(pkg, hip, oracle, scene):
    """Per ray count: (origins, directions, the oracle's t, the oracle's prim).  Computed once per scene and left unchanged."""
    if scene not in _cache:
        sd = SCENES[scene](pkg.scenes)
        rng = np.random.default_rng(23)
        w, h = int(sd.camera["width"]), int(sd.camera["height"])
        hs, os_ = hip.HipScene(sd), oracle.OracleScene(sd)
        sets = []
        for n in COUNTS:
            o, d = hs.camera_rays(rng.integers(0, w * h, n).astype(np.uint32), rng.integers(0, 64, n).astype(np.uint32), seed=3)
            d = d.copy()
            k = (n + 9) // 10
            d[np.arange(k), np.arange(k) % 3] = 0.0
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            t, p = os_.intersect(o, d)
            for a in (o, d, t, p):
                a.setflags(write=False)
            sets.append((o, d, t, p))
        hs.close()
        _cache[scene] = (sd, sets)
    return _cache[scene]


@pytest.mark.parametrize("scene,flavour", CASES)
def test_every_traversal_flavour_returns_the_oracles_hits(pkg, hip, hip_check, oracle, monkeypatch, scene, flavour):
    sd, sets = _rays_and_reference(pkg, hip, oracle, scene)
    kw, check, not_small = FLAVOURS[flavour]
    if not_small:
        monkeypatch.setenv("MCPT_SMALL_SCENE", "0")
    hs = hip.HipScene(sd, library=hip_check if check else None, **kw)
    info = hs.info()
    if flavour.startswith("instanced"):
        assert info["n_instances"] > 0
    if "quantise" in kw:
        assert info["quantised"] == kw["quantise"]
    if scene == "cornell" and not check:
        assert info["lds_resident"] == (0 if not_small else 1)
    for o, d, t_ref, p_ref in sets:
        t, p = hs.intersect(o, d)
        assert len(p) == len(p_ref)  # no ray is left out
        assert np.array_equal(p, p_ref), (len(p), int((p != p_ref).sum()))
        hit = p_ref >= 0
        assert np.array_equal(t[hit].view(np.uint64), t_ref[hit].view(np.uint64)), (len(p), int((t[hit] != t_ref[hit]).sum()))
    hs.close()
