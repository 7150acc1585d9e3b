"""direct_is_zero's total-internal-reflection rule (csrc/mcpt_kernels.hip, DESIGN.md section 6 shortcut 8) on a scene built onto its bound.

The rule: a Dirac dielectric seen from inside with  sin2 = ior^2 |wo_t|^2 > 1.001 (1 + 0.0143 (1 + ior))^2  skips direct lighting: no
direction ws passes Material::eval's `h.N >= 1 - EPSILON` (tests/test_direct_tir_cpu.py restates the proof in numpy).

The scene (tir_scene in that file): 36 glass prisms, indices of refraction 1.5 and 1.8, whose second face the camera's ray meets from
inside at the bound's angle -5 ... +5 degrees in steps down to 0.1, and one long emitter near the tangent plane of those faces, opposite
wo_t: where the refracted ray leaves just short of total internal reflection and where eval comes closest to passing just beyond it.
The checking build evaluates every skipped vertex anyway: mcpt_debug_counters 14 / 15 count the light samples at skipped vertices and
the non-zero ones among them, 10 / 11 the same for the vertices the total-internal-reflection rule claims.  A kernel whose bound were
too low (a plain sin2 > 1, a constant 0.00143) would claim the prisms 0.1 to 1.5 degrees short of the shipped bound, which the emitter
does light.

Negative control: the checking build created with MCPT_TIR_BOUND_SCALE=0.85 (ior 1.5: sin2 > 0.91 instead of 1.07) claims those prisms
and must count non-zero samples."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("mcpt_tir_cpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_direct_tir_cpu.py"))
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)


def _render_checked(hip, hip_check, sd, spp, seed):
    hc = hip.HipScene(sd, library=hip_check)
    assert b"checking build" in hc.L.mcpt_version()
    fb, st = hc.render(spp=spp, seed=seed)
    c = hc.debug_counters()
    hc.close()
    return fb, st, [int(c[k]) for k in (10, 11, 14, 15)]


def test_tir_rule_on_its_bound(pkg, hip, hip_check, oracle, monkeypatch):
    monkeypatch.delenv("MCPT_TIR_BOUND_SCALE", raising=False)
    sd, items, _ = _cpu.tir_scene()
    fb_check, st_check, (t_samples, t_nonzero, skipped, nonzero) = _render_checked(hip, hip_check, sd, 32, 3)
    print("\n[tir check] %d light samples at skipped vertices (%d non-zero), of which the total-internal-reflection rule claims %d (%d non-zero)"
          % (skipped, nonzero, t_samples, t_nonzero))
    assert nonzero == 0 and t_nonzero == 0
    # The rule demonstrably fires: 18 prisms lie beyond the bound (test_tir_scene_straddles_the_rule), each entry face 4 x 4 pixels, and
    # 96 % of the camera's paths enter the glass: at least 18 x 8 pixels x 32 spp x 3 channels x 4 light samples = 55 296.
    assert t_samples > 50000
    # the product build skips those vertices and renders the same frame
    fb, st = hip.HipScene(sd).render(spp=32, seed=3)
    assert np.array_equal(fb, fb_check, equal_nan=True)
    assert st.direct_vertices < st_check.direct_vertices
    assert hip.HipScene(sd).debug_counters().sum() == 0  # the product build counts nothing
    # and the scene itself is rendered correctly
    ref, _ = oracle.OracleScene(sd).render(spp=8, seed=3)
    gpu, _ = hip.HipScene(sd).render(spp=8, seed=3)
    assert pkg.pngio.psnr_u8(pkg.pngio.tonemap_u8(ref), pkg.pngio.tonemap_u8(gpu)) >= 60.0


def test_tir_check_can_fail(pkg, hip, hip_check, monkeypatch):
    """The negative control.  MCPT_TIR_BOUND_SCALE=0.85, read once at scene creation by the checking build only, lowers the bound below
    total internal reflection: the prisms just short of the shipped bound are claimed, and the emitter lights them."""
    sd, items, _ = _cpu.tir_scene()
    monkeypatch.setenv("MCPT_TIR_BOUND_SCALE", "0.85")
    _, _, (t_samples, t_nonzero, skipped, nonzero) = _render_checked(hip, hip_check, sd, 32, 3)
    print("\n[tir check, negative control] scale 0.85: the rule claims %d light samples, %d of them non-zero" % (t_samples, t_nonzero))
    assert t_nonzero > 0 and nonzero >= t_nonzero
    # the product library does not read the knob: same frame as without it
    fb_knob, _ = hip.HipScene(sd).render(spp=8, seed=3)
    monkeypatch.delenv("MCPT_TIR_BOUND_SCALE")
    fb, _ = hip.HipScene(sd).render(spp=8, seed=3)
    assert np.array_equal(fb, fb_knob, equal_nan=True)
    pkgdir = os.path.join(_cpu.ROOT, "final-project-monte-carlo-path-tracer-with-microfacet-bsdf_amd")
    assert b"MCPT_TIR_BOUND_SCALE" not in open(os.path.join(pkgdir, "libmcpt_hip.so"), "rb").read()
    assert b"MCPT_TIR_BOUND_SCALE" in open(hip_check, "rb").read()


@pytest.mark.parametrize("name", ["chess", "cornell_rc", "cornell_demo"])
def test_tir_rule_on_the_shipped_scenes(pkg, hip, hip_check, name, monkeypatch):
    """The three shipped scenes: no non-zero sample at a skipped vertex, and the product frame equals the checking frame bit for bit."""
    monkeypatch.delenv("MCPT_TIR_BOUND_SCALE", raising=False)
    s = pkg.scenes
    sd = {"chess": lambda: s.chess_scene(width=480, height=270, spp=16), "cornell_rc": lambda: s.cornell_rc(196, 196, 16),
          "cornell_demo": lambda: s.cornell_demo(480, 270, 16)}[name]()
    fb_check, _, (t_samples, t_nonzero, skipped, nonzero) = _render_checked(hip, hip_check, sd, 16, 5)
    print("\n[tir check] %s: %d light samples at skipped vertices (%d non-zero), of which the total-internal-reflection rule claims %d (%d non-zero)"
          % (name, skipped, nonzero, t_samples, t_nonzero))
    assert nonzero == 0 and t_nonzero == 0
    if name != "cornell_rc":  # (glass pieces and a glass sphere: the rule has work there; cornell_rc has no glass)
        assert t_samples > 0
    fb, _ = hip.HipScene(sd).render(spp=16, seed=5)
    assert np.array_equal(fb, fb_check, equal_nan=True)
