"""direct_is_zero's half-space rule (csrc/mcpt_kernels.hip, DESIGN.md section 6 shortcut 8) on a scene built onto its edges.

The rule, for every material: with c, R the emitters' bounding sphere, L = c - q and |L|^2 > 1.0201 R^2, a vertex (q, n) skips direct
lighting if  n.L < -(R + 1e-5 (|c|_1 + R + |L|_1))  -- all emitters lie behind its tangent plane, so the cosine ws.n that k_direct
computes is negative for every light sample and Material::eval returns 0 in each of its four branches.  The margin 1e-5 is more than
ten times the derived float error bound 12 * 2^-24 (tests/test_direct_halfspace_cpu.py restates rule and margin in numpy).

The scene (halfspace_scene in that file): a ladder of rough-conductor and rough-dielectric quads whose tangent planes pass from 0.3
outside to 0.3 inside the bounding sphere of two emitters 4.4 apart, in steps down to 3e-5 around the margin (1e-4 there) and tilted
by 0, 5e-3 and -2e-2 rad; the quads more than 4e-3 inside have a corner of an emitter in front of them and do receive light.  One quad
is centred on the distance gate D = 1.01 R; a clear_rough_plastic sphere next to the second emitter gives rough refraction seen from
inside.  The checking build evaluates every skipped vertex anyway: mcpt_debug_counters 14 / 15 count the light samples at skipped
vertices and the non-zero ones among them, 12 / 13 the same for the vertices the half-space rule claims.

Negative control: the checking build created with MCPT_HALFSPACE_SLACK_SCALE=-3000 (margin -0.45: the rule then claims every quad of
the ladder, lit ones included) must count non-zero samples on this scene.  Measured on MI355X (32 spp, seed 3): with the rule as
shipped it claims 92 352 light samples, none non-zero (92 532 skipped by all rules together); under the negative control it claims
170 352, of which 561 are non-zero."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("mcpt_halfspace_cpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_direct_halfspace_cpu.py"))
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)


def _render_checked(hip, hip_check, sd, spp, seed):
    hc = hip.HipScene(sd, library=hip_check)
    assert b"checking build" in hc.L.mcpt_version()
    fb, st = hc.render(spp=spp, seed=seed)
    c = hc.debug_counters()
    hc.close()
    return fb, st, [int(c[k]) for k in (12, 13, 14, 15)]


def test_halfspace_rule_on_its_edges(pkg, hip, hip_check, oracle, monkeypatch):
    monkeypatch.delenv("MCPT_HALFSPACE_SLACK_SCALE", raising=False)
    sd, c, R, quads = _cpu.halfspace_scene(pkg)
    fb_check, st_check, (h_samples, h_nonzero, skipped, nonzero) = _render_checked(hip, hip_check, sd, 32, 3)
    print("\n[half-space check] %d light samples at skipped vertices (%d non-zero), of which the half-space rule claims %d (%d non-zero)"
          % (skipped, nonzero, h_samples, h_nonzero))
    assert nonzero == 0 and h_nonzero == 0
    # The rule demonstrably fires: a third of the ladder lies outside the sphere by more than the margin and faces the camera; one pixel
    # of such a quad alone gives 32 spp x 3 channels x 4 light samples = 384 samples.
    assert h_samples > 10000
    # the product build skips those vertices and renders the same frame
    fb, st = hip.HipScene(sd).render(spp=32, seed=3)
    assert np.array_equal(fb, fb_check, equal_nan=True)
    assert st.direct_vertices < st_check.direct_vertices
    assert hip.HipScene(sd).debug_counters().sum() == 0  # the product build counts nothing
    # and the scene itself is rendered correctly
    ref, _ = oracle.OracleScene(sd).render(spp=8, seed=3)
    gpu, _ = hip.HipScene(sd).render(spp=8, seed=3)
    assert pkg.pngio.psnr_u8(pkg.pngio.tonemap_u8(ref), pkg.pngio.tonemap_u8(gpu)) >= 60.0


def test_halfspace_check_can_fail(pkg, hip, hip_check, monkeypatch):
    """The negative control.  MCPT_HALFSPACE_SLACK_SCALE=-3000, read once at scene creation by the checking build only, turns the margin
    into -0.45: the rule claims the whole ladder, and the quads that see a corner of the emitter have non-zero light samples."""
    sd, c, R, quads = _cpu.halfspace_scene(pkg)
    monkeypatch.setenv("MCPT_HALFSPACE_SLACK_SCALE", "-3000")
    _, _, (h_samples, h_nonzero, skipped, nonzero) = _render_checked(hip, hip_check, sd, 32, 3)
    print("\n[half-space check, negative control] scale -3000: the rule claims %d light samples, %d of them non-zero" % (h_samples, h_nonzero))
    assert h_nonzero > 0 and nonzero >= h_nonzero
    # the product library does not read the knob: same frame as without it
    fb_knob, _ = hip.HipScene(sd).render(spp=8, seed=3)
    monkeypatch.delenv("MCPT_HALFSPACE_SLACK_SCALE")
    fb, _ = hip.HipScene(sd).render(spp=8, seed=3)
    assert np.array_equal(fb, fb_knob, equal_nan=True)
    pkgdir = os.path.join(_cpu.ROOT, "final-project-monte-carlo-path-tracer-with-microfacet-bsdf_amd")
    assert b"MCPT_HALFSPACE_SLACK_SCALE" not in open(os.path.join(pkgdir, "libmcpt_hip.so"), "rb").read()
    assert b"MCPT_HALFSPACE_SLACK_SCALE" in open(hip_check, "rb").read()
