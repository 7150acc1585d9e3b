"""Where k_direct's zero light samples come from (the [mcpt k_direct stats] line the statistics build prints when a scene is destroyed):
light samples, samples with c == 0, and the vertices ALL of whose samples are zero, split by cause -- every emitter behind the tangent
plane (direct_is_zero's half-space rule; the statistics build lists those vertices instead of skipping them), a Dirac BSDF otherwise,
a rough BSDF otherwise.  The second [mcpt k_direct stats] line splits "Dirac otherwise" into reflections, refractions within direct_is_zero's
sin2 < 0.81 gate and vertices beyond it, and says how many of the latter its total-internal-reflection rule claims (the statistics build
lists those too).
python final-project-monte-carlo-path-tracer-with-microfacet-bsdf_amd/build.py --variant stats -DMCPT_TRAVERSAL_STATS; python tools/direct_stats.py"""
import sys, os; sys.path.insert(0, os.getcwd())
import mcpt_loader; pkg = mcpt_loader.load()
lib = os.path.join(os.getcwd(), "final-project-monte-carlo-path-tracer-with-microfacet-bsdf_amd", "libmcpt_hip_stats.so")
for name, sd in (("chess", pkg.scenes.chess_scene(width=1920, height=1080, spp=64)), ("cornell_rc", pkg.scenes.cornell_rc(784, 784, 64)),
                 ("cornell_demo", pkg.scenes.cornell_demo(1920, 1080, 64))):
    hs = pkg.HipScene(sd, library=lib)
    _, st = hs.render(spp=64, seed=1, spp_per_pass=64)
    print("%s: shaded vertices %d, on k_direct's list %d, shadow rays %d" % (name, st.shaded, st.direct_vertices, st.shadow_rays), flush=True)
    hs.close()
