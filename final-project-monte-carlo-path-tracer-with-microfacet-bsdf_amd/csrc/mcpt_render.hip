// The frame-level entry points of the C ABI (include/mcpt.h): mcpt_render / mcpt_render_device, mcpt_render_adaptive[_guided | _denoised], mcpt_render_aovs[_ex],
// mcpt_denoise, mcpt_render_denoised and mcpt_render_motion[_ex].  What they share -- the checks of (camera, params), the start of a call, its statistics -- is
// here once; each entry point is the part that differs.  csrc/mcpt_frame.h declares what csrc/mcpt_sequence.hip uses of it.
#include <cmath>
#include <cstdio>

#include "mcpt_frame.h"

using namespace mcpt;

void mcpt::add(mcpt_stats &a, const mcpt_stats &b) {
    a.samples += b.samples; a.paths += b.paths; a.vertices += b.vertices; a.shaded += b.shaded;
    a.closest_rays += b.closest_rays; a.shadow_rays += b.shadow_rays; a.ref_scene_rays += b.ref_scene_rays;
    a.iterations += b.iterations; a.overflow_paths += b.overflow_paths; a.direct_vertices += b.direct_vertices;
    a.ms_trace_closest += b.ms_trace_closest; a.ms_trace_shadow += b.ms_trace_shadow; a.ms_shade += b.ms_shade;
    a.ms_generate += b.ms_generate; a.ms_resolve += b.ms_resolve; a.ms_direct += b.ms_direct;
    a.n_trace_closest += b.n_trace_closest; a.n_trace_shadow += b.n_trace_shadow; a.n_shade += b.n_shade;
    a.n_generate += b.n_generate; a.n_resolve += b.n_resolve; a.n_direct += b.n_direct;
}

int mcpt::check_frame_call(const char *name, const mcpt_camera &cam, const mcpt_params &p, unsigned forbid) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    const bool positive = cam.width > 0 && cam.height > 0 && p.n_dir_sample > 0 && p.rr_rate > 0.f;
    if (forbid & kDenoisedFrame) {
        if (!positive || !frame_ok(cam.width, cam.height)) return bad("width/height/n_dir_sample/rr_rate must be positive");
        if (p.spp < ((forbid & kOneSample) ? 1 : 2)) return bad((forbid & kOneSample) ? "params.spp must be at least 1" : "params.spp must be at least 2");
    } else {
        if (!positive || p.spp <= 0) return bad("width/height/spp/n_dir_sample/rr_rate must be positive");
        if ((uint64_t)cam.width * cam.height > 0x7fffffffull) return bad("frame too large");
    }
    if ((forbid & kOneRank) && p.nranks != 1) return bad("nranks must be 1 (a partitioned frame is not denoised)");
    if ((forbid & kOneCallFrame) && (p.accumulate != 0 || p.spp_total != 0 || p.sample_offset != 0))
        return bad("accumulate, spp_total and sample_offset must be 0");
    return MCPT_OK;
}

void mcpt::fill_stats(mcpt_stats *stats, uint64_t samples, uint64_t traced_primary, int32_t n_dir, const Totals &rt, Clock::time_point t0) {
    std::memset(stats, 0, sizeof *stats);
    // (culled pixels count like traced ones: the reference runs one camera ray and three castRay invocations, each with one
    // Scene::intersect, for every sample of them too)
    stats->samples = samples;
    stats->paths = 3 * stats->samples;
    stats->vertices = stats->paths + rt.pushes;
    stats->shaded = rt.shaded;
    stats->closest_rays = rt.closest;
    stats->shadow_rays = rt.shadow;
    stats->direct_vertices = rt.direct;
    // Scene::intersect calls of the reference: one per castRay invocation (Scene.cpp:87), n_dir per shaded
    // vertex (Scene.cpp:73), one look-ahead per vertex that survives roulette (Scene.cpp:134,161).
    const uint64_t cont = rt.closest - traced_primary;  // closest-hit rays beyond the primary rays actually traced
    stats->ref_scene_rays = stats->vertices + (uint64_t)n_dir * rt.shaded + cont;
    stats->iterations = rt.iterations;
    stats->overflow_paths = rt.overflow;
    stats->ms_trace_closest = rt.ms[K_CLOSEST];
    stats->ms_trace_shadow = rt.ms[K_SHADOW];
    stats->ms_shade = rt.ms[K_SHADE];
    stats->ms_generate = rt.ms[K_GENERATE];
    stats->ms_resolve = rt.ms[K_RESOLVE];
    stats->ms_direct = rt.ms[K_DIRECT];
    stats->n_direct = rt.cnt[K_DIRECT];
    stats->n_trace_closest = rt.cnt[K_CLOSEST];
    stats->n_trace_shadow = rt.cnt[K_SHADOW];
    stats->n_shade = rt.cnt[K_SHADE];
    stats->n_generate = rt.cnt[K_GENERATE];
    stats->n_resolve = rt.cnt[K_RESOLVE];
    stats->ms_total = ms_since(t0);
}

namespace {

constexpr uint32_t kAovChunkRays = 4u << 20;   // at most this many rays per chunk of the AOV pass
constexpr uint32_t kMotionMapRays = 1u << 20;  // ... and of the motion pass with specular chains: 96 bytes of maps per ray, 96 MiB

int render_impl(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, float *fb_dev, hipStream_t st, mcpt_stats *stats) {
    if (!sc || !cam || !pp || !fb_dev) return fail(MCPT_ERR_ARG, "mcpt_render: null argument");
    const mcpt_params &p = *pp;
    int rc = check_frame_call("mcpt_render", *cam, p, 0);
    if (rc != MCPT_OK) return rc;
    FrameCall f{sc, p};
    if ((rc = f.begin(*cam)) != MCPT_OK) return rc;
    const float spp_total = (float)(p.spp_total > 0 ? p.spp_total : p.spp);
    if ((rc = f.pixels(p.spp, spp_total, fb_dev, st)) != MCPT_OK) return rc;
    const PixelSet &ps = f.ps;
    if (ps.n_owned == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        if (stats) std::memset(stats, 0, sizeof *stats);
        return MCPT_OK;
    }
    Totals rt;
    rc = render_list(sc, f.cc, p, ps.list, ps.cand, ps.n_pix, p.sample_offset, p.spp, spp_total, fb_dev, nullptr, st, f.t0, rt);
    if (rc != MCPT_OK) return rc;
    return f.end(stats, (uint64_t)ps.n_owned * p.spp, (uint64_t)ps.n_pix * p.spp, rt);
}

// What the chunk loop of the AOV pass works in.
struct AovPtrs {
    uint32_t *key_pixel, *key_sample;
    float4 *rec0, *rec1;  // the per-sample records
    // ray list 0 holds the camera rays and their hits; the specular chains add ray list 1, the chain states and sums of both lists and the
    // count of the next list (all nullptr without chains)
    float4 *list_o[2], *list_d[2];
    uint4 *list_hit[2];
    float4 *chain_st[2];
    double *chain_t[2];
    uint32_t *n_next;
    RetryList rl;
    bool in_ws;  // the arrays are the workspace's (aov_in_workspace), not the call's own (AovOwn)
};

// ... inside the wavefront workspace (aov_pass says what goes where) ...
// Not named here and free for a feature pass to use: the shadow queue (shq_o, shq_d), the clamp stack, contrib and fresh.  Nothing in them
// outlives a render: k_shade fills the shadow queue and k_trace_shadow drains it within one iteration.  lit_pass keeps p in shq_o.
AovPtrs aov_in_workspace(const Workspace &w, uint64_t cap, bool chain) {
    uint32_t *keys = reinterpret_cast<uint32_t *>(w.wave[1].rec0.p);
    AovPtrs a{keys, keys + cap, w.wave[1].ray_o.p, w.wave[1].ray_d.p, {w.wave[0].ray_o.p, nullptr}, {w.wave[0].ray_d.p, nullptr}, {w.wave[0].hit.p, nullptr},
              {nullptr, nullptr}, {nullptr, nullptr}, nullptr, w.retry.list(0), true};
    if (chain) {
        a.list_o[1] = w.vtx0.p;
        a.list_d[1] = w.vtx1.p;
        a.list_hit[1] = w.wave[1].hit.p;
        a.chain_st[0] = w.wave[0].rec1.p;
        a.chain_st[1] = w.wave[1].rec1.p;
        a.chain_t[0] = reinterpret_cast<double *>(w.wave[0].rec0.p);
        a.chain_t[1] = reinterpret_cast<double *>(w.vtx2.p);
        a.n_next = w.vtx_j.p;
    }
    return a;
}

// ... or in buffers of the call's own, for chunks of `cap` rays.
struct AovOwn {
    DevBuf<uint32_t> keys, count;
    DevBuf<float4> s0, s1, ray_o[2], ray_d[2], chain_st[2];
    DevBuf<double> chain_t[2];
    DevBuf<uint4> hit[2];
    RetryBufs retry;
    hipError_t alloc(uint64_t cap, bool chain, bool with_keys, int height, AovPtrs &a) {
        hipError_t e = with_keys ? keys.alloc(2 * cap) : hipSuccess;
        const auto also = [&](auto &buf, size_t n) {
            if (e == hipSuccess) e = buf.alloc(n);
        };
        also(ray_o[0], cap);
        also(ray_d[0], cap);
        also(hit[0], cap);
        also(s0, cap);
        also(s1, cap);
        if (e == hipSuccess) e = retry.for_rays((uint32_t)cap, height);
        if (chain) {
            also(ray_o[1], cap);
            also(ray_d[1], cap);
            also(hit[1], cap);
            also(count, 1);
            for (int k = 0; k < 2; ++k) {
                also(chain_st[k], cap);
                also(chain_t[k], cap);
            }
        }
        a = AovPtrs{keys.p, with_keys ? keys.p + cap : nullptr, s0.p, s1.p, {ray_o[0].p, ray_o[1].p}, {ray_d[0].p, ray_d[1].p}, {hit[0].p, hit[1].p},
                    {chain_st[0].p, chain_st[1].p}, {chain_t[0].p, chain_t[1].p}, count.p, retry.list(0), false};
        return e;
    }
};

// The chunk loop the AOV pass and the motion pass share: for chunks of whole pixels, pixel-major, the keys, the camera rays and the closest
// hits of samples 0 .. aov_spp-1 of `seed`, queued on `st`; resolve(a, p0, np, n) then turns the n traced rays of the chunk's np pixels
// (from pixel p0) into the pass's own records and folds them (it returns an mcpt status).  The loop runs inside the wavefront workspace of
// pool 0 when that holds at least one pixel's rays (after a render it holds millions): camera rays and hits in wave 0's ray / hit arrays,
// the per-sample records in wave 1's, the keys in wave 1's path records, the retrace list of the closest-hit rays.  Otherwise (no render
// yet on this scene) it uses buffers of its own for the call.  `chain`: the second ray list and the chain states of the specular chains
// are needed too (in the workspace: vtx0 / vtx1 with wave 1's hits, wave 0's and wave 1's rec1, the sums in wave 0's rec0 and vtx2, the
// count vtx_j[0]; chunks then hold at most `pool` rays); chain_bounces, below, is the loop a resolve runs over them.
// max_rays > 0: no chunk holds more rays than that (at least aov_spp: the motion pass's map storage, motion_pass).
// centre (mcpt_feature_opts; aov_spp is then 1): ray j of a chunk is the centre ray of pixel p0 + j, from k_centre_rays alone; the key
// arrays are neither written nor read (nor allocated, where the call owns its buffers) and `seed` is not looked at.
template <class Resolve>
int first_hit_chunks(mcpt_scene *sc, const CameraConst &cc, uint32_t seed, int32_t aov_spp, bool centre, bool chain, uint64_t max_rays, hipStream_t st,
                     Resolve &&resolve) {
    const uint32_t n_px = (uint32_t)cc.width * (uint32_t)cc.height;
    const uint64_t need = std::min<uint64_t>(max_rays ? std::min<uint64_t>(kAovChunkRays, max_rays) : kAovChunkRays, (uint64_t)n_px * aov_spp);
    Workspace &w = sc->pools[0].ws;
    // rays that fit: the ray arrays (ray_cap entries) and, for the keys, two uint32 per ray in wave 1's rec0 (4 per entry); the chains use
    // arrays of `pool` entries too
    const uint64_t ws_rays = w.pool ? std::min<uint64_t>(w.ray_cap, (chain ? 1ull : 2ull) * w.pool) : 0;
    const bool in_ws = ws_rays >= (uint64_t)aov_spp && (!stack_uses_retry(sc->view.height) || w.retry.cap[0] >= std::min<uint64_t>(need, ws_rays));
    const uint64_t cap = in_ws ? std::min<uint64_t>(need, ws_rays) : need;
    AovOwn own;
    AovPtrs a;
    if (in_ws) a = aov_in_workspace(w, cap, chain);
    else HIP_TRY(own.alloc(cap, chain, !centre, sc->view.height, a));
    const uint32_t px_chunk = (uint32_t)std::max<uint64_t>(1, cap / (uint64_t)aov_spp);
    for (uint32_t p0 = 0; p0 < n_px; p0 += px_chunk) {
        const uint32_t np = std::min(px_chunk, n_px - p0), n = np * (uint32_t)aov_spp;
        if (centre) {
            launch_centre_rays(cc, p0, n, a.list_o[0], a.list_d[0], st);
        } else {
            launch_aov_keys(p0, n, aov_spp, a.key_pixel, a.key_sample, st);
            launch_camera_rays(cc, seed, n, a.key_pixel, a.key_sample, a.list_o[0], a.list_d[0], st);
        }
        launch_trace_closest(sc->view, n, nullptr, a.list_o[0], a.list_d[0], a.list_hit[0], a.rl, st);
        const int rc = resolve(a, p0, np, n);
        if (rc != MCPT_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    if (!in_ws) HIP_TRY(hipStreamSynchronize(st));  // (the call's own buffers are freed on return)
    return MCPT_OK;
}

// The bounce loop of a chunk's specular chains, which aov_pass, lit_pass and motion_pass share: step(b, cur, m) launches the pass's chain
// kernel on the m rays of list `cur`, whose samples have all followed b bounces (list 0 holds the chunk's n traced camera rays); the kernel
// appends the rays that continue to list cur ^ 1 and counts them in n_next, which is read back once per bounce (the stream drains) before
// their closest hits are traced.  The loop ends after the step of bounce spec_depth, or when no sample continues.  spec_depth 0: one
// step, and n_next is neither cleared nor read.
template <class Step>
int chain_bounces(const DevScene &S, const AovPtrs &a, uint32_t n, int32_t spec_depth, hipStream_t st, Step &&step) {
    uint32_t m = n;
    for (int b = 0, cur = 0;; ++b, cur ^= 1) {
        if (b < spec_depth) HIP_TRY(hipMemsetAsync(a.n_next, 0, sizeof(uint32_t), st));
        step(b, cur, m);
        if (b == spec_depth) break;
        HIP_TRY(hipMemcpyAsync(&m, a.n_next, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (m == 0) break;
        launch_trace_closest(S, m, nullptr, a.list_o[cur ^ 1], a.list_d[cur ^ 1], a.list_hit[cur ^ 1], a.rl, st);
    }
    return MCPT_OK;
}

}  // namespace

// The AOV pass (include/mcpt.h): aov_dev[8m ..] for every pixel of the frame.  Per chunk k_aov_resolve, or with spec_depth > 0
// (mcpt_render_aovs_ex) the specular chains -- chain_bounces: k_aov_chain on the traced list, then up to spec_depth times k_trace_closest +
// k_aov_chain on the compacted list of the samples that continue -- and k_aov_fold.
int mcpt::aov_pass(mcpt_scene *sc, const CameraConst &cc, uint32_t seed, int32_t aov_spp, int32_t spec_depth, bool centre, float *aov_dev, hipStream_t st) {
    const bool chain = spec_depth > 0;
    return first_hit_chunks(sc, cc, seed, aov_spp, centre, chain, 0, st, [&](const AovPtrs &a, uint32_t p0, uint32_t np, uint32_t n) -> int {
        if (!chain) {
            launch_aov_resolve(sc->view, n, a.list_o[0], a.list_d[0], a.list_hit[0], a.rec0, a.rec1, st);
        } else {
            const int rc = chain_bounces(sc->view, a, n, spec_depth, st, [&](int b, int cur, uint32_t m) {
                launch_aov_chain(sc->view, m, b, spec_depth, a.list_o[cur], a.list_d[cur], a.list_hit[cur], b == 0 ? nullptr : a.chain_st[cur],
                                 b == 0 ? nullptr : a.chain_t[cur], a.rec0, a.rec1, a.list_o[cur ^ 1], a.list_d[cur ^ 1], a.chain_st[cur ^ 1],
                                 a.chain_t[cur ^ 1], a.n_next, st);
            });
            if (rc != MCPT_OK) return rc;
        }
        launch_aov_fold(p0, np, aov_spp, a.rec0, a.rec1, aov_dev, st);
        return MCPT_OK;
    });
}

// The lit pass (include/mcpt.h: mcpt_render_probe_lit; csrc/mcpt_frame.h says what goes where).
int mcpt::lit_pass(mcpt_scene *sc, const CameraConst &cc, uint32_t seed, int32_t aov_spp, int32_t spec_depth, bool centre, const LitVolume &vol,
                   float *lit_dev, float *position_dev, unsigned long long *lookups_dev, hipStream_t st, mcpt_lit_info &info, const LitDirect *direct,
                   mcpt_lit_direct_info *dinfo) {
    const bool chain = spec_depth > 0 || direct;
    const Workspace &w = sc->pools[0].ws;
    DevBuf<float4> own_p;  // p per sample of a chunk, when the workspace has no room for it (the first chunk is the largest)
    HIP_TRY(hipMemsetAsync(lookups_dev, 0, (direct ? 2 : 1) * sizeof(unsigned long long), st));
    int32_t pieces = 0;
    uint32_t stage_cap = 0;  // light samples a piece of the direct term may stage
    const int rc = first_hit_chunks(sc, cc, seed, aov_spp, centre, chain, 0, st, [&](const AovPtrs &a, uint32_t p0, uint32_t np, uint32_t n) -> int {
        float4 *rec2 = a.in_ws && w.shq_o.n >= n ? w.shq_o.p : nullptr;
        if (!rec2) {
            HIP_TRY(own_p.alloc(n));
            rec2 = own_p.p;
        }
        info.in_workspace = a.in_ws ? 1 : 0;
        info.chunks++;
        const int cr = chain_bounces(sc->view, a, n, spec_depth, st, [&](int b, int cur, uint32_t m) {
            launch_lit_terminal(sc->view, m, b, spec_depth, a.list_o[cur], a.list_d[cur], a.list_hit[cur], b == 0 ? nullptr : a.chain_st[cur], a.rec0, a.rec1,
                                rec2, a.list_o[cur ^ 1], a.list_d[cur ^ 1], a.chain_st[cur ^ 1], a.n_next, st);
        });
        if (cr != MCPT_OK) return cr;
        float4 *direct_d = nullptr;
        if (direct) {
            direct_d = a.chain_st[0];
            if (sc->view.n_lights == 0) {  // (an empty light table: D = 0, no ray)
                HIP_TRY(hipMemsetAsync(direct_d, 0, (size_t)n * sizeof(float4), st));
            } else {
                DirectRays src{};
                src.seed = direct->seed;
                src.N = direct->n_samples;
                src.r0 = a.rec0;
                src.r1 = a.rec1;
                src.r2 = rec2;
                src.surface_kind = kLitSurfaceKind;
                src.p0 = p0;
                src.aov_spp = aov_spp;
                src.total = lookups_dev + 1;
                if (!stage_cap) stage_cap = n;  // (the first chunk is the largest, and every list array holds at least its rays)
                const PieceCut cut = piece_cut(n, (uint64_t)direct->n_samples, stage_cap, 1);
                const int dr = direct_term(sc->view, src, n, DirectStage{a.list_o[0], a.list_d[0], a.list_o[1], a.list_hit[0], a.n_next, cut, a.rl},
                                           reinterpret_cast<float *>(direct_d), 4u, st, pieces);
                if (dr != MCPT_OK) return dr;
            }
        }
        launch_lit_shade(vol, n, a.rec0, a.rec1, rec2, direct_d, lookups_dev, st);
        launch_lit_fold(p0, np, aov_spp, a.rec0, rec2, lit_dev, position_dev, st);
        return MCPT_OK;
    });
    if (rc != MCPT_OK) return rc;
    unsigned long long lookups[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(lookups, lookups_dev, (direct ? 2 : 1) * sizeof lookups[0], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    info.samples = (int64_t)cc.width * cc.height * aov_spp;
    info.lookups = (int64_t)lookups[0];
    if (direct && dinfo) {
        dinfo->light_samples = (int64_t)lookups[0] * direct->n_samples;
        dinfo->shadow_rays = (int64_t)lookups[1];
        dinfo->pieces = pieces;
    }
    return MCPT_OK;
}

namespace {

// What a projection of the motion pass reads of a camera (csrc/mcpt_temporal.h)
tp::Cam motion_camera(const CameraConst &cc) {
    tp::Cam c;
    c.width = cc.width;
    c.height = cc.height;
    c.scale = cc.scale;
    c.aspect = cc.aspect;
    for (int k = 0; k < 3; ++k) c.eye[k] = cc.eye[k];
    for (int k = 0; k < 9; ++k) c.orient[k] = cc.orient[k];
    return c;
}

}  // namespace

int mcpt::check_features(const char *name, const mcpt_feature_opts *features, int32_t aov_spp, bool &centre) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    centre = false;
    if (!features) return MCPT_OK;
    if (features->centre != 0 && features->centre != 1) return bad("features: centre must be 0 or 1");
    for (int k = 0; k < 7; ++k)
        if (features->reserved[k] != 0) return bad("features: reserved words must be 0");
    if (features->centre == 1 && aov_spp > 1) return bad("features: centre 1 takes one feature ray per pixel (aov_spp must be 0 or 1)");
    centre = features->centre == 1;
    return MCPT_OK;
}

uint64_t mcpt::motion_map_rays(uint64_t n_px, int32_t aov_spp) { return std::min<uint64_t>(kMotionMapRays, n_px * (uint64_t)aov_spp); }

// The motion pass (include/mcpt.h: mcpt_render_motion[_ex]): motion_dev[4m ..] for every pixel of the frame, from the rays and hits of the AOV
// pass.  Per chunk k_motion_resolve and k_motion_fold (csrc/mcpt_temporal.hip); prev_tri / prev_sph are the snapshot's arrays, or the live
// ones for a scene without a snapshot.  With spec_depth > 0 the specular chains: chain_bounces with k_motion_chain in
// k_aov_chain's place, on the arrays of aov_in_workspace(.., chain = true) or AovOwn of which it uses the two ray lists with their hits,
// chain_st[0 / 1] for {reflections, sample} of each list entry, rec0 for the records and n_next (chain_t and rec1 stay unused).  The maps,
// 96 bytes per sample of a chunk, are aliased to nothing: they live in `maps` (room for map_rays samples, at least aov_spp: a sequence's,
// allocated at its creation) or, with maps null, in a buffer of the call's own, freed after the stream has drained; either way outside the
// workspace, so no array of aov_in_workspace -- wave 0 / 1 ray_o, ray_d, hit, rec0, rec1, vtx0, vtx1, vtx2, vtx_j -- can overlap them.
// A chunk holds at most motion_map_rays(..) rays so that the storage stays below 96 MiB whatever the frame.
int mcpt::motion_pass(mcpt_scene *sc, const CameraConst &cc, const CameraConst &prev_cc, uint32_t seed, int32_t aov_spp, int32_t spec_depth, bool centre,
                      float4 *maps, uint64_t map_rays, float *motion_dev, hipStream_t st) {
    const tp::Cam cur = motion_camera(cc), prev = motion_camera(prev_cc);
    const TriGeom *prev_tri = sc->has_snapshot ? sc->snap_tri.p : sc->view.tri_geom;
    const SphereRec *prev_sph = sc->has_snapshot ? sc->snap_sph.p : sc->view.spheres;
    if (spec_depth == 0)
        return first_hit_chunks(sc, cc, seed, aov_spp, centre, false, 0, st, [&](const AovPtrs &a, uint32_t p0, uint32_t np, uint32_t n) -> int {
            launch_motion_resolve(sc->view, prev_tri, prev_sph, cur, prev, n, a.list_o[0], a.list_d[0], a.list_hit[0], a.rec0, st);
            launch_motion_fold(p0, np, aov_spp, a.rec0, motion_dev, st);
            return MCPT_OK;
        });
    DevBuf<float4> own;
    if (!maps) {
        map_rays = motion_map_rays((uint64_t)cc.width * cc.height, aov_spp);
        HIP_TRY(own.alloc(map_rays * 6));
        maps = own.p;
    }
    if (map_rays < (uint64_t)aov_spp) return fail(MCPT_ERR_ARG, "motion pass: the map storage holds less than one pixel's samples");
    const int rc = first_hit_chunks(sc, cc, seed, aov_spp, centre, true, map_rays, st, [&](const AovPtrs &a, uint32_t p0, uint32_t np, uint32_t n) -> int {
        const int cr = chain_bounces(sc->view, a, n, spec_depth, st, [&](int b, int lc, uint32_t m) {
            launch_motion_chain(sc->view, prev_tri, prev_sph, cur, prev, m, b, spec_depth, a.list_o[lc], a.list_d[lc], a.list_hit[lc],
                                b == 0 ? nullptr : a.chain_st[lc], a.rec0, maps, (size_t)map_rays, a.list_o[lc ^ 1], a.list_d[lc ^ 1], a.chain_st[lc ^ 1],
                                a.n_next, st);
        });
        if (cr != MCPT_OK) return cr;
        launch_motion_fold(p0, np, aov_spp, a.rec0, motion_dev, st);
        return MCPT_OK;
    });
    if (rc != MCPT_OK) return rc;
    if (own.p) HIP_TRY(hipStreamSynchronize(st));  // (the call's own maps are freed on return)
    return MCPT_OK;
}

namespace {

// mcpt_render_aovs, mcpt_render_aovs_ex and mcpt_render_aovs_features (`name` for the messages; features null: every switch off)
int render_aovs(const char *name, mcpt_scene *sc, const mcpt_camera *cam, uint32_t seed, int32_t aov_spp, int32_t spec_depth, const mcpt_feature_opts *features,
                float *aov_host) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    if (!sc || !cam || !aov_host) return bad("null argument");
    bool centre = false;
    if (const int rc = check_features(name, features, aov_spp, centre)) return rc;
    if (!frame_ok(cam->width, cam->height)) return bad("width and height must be positive (and the frame not too large)");
    if (aov_spp < 0 || aov_spp > kMaxAovSpp) return bad("aov_spp must be 0..65536");
    if (spec_depth < 0 || spec_depth > dn::kMaxSpecularDepth) return bad("specular_depth must be 0..8");
    const int32_t n_spp = centre ? 1 : aov_spp == 0 ? 4 : aov_spp;
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)cam->width * cam->height;
    DevBuf<float> aov;
    HIP_TRY(aov.alloc(n_px * 8));
    const int rc = aov_pass(sc, make_camera(*cam), seed, n_spp, spec_depth, centre, aov.p, nullptr);
    if (rc != MCPT_OK) return drained(rc);
    HIP_TRY(download(aov_host, aov, n_px * 8));
    return MCPT_OK;
}

// mcpt_render_motion, mcpt_render_motion_ex and mcpt_render_motion_features (`name` for the messages; features null: every switch off)
int render_motion(const char *name, mcpt_scene *sc, const mcpt_camera *cam, const mcpt_camera *prev_cam, uint32_t seed, int32_t aov_spp, int32_t spec_depth,
                  const mcpt_feature_opts *features, float *motion_host) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    if (!sc || !cam || !prev_cam || !motion_host) return bad("null argument");
    bool centre = false;
    if (const int rc = check_features(name, features, aov_spp, centre)) return rc;
    if (!frame_ok(cam->width, cam->height)) return bad("width and height must be positive (and the frame not too large)");
    if (prev_cam->width != cam->width || prev_cam->height != cam->height) return bad("prev_camera must have the width and height of camera");
    if (aov_spp < 0 || aov_spp > kMaxAovSpp) return bad("aov_spp must be 0..65536");
    if (spec_depth < 0 || spec_depth > tp::kMaxSpecularMotionDepth) return bad("specular_depth must be 0..8");
    const int32_t n_spp = centre ? 1 : aov_spp == 0 ? 4 : aov_spp;
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)cam->width * cam->height;
    DevBuf<float> motion;
    HIP_TRY(motion.alloc(n_px * 4));
    const CameraConst cc = make_camera(*cam);
    const int rc = motion_pass(sc, cc, make_camera(*prev_cam), seed, n_spp, spec_depth, centre, nullptr, 0, motion.p, nullptr);
    if (rc != MCPT_OK) return drained(rc);
    HIP_TRY(download(motion_host, motion, n_px * 4));
    return MCPT_OK;
}

}  // namespace

int mcpt::check_adaptive(const char *name, const mcpt_adaptive &o, const mcpt_params &p) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    if (o.min_spp < 2) return bad("min_spp must be at least 2");
    int R = 0;
    while (R <= 15 && ((int64_t)o.min_spp << R) < p.spp) ++R;
    if (R > 15 || ((int64_t)o.min_spp << R) != p.spp) return bad("params.spp must be min_spp * 2^R, 0 <= R <= 15");
    if (!(o.threshold >= 0.f) || !std::isfinite(o.threshold)) return bad("threshold must be finite and >= 0");
    if (!(o.rel_floor > 0.f)) return bad("rel_floor must be > 0");
    if (o.dilate != 0 && o.dilate != 1) return bad("dilate must be 0 or 1");
    return MCPT_OK;
}

int mcpt::adaptive_rounds(FrameCall &f, const mcpt_adaptive &o, AdaptiveBufs &b, AdaptiveLists *own, hipStream_t st, AdaptiveResult &res) {
    mcpt_scene *sc = f.sc;
    const mcpt_params &p = f.p;
    const int W = f.cc.width, H = f.cc.height;
    const size_t n_px = (size_t)W * H;
    const int32_t S0 = o.min_spp;
    const double rel_floor = (double)o.rel_floor, threshold = (double)o.threshold;
    int rc;
    HIP_TRY(hipMemsetAsync(b.err, 0, n_px * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(b.mom, 0, n_px * 6 * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(b.spp, 0, n_px * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(b.stamp, 0, n_px, st));
    if ((rc = f.pixels(S0, (float)S0, b.fb, st)) != MCPT_OK) return rc;  // round 0 of the culled pixels: S0 additions of background / S0
    const PixelSet &ps = f.ps;
    mcpt_adaptive_info &inf = res.info;
    std::memset(&inf, 0, sizeof inf);
    Totals &all = res.totals;
    uint64_t &samples = res.samples, &traced_primary = res.traced_primary;
    samples = traced_primary = 0;
    if (ps.n_owned > 0) {
        // the culled pixels are final at S0: their estimate from the constant samples, no mark (they take no part in dilation)
        const uint32_t n_sky = ps.n_owned - ps.n_pix;
        if (n_sky > 0) {
            launch_sky_moments(ps.sky, n_sky, sc->view.background, S0, b.mom, st);
            launch_adapt_eval(ps.sky, n_sky, b.mom, S0, rel_floor, threshold, nullptr, 0.f, 0u, b.err, nullptr, b.spp, st);
        }
        // the active pixels of the current and of the next round (with their candidate entries when the cull produced them)
        uint32_t n_act = ps.n_pix;
        if (own) {
            HIP_TRY(own->alloc(n_act, ps.cand != nullptr));
            own->into(b);
        }
        if (n_act > 0) {
            HIP_TRY(hipMemcpyAsync(b.list[0], ps.list, n_act * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            if (ps.cand) HIP_TRY(hipMemcpyAsync(b.cand[0], ps.cand, n_act * sizeof(int4), hipMemcpyDeviceToDevice, st));
        }
        samples = (uint64_t)ps.n_owned * S0;
        int cur = 0;
        for (int r = 0;; ++r) {
            const auto tr = r == 0 ? f.t0 : Clock::now();
            const int32_t n = S0 << r;                   // samples per active pixel after this round
            const int32_t first = r == 0 ? 0 : n / 2;    // this round renders samples [first, n), divisor n
            const bool can_double = 2 * (int64_t)n <= p.spp;
            uint32_t n_next = 0;
            if (n_act > 0) {
                rc = render_list(sc, f.cc, p, b.list[cur], ps.cand ? b.cand[cur] : nullptr, n_act, first, n - first, (float)n, b.fb, b.mom, st, tr, all);
                if (rc != MCPT_OK) return rc;
                traced_primary += (uint64_t)n_act * (n - first);
                if (r > 0) samples += (uint64_t)n_act * (n - first);
                const uint32_t round_stamp = (uint32_t)r + 1u;
                launch_adapt_eval(b.list[cur], n_act, b.mom, n, rel_floor, threshold, b.guide, b.guide_max_history, round_stamp, b.err, b.stamp, b.spp, st);
                launch_adapt_select(b.list[cur], n_act, W, H, b.stamp, round_stamp, o.dilate, can_double ? 1 : 0, n, b.fb, b.spp, b.flags, st);
                if (can_double)
                    HIP_TRY(adapt_compact(b.list[cur], ps.cand ? b.cand[cur] : nullptr, b.flags, n_act, b.list[cur ^ 1], ps.cand ? b.cand[cur ^ 1] : nullptr,
                                          b.temp, b.temp_bytes, b.count, &n_next, st));
                else
                    HIP_TRY(hipStreamSynchronize(st));
            }
            inf.active_pixels[r] = r == 0 ? ps.n_owned : n_act;
            inf.ms_round[r] = ms_since(tr);
            inf.rounds = r + 1;
            if (n_next == 0) break;
            n_act = n_next;
            cur ^= 1;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MCPT_OK;
}

int mcpt::render_moments(FrameCall &f, float *fb, double *mom, float *var, hipStream_t st, AdaptiveResult &res) {
    const mcpt_params &p = f.p;
    const size_t n_px = (size_t)f.cc.width * f.cc.height;
    int rc;
    if (mom) HIP_TRY(hipMemsetAsync(mom, 0, n_px * 6 * sizeof(double), st));
    if ((rc = f.pixels(p.spp, (float)p.spp, fb, st)) != MCPT_OK) return rc;
    const PixelSet &ps = f.ps;
    if (mom && ps.n_owned > ps.n_pix) launch_sky_moments(ps.sky, ps.n_owned - ps.n_pix, f.sc->view.background, p.spp, mom, st);
    if (ps.n_pix > 0) {
        rc = render_list(f.sc, f.cc, p, ps.list, ps.cand, ps.n_pix, 0, p.spp, (float)p.spp, fb, mom, st, f.t0, res.totals);
        if (rc != MCPT_OK) return rc;
    }
    if (mom) launch_dn_variance((uint32_t)n_px, mom, p.spp, var, st);
    res.samples = (uint64_t)ps.n_owned * p.spp;
    res.traced_primary = (uint64_t)ps.n_pix * p.spp;
    return MCPT_OK;
}

namespace {

// The per-pixel buffers of an adaptive frame that owns them (mcpt_render_adaptive[_guided | _denoised]).
struct AdaptiveFrame {
    DevBuf<float> fb, err, var;
    DevBuf<double> mom;
    DevBuf<int32_t> sppm;
    DevBuf<uint8_t> stamp;
    hipError_t alloc(size_t n_px, bool with_var) {
        hipError_t e = fb.alloc(n_px * 3);
        if (e == hipSuccess) e = err.alloc(n_px);
        if (e == hipSuccess) e = mom.alloc(n_px * 6);
        if (e == hipSuccess) e = sppm.alloc(n_px);
        if (e == hipSuccess) e = stamp.alloc(n_px);
        if (e == hipSuccess && with_var) e = var.alloc(n_px);
        return e;
    }
    AdaptiveBufs bufs(const float *guide, float guide_max_history = 0.f) const {
        AdaptiveBufs b;
        b.fb = fb.p;
        b.mom = mom.p;
        b.spp = sppm.p;
        b.err = err.p;
        b.stamp = stamp.p;
        b.guide = guide;
        b.guide_max_history = guide_max_history;
        return b;
    }
};

// What mcpt_render_denoised and mcpt_render_adaptive_denoised share: the buffers besides the frame's own, allocated before the render,
// and everything after it.
struct DenoisedTail {
    DevBuf<float> aov, out;
    DenoiseBufs db;
    Event render_begin, render_end, aov_end, filter_end;  // around the three stages: render (or rounds), AOV pass, filter
    int alloc(size_t n_px) {
        HIP_TRY(aov.alloc(n_px * 8));
        HIP_TRY(out.alloc(n_px * 3));
        HIP_TRY(db.alloc(n_px));
        for (Event *e : {&render_begin, &render_end, &aov_end, &filter_end}) HIP_TRY(e->create(true));
        return MCPT_OK;
    }
    // The render stage ends here, with the frame in fb and its variance in var: the AOV pass, the filter, the downloads, the stage times.
    int finish(FrameCall &f, const mcpt_denoise_opts &opts, const dn::Opts &o, int32_t aov_spp, const DevBuf<float> &fb, const DevBuf<float> &var,
               hipStream_t st, float *fb_host, float *denoised_host, float *variance_host, float *aov_host, mcpt_denoise_info *info) {
        const int W = f.cc.width, H = f.cc.height;
        const size_t n_px = (size_t)W * H;
        HIP_TRY(hipEventRecord(render_end, st));
        const int rc = aov_pass(f.sc, f.cc, f.p.seed, aov_spp, opts.specular_depth, false, aov.p, st);
        if (rc != MCPT_OK) return drained(rc);
        HIP_TRY(hipEventRecord(aov_end, st));
        launch_denoise(W, H, o, fb.p, var.p, aov.p, db.rec[0].p, db.rec[1].p, db.grad.p, out.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(filter_end, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(download(fb_host, fb, n_px * 3));
        HIP_TRY(download(denoised_host, out, n_px * 3));
        if (variance_host) HIP_TRY(download(variance_host, var, n_px));
        if (aov_host) HIP_TRY(download(aov_host, aov, n_px * 8));
        if (info) {
            float render = 0.f, aovs = 0.f, filter = 0.f;
            HIP_TRY(hipEventElapsedTime(&render, render_begin, render_end));
            HIP_TRY(hipEventElapsedTime(&aovs, render_end, aov_end));
            HIP_TRY(hipEventElapsedTime(&filter, aov_end, filter_end));
            *info = {render, aovs, filter, ms_since(f.t0)};
        }
        return MCPT_OK;
    }
};

// mcpt_render_adaptive, mcpt_render_adaptive_guided and mcpt_render_adaptive_weighted (`name` for the messages; guide_host and variance_host
// null for the first; weight_max_history > 0 for the last: the guide holds history weights)
int render_adaptive_guided(const char *name, mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_adaptive *opts,
                           const float *guide_host, float weight_max_history, float *fb_host, int32_t *spp_host, float *err_host, float *variance_host, mcpt_adaptive_info *info,
                           mcpt_stats *stats) {
    if (!sc || !cam || !pp || !opts || !fb_host) return fail(MCPT_ERR_ARG, std::string(name) + ": null argument");
    const mcpt_params &p = *pp;
    int rc = check_frame_call(name, *cam, p, kOneCallFrame);
    if (rc != MCPT_OK) return rc;
    if ((rc = check_adaptive(name, *opts, p)) != MCPT_OK) return rc;
    FrameCall f{sc, p};
    if ((rc = f.begin(*cam)) != MCPT_OK) return rc;
    const hipStream_t st = nullptr;
    const size_t n_px = (size_t)cam->width * cam->height;
    AdaptiveFrame af;
    DevBuf<float> guide;
    HIP_TRY(af.alloc(n_px, variance_host != nullptr));
    if (guide_host) HIP_TRY(upload(guide, guide_host, n_px));
    AdaptiveBufs b = af.bufs(guide_host ? guide.p : nullptr, weight_max_history);
    AdaptiveLists lists;
    AdaptiveResult res;
    if ((rc = adaptive_rounds(f, *opts, b, &lists, st, res)) != MCPT_OK) return rc;
    if (variance_host) {
        launch_dn_variance_map((uint32_t)n_px, af.mom.p, af.sppm.p, af.var.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(download(fb_host, af.fb, n_px * 3));
    if (spp_host) HIP_TRY(download(spp_host, af.sppm, n_px));
    if (err_host) HIP_TRY(download(err_host, af.err, n_px));
    if (variance_host) HIP_TRY(download(variance_host, af.var, n_px));
    if (info) *info = res.info;
    return f.end(stats, res.samples, res.traced_primary, res.totals);
}

// mcpt_denoise and mcpt_denoise_feedback (`name` for the messages): the checks, the three planes staged on the device, the filter -- with the
// feedback kernel behind iteration fopts->iteration when that is not 0 -- and the results back.
int denoise_call(const char *name, mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host,
                 const float *aov_host, const mcpt_denoise_opts *opts, const mcpt_feedback_opts *fopts, float *out_host, float *fb_color_host,
                 float *fb_variance_host) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    if (!sc || !color_host || !variance_host || !aov_host || !opts || !out_host) return bad("null argument");
    if (!frame_ok(width, height)) return bad("width and height must be positive (and the frame not too large)");
    dn::Opts o;
    if (dn::resolve_opts(*opts, o) != 0) return bad("option out of range");
    int k = 0;
    if (dn::resolve_feedback(fopts, o, k) != 0) return bad("feedback: iteration must be 0 or 1..iterations, reserved words 0");
    if (k > 0 && !fb_color_host) return bad("feedback: null feedback_color_host");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)width * height;
    DevBuf<float> col, var, aov, out, fcol, fvar;
    HIP_TRY(col.alloc(n_px * 3));
    HIP_TRY(var.alloc(n_px));
    HIP_TRY(aov.alloc(n_px * 8));
    HIP_TRY(out.alloc(n_px * 3));
    if (k > 0) HIP_TRY(fcol.alloc(n_px * 3));
    if (k > 0 && fb_variance_host) HIP_TRY(fvar.alloc(n_px));
    HIP_TRY(upload(col, color_host, n_px * 3));
    HIP_TRY(upload(var, variance_host, n_px));
    HIP_TRY(upload(aov, aov_host, n_px * 8));
    DenoiseBufs db;
    HIP_TRY(db.alloc(n_px));
    launch_denoise_feedback(width, height, o, col.p, var.p, aov.p, db.rec[0].p, db.rec[1].p, db.grad.p, out.p, k, fcol.p, fvar.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(download(out_host, out, n_px * 3));
    if (k > 0) HIP_TRY(download(fb_color_host, fcol, n_px * 3));
    if (k > 0 && fb_variance_host) HIP_TRY(download(fb_variance_host, fvar, n_px));
    return MCPT_OK;
}

}  // namespace

extern "C" {

int mcpt_render_device(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *p, float *fb_device, void *hip_stream,
                       mcpt_stats *stats) {
    return render_impl(sc, cam, p, fb_device, (hipStream_t)hip_stream, stats);
}

int mcpt_render(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *p, float *fb_host, mcpt_stats *stats) {
    if (!sc || !cam || !p || !fb_host) return fail(MCPT_ERR_ARG, "mcpt_render: null argument");
    HIP_TRY(hipSetDevice(sc->device));
    const size_t n = (size_t)cam->width * cam->height * 3;
    DevBuf<float> fb;
    HIP_TRY(fb.alloc(n));
    if (p->accumulate) HIP_TRY(upload(fb, fb_host, n));
    const int rc = render_impl(sc, cam, p, fb.p, nullptr, stats);
    if (rc == MCPT_OK || rc == MCPT_ERR_OVERFLOW) {
        const hipError_t e = download(fb_host, fb, n);
        if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("framebuffer download: ") + hipGetErrorString(e));
    }
    return rc;
}

int mcpt_render_adaptive(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_adaptive *opts, float *fb_host, int32_t *spp_host,
                         float *err_host, mcpt_adaptive_info *info, mcpt_stats *stats) {
    return render_adaptive_guided("mcpt_render_adaptive", sc, cam, pp, opts, nullptr, 0.f, fb_host, spp_host, err_host, nullptr, info, stats);
}

int mcpt_render_adaptive_guided(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_adaptive *rule, const float *guide_host,
                                float *fb_host, int32_t *spp_host, float *err_host, float *variance_host, mcpt_adaptive_info *info, mcpt_stats *stats) {
    return render_adaptive_guided("mcpt_render_adaptive_guided", sc, cam, pp, rule, guide_host, 0.f, fb_host, spp_host, err_host, variance_host, info, stats);
}

int mcpt_render_adaptive_weighted(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_adaptive *rule, const float *history_weight_host,
                                  int32_t max_history, float *fb_host, int32_t *spp_host, float *err_host, float *variance_host, mcpt_adaptive_info *info,
                                  mcpt_stats *stats) {
    const char *name = "mcpt_render_adaptive_weighted";
    mcpt_temporal_opts to{};
    to.max_history = max_history;
    tp::Opts o;
    if (tp::resolve_opts(to, o) != 0) return fail(MCPT_ERR_ARG, std::string(name) + ": max_history out of range");
    return render_adaptive_guided(name, sc, cam, pp, rule, history_weight_host, o.max_history, fb_host, spp_host, err_host, variance_host, info, stats);
}

int mcpt_render_adaptive_denoised(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_adaptive *rule, const float *guide_host,
                                  const mcpt_denoise_opts *opts, float *fb_host, float *denoised_host, int32_t *spp_host, float *err_host,
                                  float *variance_host, float *aov_host, mcpt_adaptive_info *ainfo, mcpt_denoise_info *info, mcpt_stats *stats) {
    const char *name = "mcpt_render_adaptive_denoised";
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    if (!sc || !cam || !pp || !rule || !opts || !fb_host || !denoised_host) return bad("null argument");
    const mcpt_params &p = *pp;
    int rc = check_frame_call(name, *cam, p, kDenoisedFrame | kOneRank | kOneCallFrame);
    if (rc != MCPT_OK) return rc;
    if ((rc = check_adaptive(name, *rule, p)) != MCPT_OK) return rc;
    dn::Opts o;
    if (dn::resolve_opts(*opts, o) != 0) return bad("option out of range");
    // every pixel has at least min_spp samples, and feature sample k is render sample k
    if (opts->aov_spp > rule->min_spp || opts->aov_spp > kMaxAovSpp) return bad("aov_spp must be at most min_spp and 65536");
    const int32_t aov_spp = opts->aov_spp == 0 ? std::min(4, rule->min_spp) : opts->aov_spp;
    FrameCall f{sc, p};
    if ((rc = f.begin(*cam)) != MCPT_OK) return rc;
    const hipStream_t st = nullptr;
    const size_t n_px = (size_t)cam->width * cam->height;
    AdaptiveFrame af;
    DevBuf<float> guide;
    DenoisedTail tail;
    HIP_TRY(af.alloc(n_px, true));
    if (guide_host) HIP_TRY(upload(guide, guide_host, n_px));
    if ((rc = tail.alloc(n_px)) != MCPT_OK) return rc;
    HIP_TRY(hipEventRecord(tail.render_begin, st));
    AdaptiveBufs b = af.bufs(guide_host ? guide.p : nullptr);
    AdaptiveLists lists;
    AdaptiveResult res;
    if ((rc = adaptive_rounds(f, *rule, b, &lists, st, res)) != MCPT_OK) return rc;
    launch_dn_variance_map((uint32_t)n_px, af.mom.p, af.sppm.p, af.var.p, st);
    if ((rc = tail.finish(f, *opts, o, aov_spp, af.fb, af.var, st, fb_host, denoised_host, variance_host, aov_host, info)) != MCPT_OK) return rc;
    if (spp_host) HIP_TRY(download(spp_host, af.sppm, n_px));
    if (err_host) HIP_TRY(download(err_host, af.err, n_px));
    if (ainfo) *ainfo = res.info;
    return f.end(stats, res.samples, res.traced_primary, res.totals);
}

int mcpt_render_aovs(mcpt_scene *sc, const mcpt_camera *cam, uint32_t seed, int32_t aov_spp, float *aov_host) {
    return render_aovs("mcpt_render_aovs", sc, cam, seed, aov_spp, 0, nullptr, aov_host);
}

int mcpt_render_aovs_ex(mcpt_scene *sc, const mcpt_camera *cam, uint32_t seed, int32_t aov_spp, int32_t specular_depth, float *aov_host) {
    return render_aovs("mcpt_render_aovs_ex", sc, cam, seed, aov_spp, specular_depth, nullptr, aov_host);
}

int mcpt_render_aovs_features(mcpt_scene *sc, const mcpt_camera *cam, uint32_t seed, int32_t aov_spp, int32_t specular_depth,
                              const mcpt_feature_opts *features, float *aov_host) {
    return render_aovs("mcpt_render_aovs_features", sc, cam, seed, aov_spp, specular_depth, features, aov_host);
}

int mcpt_denoise(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *aov_host,
                 const mcpt_denoise_opts *opts, float *out_host) {
    return denoise_call("mcpt_denoise", sc, width, height, color_host, variance_host, aov_host, opts, nullptr, out_host, nullptr, nullptr);
}

int mcpt_denoise_feedback(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *aov_host,
                          const mcpt_denoise_opts *opts, const mcpt_feedback_opts *feedback, float *out_host, float *feedback_color_host,
                          float *feedback_variance_host) {
    return denoise_call("mcpt_denoise_feedback", sc, width, height, color_host, variance_host, aov_host, opts, feedback, out_host, feedback_color_host,
                        feedback_variance_host);
}

int mcpt_render_denoised(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_denoise_opts *opts, float *fb_host,
                         float *denoised_host, float *variance_host, float *aov_host, mcpt_denoise_info *info, mcpt_stats *stats) {
    if (!sc || !cam || !pp || !opts || !fb_host || !denoised_host) return fail(MCPT_ERR_ARG, "mcpt_render_denoised: null argument");
    const mcpt_params &p = *pp;
    int rc = check_frame_call("mcpt_render_denoised", *cam, p, kDenoisedFrame | kOneRank | kOneCallFrame);
    if (rc != MCPT_OK) return rc;
    dn::Opts o;
    if (dn::resolve_opts(*opts, o) != 0) return fail(MCPT_ERR_ARG, "mcpt_render_denoised: option out of range");
    if (opts->aov_spp > p.spp || opts->aov_spp > kMaxAovSpp) return fail(MCPT_ERR_ARG, "mcpt_render_denoised: aov_spp must be at most params.spp and 65536");
    const int32_t aov_spp = opts->aov_spp == 0 ? std::min(4, p.spp) : opts->aov_spp;
    FrameCall f{sc, p};
    if ((rc = f.begin(*cam)) != MCPT_OK) return rc;
    const hipStream_t st = nullptr;
    const size_t n_px = (size_t)cam->width * cam->height;
    DevBuf<float> fb, var;
    DevBuf<double> mom;
    DenoisedTail tail;
    HIP_TRY(fb.alloc(n_px * 3));
    HIP_TRY(var.alloc(n_px));
    HIP_TRY(mom.alloc(n_px * 6));
    if ((rc = tail.alloc(n_px)) != MCPT_OK) return rc;
    HIP_TRY(hipEventRecord(tail.render_begin, st));
    AdaptiveResult res;
    if ((rc = render_moments(f, fb.p, mom.p, var.p, st, res)) != MCPT_OK) return rc;
    if ((rc = tail.finish(f, *opts, o, aov_spp, fb, var, st, fb_host, denoised_host, variance_host, aov_host, info)) != MCPT_OK) return rc;
    return f.end(stats, res.samples, res.traced_primary, res.totals);
}

int mcpt_render_motion(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_camera *prev_cam, uint32_t seed, int32_t aov_spp, float *motion_host) {
    return render_motion("mcpt_render_motion", sc, cam, prev_cam, seed, aov_spp, 0, nullptr, motion_host);
}

int mcpt_render_motion_ex(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_camera *prev_cam, uint32_t seed, int32_t aov_spp, int32_t specular_depth,
                          float *motion_host) {
    return render_motion("mcpt_render_motion_ex", sc, cam, prev_cam, seed, aov_spp, specular_depth, nullptr, motion_host);
}

int mcpt_render_motion_features(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_camera *prev_cam, uint32_t seed, int32_t aov_spp, int32_t specular_depth,
                                const mcpt_feature_opts *features, float *motion_host) {
    return render_motion("mcpt_render_motion_features", sc, cam, prev_cam, seed, aov_spp, specular_depth, features, motion_host);
}

}  // extern "C"
