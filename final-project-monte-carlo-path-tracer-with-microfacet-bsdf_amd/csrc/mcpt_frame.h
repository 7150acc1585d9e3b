// What the frame-level translation units share (mcpt_render.hip defines it; mcpt_sequence.hip runs the same passes on buffers of its
// own): the checks of (camera, params), the start and the end of a call, the AOV pass and the motion pass, the filter's working buffers.
#pragma once
#include "mcpt_host.h"
#include "mcpt_adaptive.h"
#include "mcpt_denoise.h"
#include "mcpt_direct.h"
#include "mcpt_sh.h"
#include "mcpt_temporal.h"

namespace mcpt {

constexpr int32_t kMaxAovSpp = 65536;

// a frame whose AOV records (8 floats per pixel) can be indexed
inline bool frame_ok(int W, int H) { return W > 0 && H > 0 && (uint64_t)W * H <= 0x7fffffffull / 8; }

// What an entry point forbids on top of the common checks of (cam, params).
enum : unsigned {
    kOneCallFrame = 1u,  // no progressive accumulation: accumulate, spp_total and sample_offset must be 0
    kOneRank = 2u,       // nranks must be 1
    kDenoisedFrame = 4u,  // spp >= 2 (a variance needs two samples) and a frame the AOV pass can hold (frame_ok)
    kOneSample = 8u       // with kDenoisedFrame: spp >= 1 (a moments sequence takes its variance from the frames, csrc/mcpt_moments.h)
};

// The checks of (cam, params) every frame-level call makes before it touches the scene, in the order the entry points have always made
// them; `name` is the entry point's, for the message.
int check_frame_call(const char *name, const mcpt_camera &cam, const mcpt_params &p, unsigned forbid);

// mcpt_stats of a call that rendered `samples` camera samples, `traced_primary` of them through the wavefront loop (the rest: sky cull).
void fill_stats(mcpt_stats *stats, uint64_t samples, uint64_t traced_primary, int32_t n_dir, const Totals &rt, Clock::time_point t0);

// The start and the end every frame-level render call shares, once its arguments have passed the checks.
struct FrameCall {
    mcpt_scene *sc;
    const mcpt_params &p;
    Clock::time_point t0;
    CameraConst cc;
    PixelSet ps;
    int begin(const mcpt_camera &cam) {
        HIP_TRY(hipSetDevice(sc->device));
        (void)hipGetLastError();  // an earlier, already reported failure of this thread must not be taken for one of this call
        t0 = Clock::now();
        cc = make_camera(cam);
        return MCPT_OK;
    }
    // the owned pixels, the cleared frame and the sky cull, whose pixels get `spp` additions of background / spp_total
    int pixels(int32_t spp, float spp_total, float *fb_dev, hipStream_t st) { return prepare_pixels(sc, cc, p, spp, spp_total, fb_dev, st, ps); }
    int end(mcpt_stats *stats, uint64_t samples, uint64_t traced_primary, const Totals &rt) const {
        if (stats) fill_stats(stats, samples, traced_primary, p.n_dir_sample, rt, t0);
        sc->last_cont_traced = rt.cont_traced;  // (mcpt_scene_ray_counts)
        sc->last_cont_shared = rt.cont_shared;
        sc->last_pc_samples = rt.pc_samples;  // (mcpt_scene_primary_conductor_counts)
        sc->last_pc_rays = rt.pc_rays;
        if (rt.overflow) return fail(MCPT_ERR_OVERFLOW, "some paths outran the clamp stack (raise params.max_depth)");
        return MCPT_OK;
    }
};

// The AOV pass (include/mcpt.h): aov_dev[8m ..] for every pixel of the frame, queued on `st` (with spec_depth > 0 it waits for the
// stream once per bounce).
// centre (mcpt_feature_opts, for both passes): one feature ray per pixel, its centre ray; aov_spp must then be 1 and seed is ignored.
int aov_pass(mcpt_scene *sc, const CameraConst &cc, uint32_t seed, int32_t aov_spp, int32_t spec_depth, bool centre, float *aov_dev, hipStream_t st);
// The checks of a mcpt_feature_opts (nullable: every switch off) beside the aov_spp it is used with: MCPT_ERR_ARG in `name`'s name for a
// centre that is not 0 or 1, a non-zero reserved word, or centre 1 with aov_spp > 1; otherwise `centre` is set.
int check_features(const char *name, const mcpt_feature_opts *features, int32_t aov_spp, bool &centre);
// The motion pass (include/mcpt.h: mcpt_render_motion[_ex]): motion_dev[4m ..] for every pixel of the frame, against the scene's snapshot.
// spec_depth > 0: through the specular chains of aov_pass(.., spec_depth, ..) (it then waits for the stream once per bounce); their maps go
// into `maps`, six planes of map_rays float4 with map_rays >= motion_map_rays(pixels, aov_spp), or with maps null into a buffer of the call's.
int motion_pass(mcpt_scene *sc, const CameraConst &cc, const CameraConst &prev_cc, uint32_t seed, int32_t aov_spp, int32_t spec_depth, bool centre,
                float4 *maps, uint64_t map_rays, float *motion_dev, hipStream_t st);
uint64_t motion_map_rays(uint64_t n_px, int32_t aov_spp);

// The probe volume a lit pass shades from: the grid and device arrays of mcpt_probe_volume after their checks.  moments null: the plain
// lookup (sh::probe_shade), counts and the two options are then not read.
struct LitVolume {
    sh::Grid g;
    const float *sh = nullptr, *moments = nullptr;
    const int32_t *counts = nullptr;
    float normal_bias = 0.f, backface_max = 0.f;
};
// The lit pass (include/mcpt.h: mcpt_render_probe_lit): lit_dev[3m ..] and, when not null, position_dev[3m ..] for every pixel of the frame,
// queued on `st` (with spec_depth > 0 it waits for the stream once per bounce).  The chunk loop and the bounce loop of aov_pass (first_hit_chunks, chain_bounces) with
// k_lit_terminal in k_aov_chain's place, then k_lit_shade and k_lit_fold (csrc/mcpt_probes.hip).  Besides the arrays of the AOV pass a
// chunk keeps p per sample: in the workspace's shadow queue origins (shq_o, which no feature pass touches) when they hold a chunk, else in
// a buffer of the call's own.  lookups_dev: one device counter, cleared here, that ends as info.lookups.  Returns with the stream drained.
// direct (mcpt_render_probe_lit_direct; null: off): n_samples >= 1 light samples per surface sample through direct_term, staged after the
// chain loop in the chunk's two ray lists, which are free by then -- shadow rays and hits in list 0, the sample records in list 1's
// origins, D per sample in the chain states of list 0, the piece's ray count in n_next -- so the chunk loop then always runs with the
// chain arrays.  lookups_dev then holds a second counter, the live light samples, which ends as dinfo.shadow_rays.
struct LitDirect {
    int32_t n_samples;
    uint32_t seed;
};
int lit_pass(mcpt_scene *sc, const CameraConst &cc, uint32_t seed, int32_t aov_spp, int32_t spec_depth, bool centre, const LitVolume &vol, float *lit_dev,
             float *position_dev, unsigned long long *lookups_dev, hipStream_t st, mcpt_lit_info &info, const LitDirect *direct = nullptr,
             mcpt_lit_direct_info *dinfo = nullptr);
// csrc/mcpt_probes.hip.  One step of the lit pass's chains: launch_aov_chain's arguments (max_b == 0: every sample stops, the lists of the
// next step may be null) with the three per-sample records {a or v, kind} {nf} {p} in place of the AOV pass's two.
void launch_lit_terminal(const DevScene &S, uint32_t n, int32_t b, int32_t max_b, const float4 *ray_o, const float4 *ray_d, const uint4 *hit,
                         const float4 *chain_in, float4 *r0, float4 *r1, float4 *r2, float4 *next_o, float4 *next_d, float4 *chain_out,
                         uint32_t *n_next, hipStream_t st);
// The lookup of the n samples of a chunk: r0[j].xyz = a * max(E, 0) for the samples that ended on a surface; their number is added to *lookups.
// direct_d (nullable): D per sample in .xyz; the samples then get a * (max(E, 0) + D).
void launch_lit_shade(const LitVolume &vol, uint32_t n, float4 *r0, const float4 *r1, const float4 *r2, const float4 *direct_d, unsigned long long *lookups,
                      hipStream_t st);
constexpr uint32_t kLitSurfaceKind = 2u;  // r0[j].w of a lit sample that ended on a surface (kLitSurface, csrc/mcpt_probes.hip)
// The sampled direct term (csrc/mcpt_direct.h) of n points into out[stride * i + 0..2], staged in the pieces of stg.cut -- the caller's
// piece_cut(n, src.N, capacity, 1), whose staged() light samples every array here holds -- through arrays the caller owns: per piece
// k_direct_rays (csrc/mcpt_kernels.hip), launch_trace_closest over the compacted shadow rays and k_direct_fold.  src: where the points
// and keys come from (DirectRays, csrc/mcpt_kernels.h; the staging and piece members are set here).  pieces: the launches are added to
// it.  The result does not depend on the cut.
struct DirectStage {
    float4 *ray_o, *ray_d, *slot;
    uint4 *hit;
    uint32_t *n_rays;
    PieceCut cut;
    RetryList rl;
};
int direct_term(const DevScene &S, DirectRays src, uint64_t n, const DirectStage &stg, float *out, uint32_t stride, hipStream_t st, int32_t &pieces);
void launch_lit_fold(uint32_t p0, uint32_t n_pix, int32_t aov_spp, const float4 *r0, const float4 *r2, float *lit, float *position, hipStream_t st);

// What the rounds of an adaptive frame work in (adaptive_rounds): device buffers the caller owns.  Per pixel of the frame: fb 3 floats,
// mom 6 doubles, spp, err, stamp (1 byte), guide (nullable: the plain rule; history lengths, or with guide_max_history > 0 history weights
// and the cap of the weighted blend: mcpt_render_adaptive_weighted).  Per listed pixel: the two lists in turn with their candidate
// entries (read only when the sky cull produced some), the continue flags; the compaction's scratch and its count.
struct AdaptiveBufs {
    float *fb = nullptr;
    double *mom = nullptr;
    int32_t *spp = nullptr;
    float *err = nullptr;
    uint8_t *stamp = nullptr;
    const float *guide = nullptr;
    float guide_max_history = 0.f;
    uint32_t *list[2] = {nullptr, nullptr};
    int4 *cand[2] = {nullptr, nullptr};
    uint8_t *flags = nullptr;
    void *temp = nullptr;
    size_t temp_bytes = 0;
    uint32_t *count = nullptr;
};

// The list side of AdaptiveBufs as one owner: room for n listed pixels (at least 1), 9 bytes each and 32 more with the candidate entries,
// plus the compaction's scratch (adapt_temp_bytes(n)).
struct AdaptiveLists {
    DevBuf<uint32_t> list[2], count;
    DevBuf<int4> cand[2];
    DevBuf<uint8_t> flags, temp;
    size_t temp_bytes = 0;
    hipError_t alloc(uint32_t n, bool with_cand) {
        n = std::max<uint32_t>(n, 1u);
        temp_bytes = adapt_temp_bytes(n);
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2; ++k) {
            if (e == hipSuccess) e = list[k].alloc(n);
            if (e == hipSuccess && with_cand) e = cand[k].alloc(n);
        }
        if (e == hipSuccess) e = flags.alloc(n);
        if (e == hipSuccess) e = temp.alloc(temp_bytes);
        if (e == hipSuccess) e = count.alloc(1);
        return e;
    }
    void into(AdaptiveBufs &b) const {
        for (int k = 0; k < 2; ++k) {
            b.list[k] = list[k].p;
            b.cand[k] = cand[k].p;
        }
        b.flags = flags.p;
        b.temp = temp.p;
        b.temp_bytes = temp_bytes;
        b.count = count.p;
    }
};

// What adaptive_rounds reports besides the buffers: mcpt_adaptive_info, the kernel totals of all rounds, the samples rendered (the sum of
// the count map) and how many of them were traced (the rest: sky cull).
struct AdaptiveResult {
    mcpt_adaptive_info info{};
    Totals totals;
    uint64_t samples = 0, traced_primary = 0;
};

// The checks of an adaptive rule against params.spp (mcpt_render_adaptive), `name` for the message.
int check_adaptive(const char *name, const mcpt_adaptive &o, const mcpt_params &p);

// The rounds of an adaptive frame (include/mcpt.h: mcpt_render_adaptive, with b.guide mcpt_render_adaptive_guided / _weighted), queued on `st`, which it
// waits for once per round: clears err, moments, counts and stamps; f.pixels at S0 (the frame cleared, the sky cull); the culled pixels'
// moments and estimate; then round by round render_list, k_adapt_eval, k_adapt_select and the compaction.  own != nullptr: the list side
// of b is allocated there once the number of traced pixels is known (a call that owns its buffers); otherwise b has room for every pixel
// of the frame.  Returns with the stream drained.
int adaptive_rounds(FrameCall &f, const mcpt_adaptive &o, AdaptiveBufs &b, AdaptiveLists *own, hipStream_t st, AdaptiveResult &res);

// A uniform frame of f.p.spp samples with its moments, and the variance of its mean, on buffers the caller owns (fb 3 floats per pixel, mom 6
// doubles, var 1), queued on `st` (steps 1-2 of mcpt_render_denoised): clears the moments; f.pixels; the culled pixels' moments;
// render_list; k_dn_variance.  res gets the totals, the samples and how many were traced (res.info stays zero).  mom null: the plain frame
// of mcpt_render, without moments and without variance (var is not written).
int render_moments(FrameCall &f, float *fb, double *mom, float *var, hipStream_t st, AdaptiveResult &res);

// Working buffers of the filter: two record buffers and the depth gradient, 72 bytes per pixel.
struct DenoiseBufs {
    DevBuf<dn::Rec> rec[2];
    DevBuf<float2> grad;
    hipError_t alloc(size_t n_px) {
        hipError_t e = rec[0].alloc(n_px);
        if (e == hipSuccess) e = rec[1].alloc(n_px);
        if (e == hipSuccess) e = grad.alloc(n_px);
        return e;
    }
};

}  // namespace mcpt
