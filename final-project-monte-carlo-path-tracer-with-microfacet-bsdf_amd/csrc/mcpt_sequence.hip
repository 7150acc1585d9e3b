// Temporal reuse on host arrays and frame sequences (include/mcpt.h: mcpt_temporal_blend, mcpt_temporal_accumulate[_ex],
// mcpt_temporal_history_len, mcpt_sequence_*).  The host-array entry points stage their planes on the device and run one kernel of
// csrc/mcpt_temporal.hip.  A sequence is the frame loop of temporal reuse with its history, the variance of the accumulated frame and every
// working buffer resident on the device: a frame is the passes of csrc/mcpt_render.hip (csrc/mcpt_frame.h) on the sequence's buffers,
// k_temporal_accumulate between the two history sets (the instantiation the sequence's history rejection selects; with rejection a set
// also keeps a normal and a flags plane), the filter and the tone map, all queued on one stream; only the outputs the caller asks for are
// copied to the host.  A sequence created with a rule (mcpt_sequence_create_adaptive) renders adaptive frames: the AOVs and the motion
// first, k_history_len from the previous history set into the guide, then the rounds of csrc/mcpt_render.hip (adaptive_rounds) on the
// sequence's buffers and k_dn_variance_map.  A sequence created with specular motion (mcpt_sequence_create_motion) and a specular depth D > 0
// takes its motion through the chains (motion_pass at depth D, its maps in a buffer of the sequence's) and the history's depth and normal
// from the chain AOVs, and neither runs nor allocates the extra first-hit AOV pass.  A sequence created with weighted 1
// (mcpt_sequence_create_weighted) keeps a weight plane in each history set, accumulates with the kWeight instantiations and, adaptive and
// guided, takes its guide from k_history_weight.  A sequence created with moments (mcpt_sequence_create_moments, enabled 1) renders the plain
// frame, keeps a moments plane in each history set, accumulates with the kMoments instantiations and takes the variance of the accumulated
// frame from k_moments_variance (csrc/mcpt_moments.hip) right after; it has no moments of the render and runs at one sample per pixel.
// A sequence created with centre features (mcpt_sequence_create_features, centre 1) takes every feature pass of a frame from the centre
// rays, one per pixel.  A sequence created with feedback (mcpt_sequence_create_feedback, iteration k > 0) keeps a fed colour plane (and,
// without moments, a fed variance plane) in each history set: k_dn_feedback writes them behind iteration k of the frame's filter, and the
// next frame's accumulation reads them where it read the set's colour and variance.
#include <new>

#include "mcpt_frame.h"
#include "mcpt_moments.h"

using namespace mcpt;

namespace {

// One history set: what k_temporal_accumulate reads of the previous frame and writes for the next one.
struct History {
    DevBuf<float> color, variance, depth, len;
    DevBuf<float> normal;   // first-hit normals, 3 per pixel (history rejection with the normal test only)
    DevBuf<uint8_t> flags;  // what the rejection did to each pixel of the frame that wrote this set (either switch on)
    DevBuf<float> weight;   // the samples behind each pixel (a weighted sequence only)
    DevBuf<float> moments;  // the running luminance moments, 2 per pixel (a moments sequence only)
    DevBuf<float> fed_color, fed_variance;  // iteration k of the filter of this set's frame (a feedback sequence only; no variance with moments)
    hipError_t alloc(size_t n_px, bool with_normal, bool with_flags, bool with_weight, bool with_moments, bool with_fed) {
        hipError_t e = color.alloc(n_px * 3);
        if (e == hipSuccess) e = variance.alloc(n_px);
        if (e == hipSuccess) e = depth.alloc(n_px);
        if (e == hipSuccess) e = len.alloc(n_px);
        if (e == hipSuccess && with_normal) e = normal.alloc(n_px * 3);
        if (e == hipSuccess && with_flags) e = flags.alloc(n_px);
        if (e == hipSuccess && with_weight) e = weight.alloc(n_px);
        if (e == hipSuccess && with_moments) e = moments.alloc(n_px * 2);
        if (e == hipSuccess && with_fed) e = fed_color.alloc(n_px * 3);
        if (e == hipSuccess && with_fed && !with_moments) e = fed_variance.alloc(n_px);
        return e;
    }
    hipError_t clear(size_t n_px) {
        hipError_t e = hipMemset(color.p, 0, n_px * 3 * sizeof(float));
        if (e == hipSuccess) e = hipMemset(variance.p, 0, n_px * sizeof(float));
        if (e == hipSuccess) e = hipMemset(depth.p, 0, n_px * sizeof(float));
        if (e == hipSuccess) e = hipMemset(len.p, 0, n_px * sizeof(float));
        if (e == hipSuccess && normal.p) e = hipMemset(normal.p, 0, n_px * 3 * sizeof(float));
        if (e == hipSuccess && flags.p) e = hipMemset(flags.p, 0, n_px);
        if (e == hipSuccess && weight.p) e = hipMemset(weight.p, 0, n_px * sizeof(float));
        if (e == hipSuccess && moments.p) e = hipMemset(moments.p, 0, n_px * 2 * sizeof(float));
        if (e == hipSuccess && fed_color.p) e = hipMemset(fed_color.p, 0, n_px * 3 * sizeof(float));
        if (e == hipSuccess && fed_variance.p) e = hipMemset(fed_variance.p, 0, n_px * sizeof(float));
        return e;
    }
    // the set as the kernels take it: the previous frame's, or the one the frame writes
    // (a feedback sequence reads the fed planes where the others read colour and variance; with moments no variance is read)
    tp::Prev prev() const {
        if (fed_color.p) return {fed_color.p, fed_variance.p, depth.p, len.p, normal.p, weight.p};
        return {color.p, variance.p, depth.p, len.p, normal.p, weight.p};
    }
    tp::Next next() { return {color.p, variance.p, depth.p, len.p, normal.p, flags.p, weight.p}; }
};

// The counts of one adaptive frame and the guide it was rendered with; two sets, used in turn with the history sets, so that a failed
// frame leaves those of the last successful one.
struct Counts {
    DevBuf<int32_t> spp;
    DevBuf<float> err, guide;
    hipError_t alloc(size_t n_px) {
        hipError_t e = spp.alloc(n_px);
        if (e == hipSuccess) e = err.alloc(n_px);
        if (e == hipSuccess) e = guide.alloc(n_px);
        if (e == hipSuccess) e = hipMemset(spp.p, 0, n_px * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemset(err.p, 0, n_px * sizeof(float));
        if (e == hipSuccess) e = hipMemset(guide.p, 0, n_px * sizeof(float));
        return e;
    }
};

// The HIP events of a frame, each named for the stage boundary it marks.  A uniform frame renders first, so render_end is where its AOV
// pass begins and motion_end where its accumulation begins; an adaptive one takes its features first, from features_begin, and its
// accumulation begins at render_end.
struct StageEvents {
    Event render_begin, render_end, features_begin, aov_end, motion_end, accumulate_end, filter_end;
    hipError_t create() {
        hipError_t e = hipSuccess;
        for (Event *ev : {&render_begin, &render_end, &features_begin, &aov_end, &motion_end, &accumulate_end, &filter_end})
            if (e == hipSuccess) e = ev->create(true);
        return e;
    }
};

// The host-array entry points mcpt_temporal_blend, mcpt_temporal_accumulate[_ex | _weighted] and mcpt_temporal_history_len / _weight (`name`
// for the messages): the checks in the order they have always had, the arrays that are given staged on the device (normals packed, no
// depth plane), one kernel, the results back.  fh, ph and nh hold the host arrays; what a pass does not take is null.  hopts null: both
// switches 0.  The two weighted passes take ph.weight and nh.weight (history_weight writes nh.weight and no len), accumulate_weighted
// also fh.count (nullable) or fh.uniform_count.  accumulate_moments takes the host moments mh and no variance array.
enum class Pass { blend, accumulate, history_len, accumulate_weighted, history_weight, accumulate_moments };
int temporal_call(const char *name, Pass pass, mcpt_scene *sc, int32_t width, int32_t height, tp::Frame fh, tp::Prev ph, const mcpt_temporal_opts *opts,
                  const mcpt_history_opts *hopts, const tp::Next &nh, const tp::Moments mh = {}) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, std::string(name) + ": " + what); };
    const bool wacc = pass == Pass::accumulate_weighted, hweight = pass == Pass::history_weight, weighted = wacc || hweight;
    const bool macc = pass == Pass::accumulate_moments;
    const bool color = pass != Pass::history_len && !hweight, var = pass == Pass::accumulate || wacc;
    if (!sc || !fh.motion || !ph.color || !ph.depth || !ph.len || !opts || (!hweight && !nh.len) || (color && (!fh.color || !nh.color)) ||
        (var && (!fh.variance || !ph.variance || !hopts || !nh.variance)) || (weighted && (!ph.weight || !nh.weight)) ||
        (macc && (!hopts || !mh.prev || !mh.next)))
        return bad("null argument");
    if (!frame_ok(width, height)) return bad("width and height must be positive (and the frame not too large)");
    tp::Opts o;
    tp::HistOpts ho{};
    if (tp::resolve_opts(*opts, o) != 0) return bad("option out of range");
    if (hopts && tp::resolve_history_opts(*hopts, ho) != 0) return bad("history option out of range");
    if (ho.normal_test && (!fh.normal || !ph.normal)) return bad("normal_test needs both normal arrays");
    if (!ho.normal_test) fh.normal = ph.normal = nullptr;  // (neither read nor uploaded)
    const size_t n_px = (size_t)width * height;
    if (wacc && fh.count) {
        for (size_t m = 0; m < n_px; ++m)
            if (fh.count[m] < 1) return bad("every count must be at least 1");
    } else if (wacc && !(fh.uniform_count >= 1.0f && fh.uniform_count <= 3.0e38f)) {  // (NaN fails)
        return bad("uniform_count must be finite and at least 1");
    }
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const bool flags = nh.flags && (ho.normal_test || ho.color_clamp);  // (both switches 0: every flag is 0, and the kernel writes none)
    DevBuf<float> in[11], out, ovar, olen, oweight, omoments;
    DevBuf<int32_t> count;
    DevBuf<uint8_t> oflags;
    if (color) HIP_TRY(out.alloc(n_px * 3));
    if (var) HIP_TRY(ovar.alloc(n_px));
    if (!hweight) HIP_TRY(olen.alloc(n_px));
    if (weighted) HIP_TRY(oweight.alloc(n_px));
    if (macc) HIP_TRY(omoments.alloc(n_px * 2));
    if (wacc && fh.count) HIP_TRY(upload(count, fh.count, n_px));
    if (flags) HIP_TRY(oflags.alloc(n_px));
    hipError_t e = hipSuccess;
    int k = 0;
    const auto up = [&](const float *host, size_t per_px) -> const float * {  // a null array stays a null plane
        DevBuf<float> &d = in[k++];
        if (e == hipSuccess && host) e = upload(d, host, n_px * per_px);
        return d.p;
    };
    const tp::Frame f = {up(fh.color, 3), up(fh.variance, 1), up(fh.motion, 4), up(fh.normal, 3), 3, nullptr, 1, count.p, fh.uniform_count};
    const tp::Prev p = {up(ph.color, 3), up(ph.variance, 1), up(ph.depth, 1), up(ph.len, 1), up(ph.normal, 3), up(weighted ? ph.weight : nullptr, 1)};
    const tp::Moments mo = {up(mh.prev, 2), omoments.p};
    HIP_TRY(e);
    const tp::Next n = {out.p, ovar.p, nullptr, olen.p, nullptr, oflags.p, wacc ? oweight.p : nullptr};
    if (pass == Pass::blend) launch_temporal_blend(width, height, o, f, p, n, nullptr);
    if (macc) launch_temporal_accumulate_moments(width, height, o, ho, f, p, n, mo, nullptr);
    if (pass == Pass::accumulate || wacc) launch_temporal_accumulate(width, height, o, ho, f, p, n, nullptr);
    if (pass == Pass::history_len) launch_history_len(width, height, o, ho, f, p, olen.p, nullptr);
    if (hweight) launch_history_weight(width, height, o, ho, f, p, oweight.p, nullptr);
    HIP_TRY(hipGetLastError());
    if (color) HIP_TRY(download(nh.color, out, n_px * 3));
    if (var) HIP_TRY(download(nh.variance, ovar, n_px));
    if (!hweight) HIP_TRY(download(nh.len, olen, n_px));
    if (weighted) HIP_TRY(download(nh.weight, oweight, n_px));
    if (macc) HIP_TRY(download(mh.next, omoments, n_px * 2));
    if (flags)
        HIP_TRY(download(nh.flags, oflags, n_px));
    else if (nh.flags)
        std::memset(nh.flags, 0, n_px);
    return MCPT_OK;
}

}  // namespace

// Members are destroyed with the scene's device current (mcpt_sequence_destroy).
struct mcpt_sequence {
    mcpt_scene *sc = nullptr;  // borrowed
    int device = 0;
    int W = 0, H = 0;
    mcpt_sequence_opts opts{};
    tp::Opts temporal{};
    tp::HistOpts reject{};  // both switches 0: a sequence of mcpt_sequence_create
    dn::Opts denoise{};
    History hist[2];
    int cur = 0;        // the set that holds the history of the previous frame; a frame writes the other one
    bool fresh = true;  // no frame since create / reset: the next one takes no history
    int32_t frame_index = 0;
    CameraConst prev_cc{};
    DevBuf<float> fb, var, aov, aov_first, motion, out;
    DevBuf<double> mom;
    DevBuf<uint8_t> rgba;
    DenoiseBufs db;
    StageEvents ev;
    // a sequence created with mcpt_sequence_create_adaptive and a rule (all empty otherwise)
    bool adaptive = false;
    mcpt_adaptive rule{};
    bool guided = false;
    Counts cnt[2];  // indexed as hist
    DevBuf<uint8_t> stamp;
    AdaptiveLists lists;
    // a sequence created with mcpt_sequence_create_motion, specular_motion 1 and a specular depth > 0 (false and empty otherwise)
    bool chain_motion = false;
    DevBuf<float4> maps;  // the maps of the motion pass's chains, six planes of map_rays entries
    uint64_t map_rays = 0;
    mcpt_adaptive_info ainfo{};  // of the last successful frame
    bool weighted = false;       // a sequence created with mcpt_sequence_create_weighted and weighted 1: the history sets have a weight plane
    bool moments = false;        // a sequence created with mcpt_sequence_create_moments and enabled 1: the history sets have a moments plane,
    mo::Opts mopts{};            // there is no `mom`, and the variance of the accumulated frame is k_moments_variance's
    bool centre = false;         // a sequence created with mcpt_sequence_create_features and centre 1: the feature passes run on the centre rays
    int feedback = 0;            // a sequence created with mcpt_sequence_create_feedback and iteration k > 0: k, and the sets have fed planes
};

extern "C" {

int mcpt_temporal_blend(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *motion_host, const float *prev_color_host,
                        const float *prev_depth_host, const float *prev_len_host, const mcpt_temporal_opts *opts, float *out_color_host,
                        float *out_len_host) {
    return temporal_call("mcpt_temporal_blend", Pass::blend, sc, width, height, {color_host, nullptr, motion_host, nullptr, 3, nullptr, 1},
                         {prev_color_host, nullptr, prev_depth_host, prev_len_host, nullptr}, opts, nullptr,
                         {out_color_host, nullptr, nullptr, out_len_host, nullptr, nullptr});
}

int mcpt_temporal_accumulate(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *motion_host,
                             const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host, const float *prev_len_host,
                             const mcpt_temporal_opts *opts, float *out_color_host, float *out_variance_host, float *out_len_host) {
    const mcpt_history_opts off{};  // the _ex call with zeroed options, no normals and no flags
    return temporal_call("mcpt_temporal_accumulate", Pass::accumulate, sc, width, height, {color_host, variance_host, motion_host, nullptr, 3, nullptr, 1},
                         {prev_color_host, prev_variance_host, prev_depth_host, prev_len_host, nullptr}, opts, &off,
                         {out_color_host, out_variance_host, nullptr, out_len_host, nullptr, nullptr});
}

int mcpt_temporal_accumulate_ex(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *motion_host,
                                const float *normal_host, const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host,
                                const float *prev_len_host, const float *prev_normal_host, const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts,
                                float *out_color_host, float *out_variance_host, float *out_len_host, uint8_t *out_flags_host) {
    return temporal_call("mcpt_temporal_accumulate_ex", Pass::accumulate, sc, width, height, {color_host, variance_host, motion_host, normal_host, 3, nullptr, 1},
                         {prev_color_host, prev_variance_host, prev_depth_host, prev_len_host, prev_normal_host}, opts, hopts,
                         {out_color_host, out_variance_host, nullptr, out_len_host, nullptr, out_flags_host});
}

int mcpt_temporal_accumulate_weighted(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host,
                                      const float *motion_host, const float *normal_host, const int32_t *count_host, float uniform_count,
                                      const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host,
                                      const float *prev_len_host, const float *prev_normal_host, const float *prev_weight_host,
                                      const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *out_color_host, float *out_variance_host,
                                      float *out_len_host, uint8_t *out_flags_host, float *out_weight_host) {
    return temporal_call("mcpt_temporal_accumulate_weighted", Pass::accumulate_weighted, sc, width, height,
                         {color_host, variance_host, motion_host, normal_host, 3, nullptr, 1, count_host, uniform_count},
                         {prev_color_host, prev_variance_host, prev_depth_host, prev_len_host, prev_normal_host, prev_weight_host}, opts, hopts,
                         {out_color_host, out_variance_host, nullptr, out_len_host, nullptr, out_flags_host, out_weight_host});
}

int mcpt_temporal_accumulate_moments(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *motion_host,
                                     const float *normal_host, const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host,
                                     const float *prev_normal_host, const float *prev_moments_host, const mcpt_temporal_opts *opts,
                                     const mcpt_history_opts *hopts, float *out_color_host, float *out_len_host, uint8_t *out_flags_host,
                                     float *out_moments_host) {
    return temporal_call("mcpt_temporal_accumulate_moments", Pass::accumulate_moments, sc, width, height, {color_host, nullptr, motion_host, normal_host, 3, nullptr, 1},
                         {prev_color_host, nullptr, prev_depth_host, prev_len_host, prev_normal_host}, opts, hopts,
                         {out_color_host, nullptr, nullptr, out_len_host, nullptr, out_flags_host}, {prev_moments_host, out_moments_host});
}

int mcpt_moments_variance(mcpt_scene *sc, int32_t width, int32_t height, const float *moments_host, const float *len_host, const uint8_t *flags_host,
                          const float *aov_host, const mcpt_moments_opts *opts, float *out_variance_host) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_moments_variance: ") + what); };
    if (!sc || !moments_host || !len_host || !aov_host || !opts || !out_variance_host) return bad("null argument");
    if (!frame_ok(width, height)) return bad("width and height must be positive (and the frame not too large)");
    mo::Opts o;
    if (mo::resolve_opts(*opts, o) != 0) return bad("option out of range");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)width * height;
    DevBuf<float> mom, len, aov, out;
    DevBuf<uint8_t> flags;
    HIP_TRY(upload(mom, moments_host, n_px * 2));
    HIP_TRY(upload(len, len_host, n_px));
    HIP_TRY(upload(aov, aov_host, n_px * 8));
    if (flags_host) HIP_TRY(upload(flags, flags_host, n_px));
    HIP_TRY(out.alloc(n_px));
    launch_moments_variance(width, height, o, mom.p, len.p, flags.p, aov.p, out.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(download(out_variance_host, out, n_px));
    return MCPT_OK;
}

int mcpt_temporal_history_weight(mcpt_scene *sc, int32_t width, int32_t height, const float *motion_host, const float *normal_host,
                                 const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host, const float *prev_normal_host,
                                 const float *prev_weight_host, const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *weight_host) {
    return temporal_call("mcpt_temporal_history_weight", Pass::history_weight, sc, width, height, {nullptr, nullptr, motion_host, normal_host, 3, nullptr, 1},
                         {prev_color_host, nullptr, prev_depth_host, prev_len_host, prev_normal_host, prev_weight_host}, opts, hopts,
                         {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, weight_host});
}

int mcpt_temporal_history_len(mcpt_scene *sc, int32_t width, int32_t height, const float *motion_host, const float *normal_host,
                              const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host, const float *prev_normal_host,
                              const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *len_host) {
    return temporal_call("mcpt_temporal_history_len", Pass::history_len, sc, width, height, {nullptr, nullptr, motion_host, normal_host, 3, nullptr, 1},
                         {prev_color_host, nullptr, prev_depth_host, prev_len_host, prev_normal_host}, opts, hopts,
                         {nullptr, nullptr, nullptr, len_host, nullptr, nullptr});
}

void mcpt_sequence_destroy(mcpt_sequence *seq) {
    if (!seq) return;
    (void)hipSetDevice(seq->device);
    (void)hipDeviceSynchronize();  // (nothing of a frame may still read the buffers)
    delete seq;
}

int mcpt_sequence_create(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, mcpt_sequence **out) {
    return mcpt_sequence_create_ex(sc, width, height, opts, nullptr, out);
}

int mcpt_sequence_create_ex(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                            mcpt_sequence **out) {
    return mcpt_sequence_create_adaptive(sc, width, height, opts, hopts, nullptr, out);
}

int mcpt_sequence_create_adaptive(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                                  const mcpt_sequence_adaptive *aopts, mcpt_sequence **out) {
    return mcpt_sequence_create_motion(sc, width, height, opts, hopts, aopts, nullptr, out);
}

int mcpt_sequence_create_motion(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                                const mcpt_sequence_adaptive *aopts, const mcpt_sequence_motion *mopts, mcpt_sequence **out) {
    return mcpt_sequence_create_weighted(sc, width, height, opts, hopts, aopts, mopts, nullptr, out);
}

int mcpt_sequence_create_weighted(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                                  const mcpt_sequence_adaptive *aopts, const mcpt_sequence_motion *mopts, const mcpt_sequence_weighted *wopts,
                                  mcpt_sequence **out) {
    return mcpt_sequence_create_moments(sc, width, height, opts, hopts, aopts, mopts, wopts, nullptr, out);
}

int mcpt_sequence_create_moments(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                                 const mcpt_sequence_adaptive *aopts, const mcpt_sequence_motion *mopts, const mcpt_sequence_weighted *wopts,
                                 const mcpt_moments_opts *momopts, mcpt_sequence **out) {
    return mcpt_sequence_create_features(sc, width, height, opts, hopts, aopts, mopts, wopts, momopts, nullptr, out);
}

int mcpt_sequence_create_features(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                                  const mcpt_sequence_adaptive *aopts, const mcpt_sequence_motion *mopts, const mcpt_sequence_weighted *wopts,
                                  const mcpt_moments_opts *momopts, const mcpt_feature_opts *fopts, mcpt_sequence **out) {
    return mcpt_sequence_create_feedback(sc, width, height, opts, hopts, aopts, mopts, wopts, momopts, fopts, nullptr, out);
}

int mcpt_sequence_create_feedback(mcpt_scene *sc, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *hopts,
                                  const mcpt_sequence_adaptive *aopts, const mcpt_sequence_motion *mopts, const mcpt_sequence_weighted *wopts,
                                  const mcpt_moments_opts *momopts, const mcpt_feature_opts *fopts, const mcpt_feedback_opts *fbopts,
                                  mcpt_sequence **out) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_sequence_create: ") + what); };
    if (!sc || !opts || !out) return bad("null argument");
    *out = nullptr;
    tp::HistOpts ho{};
    if (hopts && tp::resolve_history_opts(*hopts, ho) != 0) return bad("history option out of range");
    if (!frame_ok(width, height)) return bad("width and height must be positive (and the frame not too large)");
    tp::Opts to;
    dn::Opts dno;
    if (tp::resolve_opts(opts->temporal, to) != 0) return bad("temporal option out of range");
    if (dn::resolve_opts(opts->denoise, dno) != 0 || opts->denoise.aov_spp > kMaxAovSpp) return bad("denoise option out of range");
    if (opts->filter != 0 && opts->filter != 1) return bad("filter must be 0 or 1");
    for (int k = 0; k < 7; ++k)
        if (opts->reserved[k] != 0) return bad("reserved words must be 0");
    if (aopts) {
        // what of the rule does not depend on a frame's params.spp (mcpt_sequence_frame checks the rest)
        const mcpt_adaptive &r = aopts->rule;
        if (r.min_spp < 2) return bad("adaptive: min_spp must be at least 2");
        if (!(r.threshold >= 0.f) || !(r.threshold <= 3.0e38f)) return bad("adaptive: threshold must be finite and >= 0");
        if (!(r.rel_floor > 0.f)) return bad("adaptive: rel_floor must be > 0");
        if (r.dilate != 0 && r.dilate != 1) return bad("adaptive: dilate must be 0 or 1");
        if (aopts->guided != 0 && aopts->guided != 1) return bad("adaptive: guided must be 0 or 1");
        for (int k = 0; k < 4; ++k)
            if (r.reserved[k] != 0) return bad("adaptive: reserved words must be 0");
        for (int k = 0; k < 7; ++k)
            if (aopts->reserved[k] != 0) return bad("adaptive: reserved words must be 0");
        if (opts->denoise.aov_spp > r.min_spp) return bad("adaptive: denoise.aov_spp must be at most min_spp");
    }
    if (mopts) {
        if (mopts->specular_motion != 0 && mopts->specular_motion != 1) return bad("motion: specular_motion must be 0 or 1");
        for (int k = 0; k < 7; ++k)
            if (mopts->reserved[k] != 0) return bad("motion: reserved words must be 0");
    }
    if (wopts) {
        if (wopts->weighted != 0 && wopts->weighted != 1) return bad("weighted: weighted must be 0 or 1");
        for (int k = 0; k < 7; ++k)
            if (wopts->reserved[k] != 0) return bad("weighted: reserved words must be 0");
    }
    const bool weighted = wopts && wopts->weighted == 1;
    mo::Opts mo_opts{};
    if (momopts && mo::resolve_opts(*momopts, mo_opts) != 0) return bad("moments: option out of range");
    const bool moments = momopts && momopts->enabled == 1;
    if (moments && aopts) return bad("moments: an adaptive rule brings its own variance (its counts need min_spp >= 2)");
    if (moments && weighted) return bad("moments: weighted must be 0 (a one-sample sequence has uniform counts)");
    bool centre = false;
    if (const int rc = check_features("mcpt_sequence_create", fopts, opts->denoise.aov_spp, centre)) return rc;
    int feedback = 0;
    if (dn::resolve_feedback(fbopts, dno, feedback) != 0) return bad("feedback: iteration must be 0 or 1..denoise.iterations, reserved words 0");
    if (feedback > 0 && opts->filter == 0) return bad("feedback: needs filter 1 (the history is an iteration of the filter)");
    if (feedback > 0 && aopts) return bad("feedback: does not combine with an adaptive rule");
    if (feedback > 0 && weighted) return bad("feedback: weighted must be 0");
    // (with a specular depth of 0 the chains are the first hits: the switch changes nothing)
    const bool chain_motion = mopts && mopts->specular_motion == 1 && opts->denoise.specular_depth > 0;
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    mcpt_sequence *seq = new (std::nothrow) mcpt_sequence();
    if (!seq) return fail(MCPT_ERR_OOM, "mcpt_sequence_create: host allocation failed");
    seq->sc = sc;
    seq->device = sc->device;
    seq->W = width;
    seq->H = height;
    seq->opts = *opts;
    seq->temporal = to;
    seq->reject = ho;
    seq->denoise = dno;
    if (aopts) {
        seq->adaptive = true;
        seq->rule = aopts->rule;
        seq->guided = aopts->guided != 0;
    }
    seq->chain_motion = chain_motion;
    seq->weighted = weighted;
    seq->moments = moments;
    seq->mopts = mo_opts;
    seq->centre = centre;
    seq->feedback = feedback;
    const size_t n_px = (size_t)width * height;
    hipError_t e = hipSuccess;
    const auto also = [&](auto &buf, size_t n) {
        if (e == hipSuccess) e = buf.alloc(n);
    };
    for (int k = 0; k < 2; ++k) {
        if (e == hipSuccess) e = seq->hist[k].alloc(n_px, ho.normal_test != 0, ho.normal_test || ho.color_clamp, weighted, moments, feedback > 0);
        if (e == hipSuccess) e = seq->hist[k].clear(n_px);
    }
    also(seq->fb, n_px * 3);
    if (!moments) also(seq->mom, n_px * 6);
    if (!moments) also(seq->var, n_px);  // (a moments sequence has no variance of the frame)
    also(seq->aov, n_px * 8);
    if (opts->denoise.specular_depth > 0 && !chain_motion) also(seq->aov_first, n_px * 8);
    if (chain_motion) {  // for the most feature samples a frame can ask for (aov_spp 0: at most 4; centre features: always 1)
        seq->map_rays = motion_map_rays(n_px, centre ? 1 : opts->denoise.aov_spp == 0 ? 4 : opts->denoise.aov_spp);
        also(seq->maps, seq->map_rays * 6);
    }
    also(seq->motion, n_px * 4);
    if (opts->filter) also(seq->out, n_px * 3);
    also(seq->rgba, n_px * 4);
    if (opts->filter && e == hipSuccess) e = seq->db.alloc(n_px);
    if (aopts) {  // every working buffer of the rounds, for all pixels active
        for (int k = 0; k < 2; ++k)
            if (e == hipSuccess) e = seq->cnt[k].alloc(n_px);
        also(seq->stamp, n_px);
        if (e == hipSuccess) e = seq->lists.alloc((uint32_t)n_px, true);
    }
    if (e == hipSuccess) e = seq->ev.create();
    // the snapshot's arrays are allocated here too, so that the one at the end of a frame only copies
    const int rc = e == hipSuccess ? mcpt_scene_snapshot(sc)
                                   : fail(e == hipErrorOutOfMemory ? MCPT_ERR_OOM : MCPT_ERR_HIP, std::string("mcpt_sequence_create: ") + hipGetErrorString(e));
    if (rc != MCPT_OK) {
        delete seq;
        return rc;
    }
    *out = seq;
    return MCPT_OK;
}

int mcpt_sequence_flags(mcpt_sequence *seq, uint8_t *flags_host) {
    if (!seq || !flags_host) return fail(MCPT_ERR_ARG, "mcpt_sequence_flags: null argument");
    const DevBuf<uint8_t> &flags = seq->hist[seq->cur].flags;  // (the set the last successful frame wrote)
    if (!flags.p) return fail(MCPT_ERR_ARG, "mcpt_sequence_flags: the sequence was created without history rejection and keeps no flags");
    HIP_TRY(hipSetDevice(seq->device));
    HIP_TRY(download(flags_host, flags, (size_t)seq->W * seq->H));
    return MCPT_OK;
}

int mcpt_sequence_weight(mcpt_sequence *seq, float *weight_host) {
    if (!seq || !weight_host) return fail(MCPT_ERR_ARG, "mcpt_sequence_weight: null argument");
    const DevBuf<float> &weight = seq->hist[seq->cur].weight;  // (the set the last successful frame wrote)
    if (!weight.p) return fail(MCPT_ERR_ARG, "mcpt_sequence_weight: the sequence was created without weighted 1 and keeps no weights");
    HIP_TRY(hipSetDevice(seq->device));
    HIP_TRY(download(weight_host, weight, (size_t)seq->W * seq->H));
    return MCPT_OK;
}

int mcpt_sequence_moments(mcpt_sequence *seq, float *moments_host) {
    if (!seq || !moments_host) return fail(MCPT_ERR_ARG, "mcpt_sequence_moments: null argument");
    const DevBuf<float> &moments = seq->hist[seq->cur].moments;  // (the set the last successful frame wrote)
    if (!moments.p) return fail(MCPT_ERR_ARG, "mcpt_sequence_moments: the sequence was created without moments and keeps none");
    HIP_TRY(hipSetDevice(seq->device));
    HIP_TRY(download(moments_host, moments, (size_t)seq->W * seq->H * 2));
    return MCPT_OK;
}

int mcpt_sequence_history(mcpt_sequence *seq, float *color_host, float *variance_host) {
    if (!seq || !color_host) return fail(MCPT_ERR_ARG, "mcpt_sequence_history: null argument");
    const History &h = seq->hist[seq->cur];  // (the set the last successful frame wrote: what the next frame reads)
    const bool fed = seq->feedback > 0;
    if (fed && variance_host && !h.fed_variance.p)
        return fail(MCPT_ERR_ARG, "mcpt_sequence_history: a moments sequence with feedback keeps no fed variance");
    const size_t n_px = (size_t)seq->W * seq->H;
    HIP_TRY(hipSetDevice(seq->device));
    HIP_TRY(download(color_host, fed ? h.fed_color : h.color, n_px * 3));
    if (variance_host) HIP_TRY(download(variance_host, fed ? h.fed_variance : h.variance, n_px));
    return MCPT_OK;
}

int mcpt_sequence_counts(mcpt_sequence *seq, int32_t *spp_host, float *err_host, float *guide_host, mcpt_adaptive_info *info) {
    if (!seq) return fail(MCPT_ERR_ARG, "mcpt_sequence_counts: null sequence");
    if (!seq->adaptive) return fail(MCPT_ERR_ARG, "mcpt_sequence_counts: the sequence was created without an adaptive rule and keeps no counts");
    const Counts &c = seq->cnt[seq->cur];  // (the set the last successful frame wrote)
    const size_t n_px = (size_t)seq->W * seq->H;
    HIP_TRY(hipSetDevice(seq->device));
    if (spp_host) HIP_TRY(download(spp_host, c.spp, n_px));
    if (err_host) HIP_TRY(download(err_host, c.err, n_px));
    if (guide_host) HIP_TRY(download(guide_host, c.guide, n_px));
    if (info) *info = seq->ainfo;
    return MCPT_OK;
}

int mcpt_sequence_reset(mcpt_sequence *seq) {
    if (!seq) return fail(MCPT_ERR_ARG, "mcpt_sequence_reset: null sequence");
    seq->fresh = true;
    seq->frame_index = 0;
    return MCPT_OK;
}

int mcpt_sequence_frame(mcpt_sequence *seq, const mcpt_camera *cam, const mcpt_params *pp, const mcpt_sequence_outputs *outputs, mcpt_sequence_info *info,
                        mcpt_stats *stats) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_sequence_frame: ") + what); };
    if (!seq || !cam || !pp) return bad("null argument");
    const mcpt_params &p = *pp;
    int rc = check_frame_call("mcpt_sequence_frame", *cam, p, kDenoisedFrame | kOneRank | kOneCallFrame | (seq->moments ? kOneSample : 0u));
    if (rc != MCPT_OK) return rc;
    if (cam->width != seq->W || cam->height != seq->H) return bad("the camera must have the width and height of the sequence");
    const mcpt_denoise_opts &dopts = seq->opts.denoise;
    if (dopts.aov_spp > p.spp) return bad("denoise.aov_spp must be at most params.spp");
    const mcpt_sequence_outputs want = outputs ? *outputs : mcpt_sequence_outputs{};
    const bool filter = seq->opts.filter != 0;
    if (want.denoised && !filter) return bad("outputs.denoised needs a sequence created with filter 1");
    if (seq->adaptive) {
        if ((rc = check_adaptive("mcpt_sequence_frame", seq->rule, p)) != MCPT_OK) return rc;
        if (dopts.aov_spp > seq->rule.min_spp) return bad("denoise.aov_spp must be at most min_spp");
    }
    const bool centre = seq->centre;  // (denoise.aov_spp is then 0 or 1: one centre ray per pixel)
    const int32_t aov_spp = centre ? 1 : dopts.aov_spp == 0 ? std::min(4, seq->adaptive ? seq->rule.min_spp : p.spp) : dopts.aov_spp;
    mcpt_scene *sc = seq->sc;
    FrameCall f{sc, p};
    if ((rc = f.begin(*cam)) != MCPT_OK) return rc;
    const hipStream_t st = nullptr;
    const int W = seq->W, H = seq->H;
    const size_t n_px = (size_t)W * H;
    const History &prev = seq->hist[seq->cur];
    History &next = seq->hist[seq->cur ^ 1];
    const StageEvents &ev = seq->ev;
    // the normals and the depth of the history come from the first-hit AOVs: channels 3-5 and 6 of the 8 (with specular motion from the
    // chain AOVs, which the motion's prev_depth is measured along)
    const int32_t motion_depth = seq->chain_motion ? dopts.specular_depth : 0;
    const float *first_hit = dopts.specular_depth > 0 && !seq->chain_motion ? seq->aov_first.p : seq->aov.p;
    // a weighted sequence: the samples behind this frame's pixels are its count map (adaptive) or params.spp (uniform)
    const int32_t *count = seq->weighted && seq->adaptive ? seq->cnt[seq->cur ^ 1].spp.p : nullptr;
    const tp::Frame planes = {seq->fb.p, seq->var.p, seq->motion.p, first_hit + 3, 8, first_hit + 6, 8, count, seq->weighted ? (float)p.spp : 0.f};
    // The feature stage, from an event the branch has recorded: the AOVs (3.) with the first-hit depth the history is validated against,
    // and the motion (4.) against the snapshot and the previous frame's camera; a fresh sequence takes no history.
    const auto features = [&]() -> int {
        int rc = aov_pass(sc, f.cc, p.seed, aov_spp, dopts.specular_depth, centre, seq->aov.p, st);
        if (rc == MCPT_OK && dopts.specular_depth > 0 && !seq->chain_motion) rc = aov_pass(sc, f.cc, p.seed, aov_spp, 0, centre, seq->aov_first.p, st);
        if (rc != MCPT_OK) return drained(rc);
        HIP_TRY(hipEventRecord(ev.aov_end, st));
        rc = motion_pass(sc, f.cc, seq->fresh ? f.cc : seq->prev_cc, p.seed, aov_spp, motion_depth, centre, seq->maps.p, seq->map_rays,
                         seq->motion.p, st);
        if (rc != MCPT_OK) return drained(rc);
        if (seq->fresh) HIP_TRY(hipMemsetAsync(prev.len.p, 0, n_px * sizeof(float), st));
        return MCPT_OK;
    };
    AdaptiveResult res;
    if (!seq->adaptive) {
        // 2. the frame with its moments, and its variance (mcpt_render_denoised, steps 1-2), then the features
        HIP_TRY(hipEventRecord(ev.render_begin, st));
        // (a moments sequence: the plain frame; seq->mom is null and neither moments nor variance of the render are formed)
        if ((rc = render_moments(f, seq->fb.p, seq->mom.p, seq->var.p, st, res)) != MCPT_OK) return rc;
        HIP_TRY(hipEventRecord(ev.render_end, st));
        if ((rc = features()) != MCPT_OK) return rc;
        HIP_TRY(hipEventRecord(ev.motion_end, st));
    } else {
        // An adaptive sequence (mcpt_sequence_create_adaptive): the features first -- they do not depend on the frame -- so that the guide
        // is known before the rounds.
        Counts &cn = seq->cnt[seq->cur ^ 1];
        HIP_TRY(hipEventRecord(ev.features_begin, st));
        if ((rc = features()) != MCPT_OK) return rc;
        // the guide: the history length each pixel is about to get (1 everywhere on a fresh sequence: prev_len is 0); counted with the motion
        // (a weighted sequence: the history weight, 0 everywhere on a fresh one)
        if (seq->guided && seq->weighted) launch_history_weight(W, H, seq->temporal, seq->reject, planes, prev.prev(), cn.guide.p, st);
        if (seq->guided && !seq->weighted) launch_history_len(W, H, seq->temporal, seq->reject, planes, prev.prev(), cn.guide.p, st);
        HIP_TRY(hipEventRecord(ev.motion_end, st));
        AdaptiveBufs b;
        b.fb = seq->fb.p;
        b.mom = seq->mom.p;
        b.spp = cn.spp.p;
        b.err = cn.err.p;
        b.stamp = seq->stamp.p;
        b.guide = seq->guided ? cn.guide.p : nullptr;
        b.guide_max_history = seq->guided && seq->weighted ? seq->temporal.max_history : 0.f;
        seq->lists.into(b);
        HIP_TRY(hipEventRecord(ev.render_begin, st));
        if ((rc = adaptive_rounds(f, seq->rule, b, nullptr, st, res)) != MCPT_OK) return rc;
        launch_dn_variance_map((uint32_t)n_px, seq->mom.p, cn.spp.p, seq->var.p, st);
        HIP_TRY(hipEventRecord(ev.render_end, st));
    }
    // 5. previous history set -> the other one
    if (seq->moments)
        launch_temporal_accumulate_moments(W, H, seq->temporal, seq->reject, planes, prev.prev(), next.next(), {prev.moments.p, next.moments.p}, st);
    else
        launch_temporal_accumulate(W, H, seq->temporal, seq->reject, planes, prev.prev(), next.next(), st);
    // 5b. a moments sequence: the variance of the accumulated frame from the new set's moments, on the AOVs the filter reads
    if (seq->moments) launch_moments_variance(W, H, seq->mopts, next.moments.p, next.len.p, next.flags.p, seq->aov.p, next.variance.p, st);
    HIP_TRY(hipEventRecord(ev.accumulate_end, st));
    // 6., 7. the filter and the tone map
    // (a feedback sequence: k_dn_feedback behind iteration seq->feedback, into the new set's fed planes; 0: launch_denoise)
    if (filter)
        launch_denoise_feedback(W, H, seq->denoise, next.color.p, next.variance.p, seq->aov.p, seq->db.rec[0].p, seq->db.rec[1].p, seq->db.grad.p,
                                seq->out.p, seq->feedback, next.fed_color.p, next.fed_variance.p, st);
    if (want.rgba) launch_tonemap(filter ? seq->out.p : next.color.p, (uint32_t)n_px, seq->rgba.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.filter_end, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (want.fb) HIP_TRY(download(want.fb, seq->fb, n_px * 3));
    if (want.accumulated) HIP_TRY(download(want.accumulated, next.color, n_px * 3));
    if (want.denoised) HIP_TRY(download(want.denoised, seq->out, n_px * 3));
    if (want.variance) HIP_TRY(download(want.variance, next.variance, n_px));
    if (want.len) HIP_TRY(download(want.len, next.len, n_px));
    if (want.aov) HIP_TRY(download(want.aov, seq->aov, n_px * 8));
    if (want.motion) HIP_TRY(download(want.motion, seq->motion, n_px * 4));
    if (want.rgba) HIP_TRY(download(want.rgba, seq->rgba, n_px * 4));
    mcpt_sequence_info timing{};
    if (info) {  // each stage between its two events: the AOVs and the accumulation begin where the branch's previous stage ended
        const auto span = [](const Event &from, const Event &to, double &ms) {
            float t = 0.f;
            const hipError_t e = hipEventElapsedTime(&t, from, to);
            ms = t;
            return e;
        };
        HIP_TRY(span(ev.render_begin, ev.render_end, timing.ms_render));
        HIP_TRY(span(seq->adaptive ? ev.features_begin : ev.render_end, ev.aov_end, timing.ms_aov));
        HIP_TRY(span(ev.aov_end, ev.motion_end, timing.ms_motion));
        HIP_TRY(span(seq->adaptive ? ev.render_end : ev.motion_end, ev.accumulate_end, timing.ms_accumulate));
        HIP_TRY(span(ev.accumulate_end, ev.filter_end, timing.ms_filter));
    }
    // 8. this frame's geometry is "previous" for the next one
    if ((rc = mcpt_scene_snapshot(sc)) != MCPT_OK) return rc;
    // the stream has drained cleanly: the history advances
    const int32_t index = seq->frame_index;
    seq->cur ^= 1;
    seq->fresh = false;
    seq->frame_index = index + 1;
    seq->prev_cc = f.cc;
    seq->ainfo = res.info;
    if (info) {
        timing.ms_total = ms_since(f.t0);
        timing.frame_index = index;
        *info = timing;
    }
    return f.end(stats, res.samples, res.traced_primary, res.totals);
}

}  // extern "C"
