// Frame sequences (include/mcpt.h: mcpt_temporal_accumulate, mcpt_sequence_*): the frame loop of temporal reuse with its history, the
// variance of the accumulated frame and every working buffer resident on the device.  A frame is the passes of csrc/mcpt_render.hip
// (csrc/mcpt_frame.h) on the sequence's buffers, k_temporal_accumulate (csrc/mcpt_temporal.hip) between the two history sets, the filter
// and the tone map, all queued on one stream; only the outputs the caller asks for are copied to the host.  A sequence created with
// history rejection (mcpt_sequence_create_ex) runs k_temporal_accumulate_ex instead and keeps a normal and a flags plane per history set.
// A sequence created with a rule (mcpt_sequence_create_adaptive) renders adaptive frames: the AOVs and the motion first, k_history_len from
// the previous history set into the guide, then the rounds of csrc/mcpt_render.hip (adaptive_rounds) on the sequence's buffers and
// k_dn_variance_map; mcpt_temporal_history_len is the guide's kernel on host arrays.
#include <new>

#include "mcpt_frame.h"

using namespace mcpt;

namespace {

// One history set: what k_temporal_accumulate reads of the previous frame and writes for the next one.
struct History {
    DevBuf<float> color, variance, depth, len;
    DevBuf<float> normal;   // first-hit normals, 3 per pixel (history rejection with the normal test only)
    DevBuf<uint8_t> flags;  // what the rejection did to each pixel of the frame that wrote this set (either switch on)
    hipError_t alloc(size_t n_px, bool with_normal, bool with_flags) {
        hipError_t e = color.alloc(n_px * 3);
        if (e == hipSuccess) e = variance.alloc(n_px);
        if (e == hipSuccess) e = depth.alloc(n_px);
        if (e == hipSuccess) e = len.alloc(n_px);
        if (e == hipSuccess && with_normal) e = normal.alloc(n_px * 3);
        if (e == hipSuccess && with_flags) e = flags.alloc(n_px);
        return e;
    }
    hipError_t clear(size_t n_px) {
        hipError_t e = hipMemset(color.p, 0, n_px * 3 * sizeof(float));
        if (e == hipSuccess) e = hipMemset(variance.p, 0, n_px * sizeof(float));
        if (e == hipSuccess) e = hipMemset(depth.p, 0, n_px * sizeof(float));
        if (e == hipSuccess) e = hipMemset(len.p, 0, n_px * sizeof(float));
        if (e == hipSuccess && normal.p) e = hipMemset(normal.p, 0, n_px * 3 * sizeof(float));
        if (e == hipSuccess && flags.p) e = hipMemset(flags.p, 0, n_px);
        return e;
    }
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

constexpr int kStages = 5;  // render, AOVs, motion, accumulate, filter (+ tone map)

}  // namespace

// Members are destroyed with the scene's device current (mcpt_sequence_destroy).
struct mcpt_sequence {
    mcpt_scene *sc = nullptr;  // borrowed
    int device = 0;
    int W = 0, H = 0;
    mcpt_sequence_opts opts{};
    tp::Opts temporal{};
    tp::HistOpts reject{};  // both switches 0: the frame runs k_temporal_accumulate, as a sequence of mcpt_sequence_create
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
    Event ev[kStages + 2];  // (the last one: the end of an adaptive sequence's rounds)
    // a sequence created with mcpt_sequence_create_adaptive and a rule (all empty otherwise)
    bool adaptive = false;
    mcpt_adaptive rule{};
    bool guided = false;
    Counts cnt[2];  // indexed as hist
    DevBuf<uint8_t> stamp;
    AdaptiveLists lists;
    mcpt_adaptive_info ainfo{};  // of the last successful frame
};

extern "C" {

int mcpt_temporal_accumulate(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *motion_host,
                             const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host, const float *prev_len_host,
                             const mcpt_temporal_opts *opts, float *out_color_host, float *out_variance_host, float *out_len_host) {
    if (!sc || !color_host || !variance_host || !motion_host || !prev_color_host || !prev_variance_host || !prev_depth_host || !prev_len_host || !opts ||
        !out_color_host || !out_variance_host || !out_len_host)
        return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate: null argument");
    if (!frame_ok(width, height)) return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate: width and height must be positive (and the frame not too large)");
    tp::Opts o;
    if (tp::resolve_opts(*opts, o) != 0) return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate: option out of range");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)width * height;
    DevBuf<float> col, var, mot, pcol, pvar, pz, plen, out, ovar, olen;
    HIP_TRY(out.alloc(n_px * 3));
    HIP_TRY(ovar.alloc(n_px));
    HIP_TRY(olen.alloc(n_px));
    HIP_TRY(upload(col, color_host, n_px * 3));
    HIP_TRY(upload(var, variance_host, n_px));
    HIP_TRY(upload(mot, motion_host, n_px * 4));
    HIP_TRY(upload(pcol, prev_color_host, n_px * 3));
    HIP_TRY(upload(pvar, prev_variance_host, n_px));
    HIP_TRY(upload(pz, prev_depth_host, n_px));
    HIP_TRY(upload(plen, prev_len_host, n_px));
    launch_temporal_accumulate(width, height, o, col.p, var.p, mot.p, pcol.p, pvar.p, pz.p, plen.p, nullptr, 0, out.p, ovar.p, nullptr, olen.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(download(out_color_host, out, n_px * 3));
    HIP_TRY(download(out_variance_host, ovar, n_px));
    HIP_TRY(download(out_len_host, olen, n_px));
    return MCPT_OK;
}

int mcpt_temporal_accumulate_ex(mcpt_scene *sc, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *motion_host,
                                const float *normal_host, const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host,
                                const float *prev_len_host, const float *prev_normal_host, const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts,
                                float *out_color_host, float *out_variance_host, float *out_len_host, uint8_t *out_flags_host) {
    if (!sc || !color_host || !variance_host || !motion_host || !prev_color_host || !prev_variance_host || !prev_depth_host || !prev_len_host || !opts ||
        !hopts || !out_color_host || !out_variance_host || !out_len_host)
        return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate_ex: null argument");
    if (!frame_ok(width, height)) return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate_ex: width and height must be positive (and the frame not too large)");
    tp::Opts o;
    tp::HistOpts ho;
    if (tp::resolve_opts(*opts, o) != 0) return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate_ex: option out of range");
    if (tp::resolve_history_opts(*hopts, ho) != 0) return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate_ex: history option out of range");
    if (ho.normal_test && (!normal_host || !prev_normal_host)) return fail(MCPT_ERR_ARG, "mcpt_temporal_accumulate_ex: normal_test needs both normal arrays");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)width * height;
    const bool reject = ho.normal_test || ho.color_clamp;
    DevBuf<float> col, var, mot, nrm, pcol, pvar, pz, plen, pnrm, out, ovar, olen;
    DevBuf<uint8_t> oflags;
    HIP_TRY(out.alloc(n_px * 3));
    HIP_TRY(ovar.alloc(n_px));
    HIP_TRY(olen.alloc(n_px));
    if (reject && out_flags_host) HIP_TRY(oflags.alloc(n_px));
    HIP_TRY(upload(col, color_host, n_px * 3));
    HIP_TRY(upload(var, variance_host, n_px));
    HIP_TRY(upload(mot, motion_host, n_px * 4));
    HIP_TRY(upload(pcol, prev_color_host, n_px * 3));
    HIP_TRY(upload(pvar, prev_variance_host, n_px));
    HIP_TRY(upload(pz, prev_depth_host, n_px));
    HIP_TRY(upload(plen, prev_len_host, n_px));
    if (ho.normal_test) {
        HIP_TRY(upload(nrm, normal_host, n_px * 3));
        HIP_TRY(upload(pnrm, prev_normal_host, n_px * 3));
    }
    if (reject)
        launch_temporal_accumulate_ex(width, height, o, ho, col.p, var.p, mot.p, nrm.p, 3, pcol.p, pvar.p, pz.p, plen.p, pnrm.p, nullptr, 0, out.p, ovar.p, nullptr,
                                      olen.p, nullptr, oflags.p, nullptr);
    else  // both switches 0: mcpt_temporal_accumulate's kernel
        launch_temporal_accumulate(width, height, o, col.p, var.p, mot.p, pcol.p, pvar.p, pz.p, plen.p, nullptr, 0, out.p, ovar.p, nullptr, olen.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(download(out_color_host, out, n_px * 3));
    HIP_TRY(download(out_variance_host, ovar, n_px));
    HIP_TRY(download(out_len_host, olen, n_px));
    if (out_flags_host) {
        if (reject)
            HIP_TRY(download(out_flags_host, oflags, n_px));
        else
            std::memset(out_flags_host, 0, n_px);
    }
    return MCPT_OK;
}

int mcpt_temporal_history_len(mcpt_scene *sc, int32_t width, int32_t height, const float *motion_host, const float *normal_host,
                              const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host, const float *prev_normal_host,
                              const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *len_host) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_temporal_history_len: ") + what); };
    if (!sc || !motion_host || !prev_color_host || !prev_depth_host || !prev_len_host || !opts || !len_host) return bad("null argument");
    if (!frame_ok(width, height)) return bad("width and height must be positive (and the frame not too large)");
    tp::Opts o;
    tp::HistOpts ho{};
    if (tp::resolve_opts(*opts, o) != 0) return bad("option out of range");
    if (hopts && tp::resolve_history_opts(*hopts, ho) != 0) return bad("history option out of range");
    if (ho.normal_test && (!normal_host || !prev_normal_host)) return bad("normal_test needs both normal arrays");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t n_px = (size_t)width * height;
    DevBuf<float> mot, nrm, pcol, pz, plen, pnrm, len;
    HIP_TRY(len.alloc(n_px));
    HIP_TRY(upload(mot, motion_host, n_px * 4));
    HIP_TRY(upload(pcol, prev_color_host, n_px * 3));
    HIP_TRY(upload(pz, prev_depth_host, n_px));
    HIP_TRY(upload(plen, prev_len_host, n_px));
    if (ho.normal_test) {
        HIP_TRY(upload(nrm, normal_host, n_px * 3));
        HIP_TRY(upload(pnrm, prev_normal_host, n_px * 3));
    }
    launch_history_len(width, height, o, ho, mot.p, nrm.p, 3, pcol.p, pz.p, plen.p, pnrm.p, len.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(download(len_host, len, n_px));
    return MCPT_OK;
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
    const size_t n_px = (size_t)width * height;
    hipError_t e = hipSuccess;
    const auto also = [&](auto &buf, size_t n) {
        if (e == hipSuccess) e = buf.alloc(n);
    };
    for (int k = 0; k < 2; ++k) {
        if (e == hipSuccess) e = seq->hist[k].alloc(n_px, ho.normal_test != 0, ho.normal_test || ho.color_clamp);
        if (e == hipSuccess) e = seq->hist[k].clear(n_px);
    }
    also(seq->fb, n_px * 3);
    also(seq->mom, n_px * 6);
    also(seq->var, n_px);
    also(seq->aov, n_px * 8);
    if (opts->denoise.specular_depth > 0) also(seq->aov_first, n_px * 8);
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
    for (int k = 0; k <= kStages + 1; ++k)
        if (e == hipSuccess) e = seq->ev[k].create(true);
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
    int rc = check_frame_call("mcpt_sequence_frame", *cam, p, kDenoisedFrame | kOneRank | kOneCallFrame);
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
    const int32_t aov_spp = dopts.aov_spp == 0 ? std::min(4, seq->adaptive ? seq->rule.min_spp : p.spp) : dopts.aov_spp;
    mcpt_scene *sc = seq->sc;
    FrameCall f{sc, p};
    if ((rc = f.begin(*cam)) != MCPT_OK) return rc;
    const hipStream_t st = nullptr;
    const int W = seq->W, H = seq->H;
    const size_t n_px = (size_t)W * H;
    const History &prev = seq->hist[seq->cur];
    History &next = seq->hist[seq->cur ^ 1];
    const Event *ev = seq->ev;
    Totals rt;
    uint64_t samples = 0, traced_primary = 0;
    mcpt_adaptive_info ainfo{};
    const float *first_hit = dopts.specular_depth > 0 ? seq->aov_first.p : seq->aov.p;
    if (!seq->adaptive) {
        // 2. the frame with its moments, and its variance (mcpt_render_denoised, steps 1-2)
        HIP_TRY(hipEventRecord(ev[0], st));
        HIP_TRY(hipMemsetAsync(seq->mom.p, 0, n_px * 6 * sizeof(double), st));
        if ((rc = f.pixels(p.spp, (float)p.spp, seq->fb.p, st)) != MCPT_OK) return rc;
        const PixelSet &ps = f.ps;
        if (ps.n_owned > ps.n_pix) launch_sky_moments(ps.sky, ps.n_owned - ps.n_pix, sc->view.background, p.spp, seq->mom.p, st);
        if (ps.n_pix > 0) {
            rc = render_list(sc, f.cc, p, ps.list, ps.cand, ps.n_pix, 0, p.spp, (float)p.spp, seq->fb.p, seq->mom.p, st, f.t0, rt);
            if (rc != MCPT_OK) return rc;
        }
        launch_dn_variance((uint32_t)n_px, seq->mom.p, p.spp, seq->var.p, st);
        samples = (uint64_t)ps.n_owned * p.spp;
        traced_primary = (uint64_t)ps.n_pix * p.spp;
        HIP_TRY(hipEventRecord(ev[1], st));
        // 3. the AOVs, and the first-hit depth the history is validated against
        rc = aov_pass(sc, f.cc, p.seed, aov_spp, dopts.specular_depth, seq->aov.p, st);
        if (rc == MCPT_OK && dopts.specular_depth > 0) rc = aov_pass(sc, f.cc, p.seed, aov_spp, 0, seq->aov_first.p, st);
        if (rc != MCPT_OK) return drained(rc);
        HIP_TRY(hipEventRecord(ev[2], st));
        // 4. the motion against the snapshot and the previous frame's camera
        rc = motion_pass(sc, f.cc, seq->fresh ? f.cc : seq->prev_cc, p.seed, aov_spp, seq->motion.p, st);
        if (rc != MCPT_OK) return drained(rc);
        HIP_TRY(hipEventRecord(ev[3], st));
        if (seq->fresh) HIP_TRY(hipMemsetAsync(prev.len.p, 0, n_px * sizeof(float), st));
    } else {
        // An adaptive sequence (mcpt_sequence_create_adaptive): the AOVs and the motion first -- neither depends on the frame -- so that the
        // guide is known before the rounds.  The events keep their stages: ev[1], ev[2], ev[3] around the AOVs and the motion (with the
        // guide), then ev[0] and ev[kStages + 1] around the rounds, which ms_render is taken between.
        Counts &cn = seq->cnt[seq->cur ^ 1];
        HIP_TRY(hipEventRecord(ev[1], st));
        rc = aov_pass(sc, f.cc, p.seed, aov_spp, dopts.specular_depth, seq->aov.p, st);
        if (rc == MCPT_OK && dopts.specular_depth > 0) rc = aov_pass(sc, f.cc, p.seed, aov_spp, 0, seq->aov_first.p, st);
        if (rc != MCPT_OK) return drained(rc);
        HIP_TRY(hipEventRecord(ev[2], st));
        rc = motion_pass(sc, f.cc, seq->fresh ? f.cc : seq->prev_cc, p.seed, aov_spp, seq->motion.p, st);
        if (rc != MCPT_OK) return drained(rc);
        if (seq->fresh) HIP_TRY(hipMemsetAsync(prev.len.p, 0, n_px * sizeof(float), st));
        // the guide: the history length each pixel is about to get (1 everywhere on a fresh sequence: prev_len is 0); counted with the motion
        if (seq->guided)
            launch_history_len(W, H, seq->temporal, seq->reject, seq->motion.p, first_hit + 3, 8, prev.color.p, prev.depth.p, prev.len.p, prev.normal.p,
                               cn.guide.p, st);
        HIP_TRY(hipEventRecord(ev[3], st));
        AdaptiveBufs b;
        b.fb = seq->fb.p;
        b.mom = seq->mom.p;
        b.spp = cn.spp.p;
        b.err = cn.err.p;
        b.stamp = seq->stamp.p;
        b.guide = seq->guided ? cn.guide.p : nullptr;
        seq->lists.into(b);
        AdaptiveResult res;
        HIP_TRY(hipEventRecord(ev[0], st));
        if ((rc = adaptive_rounds(f, seq->rule, b, nullptr, st, res)) != MCPT_OK) return rc;
        launch_dn_variance_map((uint32_t)n_px, seq->mom.p, cn.spp.p, seq->var.p, st);
        HIP_TRY(hipEventRecord(ev[kStages + 1], st));
        rt = res.totals;
        samples = res.samples;
        traced_primary = res.traced_primary;
        ainfo = res.info;
    }
    // 5. previous history set -> the other one
    if (seq->reject.normal_test || seq->reject.color_clamp)  // (the normals come from the AOVs the depth comes from)
        launch_temporal_accumulate_ex(W, H, seq->temporal, seq->reject, seq->fb.p, seq->var.p, seq->motion.p, first_hit + 3, 8, prev.color.p, prev.variance.p,
                                      prev.depth.p, prev.len.p, prev.normal.p, first_hit + 6, 8, next.color.p, next.variance.p, next.depth.p, next.len.p,
                                      next.normal.p, next.flags.p, st);
    else
        launch_temporal_accumulate(W, H, seq->temporal, seq->fb.p, seq->var.p, seq->motion.p, prev.color.p, prev.variance.p, prev.depth.p, prev.len.p,
                                   first_hit + 6, 8, next.color.p, next.variance.p, next.depth.p, next.len.p, st);
    HIP_TRY(hipEventRecord(ev[4], st));
    // 6., 7. the filter and the tone map
    if (filter) launch_denoise(W, H, seq->denoise, next.color.p, next.variance.p, seq->aov.p, seq->db.rec[0].p, seq->db.rec[1].p, seq->db.grad.p, seq->out.p, st);
    if (want.rgba) launch_tonemap(filter ? seq->out.p : next.color.p, (uint32_t)n_px, seq->rgba.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (want.fb) HIP_TRY(download(want.fb, seq->fb, n_px * 3));
    if (want.accumulated) HIP_TRY(download(want.accumulated, next.color, n_px * 3));
    if (want.denoised) HIP_TRY(download(want.denoised, seq->out, n_px * 3));
    if (want.variance) HIP_TRY(download(want.variance, next.variance, n_px));
    if (want.len) HIP_TRY(download(want.len, next.len, n_px));
    if (want.aov) HIP_TRY(download(want.aov, seq->aov, n_px * 8));
    if (want.motion) HIP_TRY(download(want.motion, seq->motion, n_px * 4));
    if (want.rgba) HIP_TRY(download(want.rgba, seq->rgba, n_px * 4));
    float ms[kStages] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (info) {
        for (int k = seq->adaptive ? 1 : 0; k < kStages; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        if (seq->adaptive) {  // the rounds ran after the motion stage: ev[0] .. ev[kStages + 1]; the accumulate stage starts where they end
            HIP_TRY(hipEventElapsedTime(&ms[0], ev[0], ev[kStages + 1]));
            HIP_TRY(hipEventElapsedTime(&ms[3], ev[kStages + 1], ev[4]));
        }
    }
    // 8. this frame's geometry is "previous" for the next one
    if ((rc = mcpt_scene_snapshot(sc)) != MCPT_OK) return rc;
    // the stream has drained cleanly: the history advances
    const int32_t index = seq->frame_index;
    seq->cur ^= 1;
    seq->fresh = false;
    seq->frame_index = index + 1;
    seq->prev_cc = f.cc;
    seq->ainfo = ainfo;
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->ms_render = ms[0];
        info->ms_aov = ms[1];
        info->ms_motion = ms[2];
        info->ms_accumulate = ms[3];
        info->ms_filter = ms[4];
        info->ms_total = ms_since(f.t0);
        info->frame_index = index;
    }
    return f.end(stats, samples, traced_primary, rt);
}

}  // extern "C"
