// The query entry points of the C ABI (include/mcpt.h): mcpt_intersect, mcpt_cast_rays, mcpt_camera_rays, mcpt_centre_rays, the tone map, and the debug
// entry points.  Each stages its arguments in call-local device buffers (mcpt_cast_rays: in the wavefront workspace of pool 0).
#include <cmath>

#include "mcpt_cull.h"
#include "mcpt_host.h"

using namespace mcpt;

namespace {

// float[3n] <-> float4[n] (w = 0), the layout of the ray arrays
std::vector<float4> pack3(const float *v, size_t n) {
    std::vector<float4> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = make_float4(v[3 * i], v[3 * i + 1], v[3 * i + 2], 0.f);
    return out;
}
void unpack3(const std::vector<float4> &v, float *out) {
    for (size_t i = 0; i < v.size(); ++i) {
        out[3 * i] = v[i].x;
        out[3 * i + 1] = v[i].y;
        out[3 * i + 2] = v[i].z;
    }
}

}  // namespace

extern "C" {

int mcpt_intersect(mcpt_scene *sc, int64_t n, const float *origins, const float *dirs, double *out_t, int32_t *out_prim) {
    if (!sc || n < 0 || (n > 0 && (!origins || !dirs || !out_t || !out_prim))) return fail(MCPT_ERR_ARG, "mcpt_intersect: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_intersect: too many rays for one call");
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float4> dO, dD;
    DevBuf<uint4> dH;
    HIP_TRY(upload(dO, pack3(origins, n)));
    HIP_TRY(upload(dD, pack3(dirs, n)));
    HIP_TRY(dH.alloc(n));
    RetryBufs retry;
    HIP_TRY(retry.for_rays((uint32_t)n, sc->view.height));
    launch_trace_closest(sc->view, (uint32_t)n, nullptr, dO.p, dD.p, dH.p, retry.list(0), nullptr);
    std::vector<uint4> h(n);
    HIP_TRY(download(h.data(), dH, n));
    for (int64_t i = 0; i < n; ++i) {
        const unsigned long long b = ((unsigned long long)h[i].y << 32) | h[i].x;
        double t;
        std::memcpy(&t, &b, sizeof t);
        out_t[i] = t;
        out_prim[i] = (int32_t)h[i].z;
    }
    return MCPT_OK;
}

int mcpt_cast_rays(mcpt_scene *sc, const mcpt_params *pp, int64_t n, const float *origins, const float *dirs,
                   const uint32_t *pixel, const uint32_t *sample, const int32_t *channel, float *out) {
    if (!sc || !pp || n < 0 || (n > 0 && (!origins || !dirs || !pixel || !sample || !channel || !out)))
        return fail(MCPT_ERR_ARG, "mcpt_cast_rays: bad argument");
    if (n == 0) return MCPT_OK;
    const mcpt_params &p = *pp;
    if (p.n_dir_sample <= 0 || !(p.rr_rate > 0.f)) return fail(MCPT_ERR_ARG, "mcpt_cast_rays: n_dir_sample/rr_rate must be positive");
    for (int64_t i = 0; i < n; ++i)
        if (channel[i] < 0 || channel[i] > 2) return fail(MCPT_ERR_ARG, "mcpt_cast_rays: channel must be 0..2");
    HIP_TRY(hipSetDevice(sc->device));
    PoolCtx &ctx = sc->pools[0];
    Workspace &w = ctx.ws;
    SharedBufs &sh = sc->shared;
    const int max_depth = derive_max_depth(p);
    const int64_t chunk_max = 1 << 20;
    ctx.timer.reset();
    ctx.timer.enabled = false;
    for (int64_t base = 0; base < n; base += chunk_max) {
        const uint32_t m = (uint32_t)std::min<int64_t>(chunk_max, n - base);
        const uint32_t pool = std::max<uint32_t>((m + 2) / 3 * 3, 3 * 256);
        HIP_TRY(ensure_workspace(ctx, std::max(pool, w.pool), p.n_dir_sample, std::max(max_depth, w.max_depth), stack_uses_retry(sc->view.height)));
        HIP_TRY(sh.result.alloc(m));
        // (the rays go into wave 0's ray arrays, where run_wavefront's mode 1 expects them; the keys into the shared buffers)
        HIP_TRY(upload(w.wave[0].ray_o, pack3(origins + 3 * base, m)));
        HIP_TRY(upload(w.wave[0].ray_d, pack3(dirs + 3 * base, m)));
        HIP_TRY(upload(sh.key_pixel, pixel + base, m));
        HIP_TRY(upload(sh.key_sample, sample + base, m));
        HIP_TRY(upload(sh.key_channel, channel + base, m));
        RenderConst C = base_consts(p, w.max_depth);
        C.mode = 1;
        C.key_pixel = sh.key_pixel.p;
        C.key_sample = sh.key_sample.p;
        C.key_channel = sh.key_channel.p;
        C.result[0] = C.result[1] = sh.result.p;
        Totals tot;
        const std::vector<PassPlan> plan{PassPlan{0u, m, 1, 0}};
        const int rc = drained(run_wavefront(sc, ctx, C, RaySource{}, plan, nullptr, nullptr, tot));
        if (rc != MCPT_OK) return rc;
        if (base == 0) sc->last_cont_traced = sc->last_cont_shared = sc->last_pc_samples = sc->last_pc_rays = 0;  // (mcpt_scene_ray_counts: summed over the chunks)
        sc->last_cont_traced += tot.cont_traced;
        sc->last_cont_shared += tot.cont_shared;
        HIP_TRY(download(out + base, sh.result, m));
    }
    return MCPT_OK;
}

int mcpt_camera_rays(mcpt_scene *sc, const mcpt_camera *cam, uint32_t seed, int64_t n, const uint32_t *pixel,
                     const uint32_t *sample, float *origins, float *dirs) {
    if (!sc || !cam || n < 0 || (n > 0 && (!pixel || !sample || !origins || !dirs))) return fail(MCPT_ERR_ARG, "mcpt_camera_rays: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_camera_rays: too many rays for one call");
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<uint32_t> dP, dS;
    DevBuf<float4> dO, dD;
    HIP_TRY(dO.alloc(n));
    HIP_TRY(dD.alloc(n));
    HIP_TRY(upload(dP, pixel, n));
    HIP_TRY(upload(dS, sample, n));
    launch_camera_rays(make_camera(*cam), seed, (uint32_t)n, dP.p, dS.p, dO.p, dD.p, nullptr);
    std::vector<float4> o(n), d(n);
    HIP_TRY(download(o.data(), dO, n));
    HIP_TRY(download(d.data(), dD, n));
    unpack3(o, origins);
    unpack3(d, dirs);
    return MCPT_OK;
}

// One launch of k_centre_rays per run of consecutive pixels (a whole frame in pixel order is one run).
int mcpt_centre_rays(mcpt_scene *sc, const mcpt_camera *cam, int64_t n, const uint32_t *pixel, float *origins, float *dirs) {
    if (!sc || !cam || n < 0 || (n > 0 && (!pixel || !origins || !dirs))) return fail(MCPT_ERR_ARG, "mcpt_centre_rays: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_centre_rays: too many rays for one call");
    if (cam->width <= 0 || cam->height <= 0) return fail(MCPT_ERR_ARG, "mcpt_centre_rays: width and height must be positive");
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float4> dO, dD;
    HIP_TRY(dO.alloc(n));
    HIP_TRY(dD.alloc(n));
    const CameraConst cc = make_camera(*cam);
    for (int64_t a = 0, b; a < n; a = b) {
        for (b = a + 1; b < n && pixel[b] == pixel[b - 1] + 1u; ++b) {
        }
        launch_centre_rays(cc, pixel[a], (uint32_t)(b - a), dO.p + a, dD.p + a, nullptr);
    }
    HIP_TRY(hipGetLastError());
    std::vector<float4> o(n), d(n);
    HIP_TRY(download(o.data(), dO, n));
    HIP_TRY(download(d.data(), dD, n));
    unpack3(o, origins);
    unpack3(d, dirs);
    return MCPT_OK;
}

int mcpt_tonemap_device(mcpt_scene *sc, const float *fb_device, int64_t n_pixels, uint8_t *rgba_device, void *hip_stream) {
    if (!sc || n_pixels < 0 || (n_pixels > 0 && (!fb_device || !rgba_device))) return fail(MCPT_ERR_ARG, "mcpt_tonemap_device: bad argument");
    if (n_pixels > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_tonemap_device: frame too large");
    HIP_TRY(hipSetDevice(sc->device));
    launch_tonemap(fb_device, (uint32_t)n_pixels, rgba_device, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_tonemap(mcpt_scene *sc, const float *fb_host, int64_t n_pixels, uint8_t *rgba_host) {
    if (!sc || n_pixels < 0 || (n_pixels > 0 && (!fb_host || !rgba_host))) return fail(MCPT_ERR_ARG, "mcpt_tonemap: bad argument");
    if (n_pixels == 0) return MCPT_OK;
    if (n_pixels > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_tonemap: frame too large");
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> fb;
    DevBuf<uint8_t> out;
    HIP_TRY(out.alloc((size_t)n_pixels * 4));
    HIP_TRY(upload(fb, fb_host, (size_t)n_pixels * 3));
    launch_tonemap(fb.p, (uint32_t)n_pixels, out.p, nullptr);
    HIP_TRY(download(rgba_host, out, (size_t)n_pixels * 4));
    return MCPT_OK;
}

int mcpt_debug_counters(mcpt_scene *sc, uint64_t out[16]) {
    if (!sc || !out) return fail(MCPT_ERR_ARG, "mcpt_debug_counters: null argument");
    std::memset(out, 0, 16 * sizeof(uint64_t));
    if (!sc->dbg.p) return MCPT_OK;  // a product build: nothing is counted
    HIP_TRY(hipSetDevice(sc->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long h[16];
    HIP_TRY(download(h, sc->dbg, 16));
    for (int k = 0; k < 16; ++k) out[k] = h[k];
    return MCPT_OK;
}

int mcpt_debug_fmath(mcpt_scene *sc, int kind, int64_t n, const float *x, const float *y, float *out) {
    if (!sc || kind < 0 || kind > 5 || n < 0 || (n > 0 && (!x || !out || ((kind == 2 || kind == 4) && !y)))) return fail(MCPT_ERR_ARG, "mcpt_debug_fmath: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_debug_fmath: too many values for one call");
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> dX, dY, dO;
    HIP_TRY(dY.alloc(n));
    HIP_TRY(dO.alloc(n));
    HIP_TRY(upload(dX, x, n));
    if (y) HIP_TRY(upload(dY, y, n));
    else HIP_TRY(hipMemset(dY.p, 0, n * sizeof(float)));
    launch_debug_fmath(kind, (uint32_t)n, dX.p, dY.p, dO.p, nullptr);
    HIP_TRY(download(out, dO, n));
    return MCPT_OK;
}

int mcpt_debug_material(mcpt_scene *sc, int kind, int64_t n, const float *in, const int32_t *sel, float *out) {
    if (!sc || kind < 0 || kind > 6 || n < 0 || (n > 0 && (!in || !sel || !out))) return fail(MCPT_ERR_ARG, "mcpt_debug_material: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x0fffffff) return fail(MCPT_ERR_ARG, "mcpt_debug_material: too many rows for one call");
    for (int64_t i = 0; i < n; ++i)
        if (sel[3 * i] < 0 || (size_t)sel[3 * i] >= sc->mats.bytes() / sizeof(MaterialRec) || sel[3 * i + 1] < 0 || sel[3 * i + 1] > 2) return fail(MCPT_ERR_ARG, "mcpt_debug_material: material or channel out of range");
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> dI, dO;
    DevBuf<int32_t> dS;
    HIP_TRY(dO.alloc((size_t)n * 4));
    HIP_TRY(upload(dI, in, (size_t)n * 13));
    HIP_TRY(upload(dS, sel, (size_t)n * 3));
    launch_debug_material(sc->view, kind, (uint32_t)n, dI.p, dS.p, dO.p, nullptr);
    HIP_TRY(download(out, dO, (size_t)n * 4));
    return MCPT_OK;
}

int mcpt_debug_shadow(mcpt_scene *sc, int32_t list, int64_t n, const float *origins, const float *dirs, const float *dist, const uint8_t *found,
                      const int32_t *shard, uint8_t *visible) {
    if (!sc || n < 0 || list < 0 || list > 1 || (n > 0 && (!origins || !dirs || !dist || !found || !visible)))
        return fail(MCPT_ERR_ARG, "mcpt_debug_shadow: bad argument");
    if (n > (int64_t)1 << 22) return fail(MCPT_ERR_ARG, "mcpt_debug_shadow: too many rays for one call");
    // the queue as k_direct leaves it (Counters, csrc/mcpt_kernels.h): per shard, found entries from the front of its region, the others
    // from its back
    uint32_t nf[kShadowShards] = {}, nw[kShadowShards] = {};
    std::vector<uint32_t> slot(n);  // ray i: its shard and its rank among the shard's entries of its kind
    for (int64_t i = 0; i < n; ++i) {
        if (found[i] > 1) return fail(MCPT_ERR_ARG, "mcpt_debug_shadow: found must be 0 or 1");
        if (!(dist[i] > 0.f) || !std::isfinite(dist[i])) return fail(MCPT_ERR_ARG, "mcpt_debug_shadow: dist must be finite and positive");
        const int64_t s = shard ? (int64_t)shard[i] : (i / 64) % (int64_t)kShadowShards;
        if (s < 0 || s >= (int64_t)kShadowShards) return fail(MCPT_ERR_ARG, "mcpt_debug_shadow: shard out of range");
        slot[i] = (uint32_t)s << 24 | (found[i] ? nf[s]++ : nw[s]++);  // (a rank is below 2^22)
    }
    if (n == 0) return MCPT_OK;
    uint32_t fill = 0;  // the fullest shard
    for (uint32_t s = 0; s < kShadowShards; ++s) fill = std::max(fill, nf[s] + nw[s]);
    const uint32_t cap = (fill + 63u) / 64u * 64u * kShadowShards;  // the smallest capacity whose region holds `fill` entries
    const uint32_t region = shadow_region(cap);
    std::vector<float4> qo((size_t)kShadowShards * region, make_float4(0.f, 0.f, 0.f, 0.f)), qd(qo);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t s = slot[i] >> 24, k = slot[i] & 0xffffffu;
        const uint32_t e = found[i] ? s * region + k : (s + 1u) * region - 1u - k;
        uint32_t bits = (uint32_t)i;
        float w;
        std::memcpy(&w, &bits, sizeof w);
        qo[e] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], w);
        qd[e] = make_float4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], dist[i]);
    }
    std::vector<Counters> hc(1);
    std::memset(static_cast<void *>(hc.data()), 0, sizeof(Counters));
    for (uint32_t s = 0; s < kShadowShards; ++s) {
        hc[0].n_shadow[list][s].v = nf[s];
        hc[0].n_shadow_w[list][s].v = nw[s];
    }
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float4> dO, dD;
    DevBuf<Counters> dC;
    DevBuf<float> dV;
    HIP_TRY(upload(dO, qo));
    HIP_TRY(upload(dD, qd));
    HIP_TRY(upload(dC, hc));
    HIP_TRY(upload(dV, std::vector<float>(n, 1.f)));
    RetryBufs retry;
    if (stack_uses_retry(sc->view.height)) {
        const uint32_t want[3] = {1u, (uint32_t)n, 1u};  // (the list holds queue positions: at most n)
        HIP_TRY(retry.alloc(want));
    }
    const Scratch X{nullptr, nullptr, nullptr, nullptr, dO.p, dD.p};
    launch_trace_shadow(sc->view, dC.p, list, (uint32_t)n, cap, X, dV.p, sc->knobs.shadow_grid_per_cu, retry.list(1), nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<float> c(n);
    HIP_TRY(download(c.data(), dV, n));
    for (int64_t i = 0; i < n; ++i) visible[i] = c[i] != 0.f;
    return MCPT_OK;
}

int mcpt_debug_classify(mcpt_scene *sc, const mcpt_camera *cam, uint8_t *may_hit, int32_t *cand, mcpt_cull_info *info) {
    if (!sc || !cam || !may_hit || !cand) return fail(MCPT_ERR_ARG, "mcpt_debug_classify: null argument");
    if (cam->width <= 0 || cam->height <= 0) return fail(MCPT_ERR_ARG, "mcpt_debug_classify: width and height must be positive");
    const int64_t n64 = (int64_t)cam->width * cam->height;
    if (n64 > ((int64_t)1 << 26)) return fail(MCPT_ERR_ARG, "mcpt_debug_classify: frame too large");
    const uint32_t n = (uint32_t)n64;
    HIP_TRY(hipSetDevice(sc->device));
    std::vector<uint32_t> pix(n);
    for (uint32_t m = 0; m < n; ++m) pix[m] = m;
    DevBuf<uint32_t> dP, dOut, dCount;
    DevBuf<uint8_t> dF, dT;
    DevBuf<int4> dC, dCo;
    const size_t tb = cull_temp_bytes(n);
    HIP_TRY(upload(dP, pix));
    HIP_TRY(dOut.alloc(n));
    HIP_TRY(dCount.alloc(1));
    HIP_TRY(dF.alloc(n));
    HIP_TRY(dT.alloc(tb));
    HIP_TRY(dC.alloc(n));
    HIP_TRY(dCo.alloc(n));
    uint32_t n_trace = n + 1;  // (left untouched when the camera is outside what the bound covers)
    CullBound B{};
    HIP_TRY(cull_sky_pixels(sc->view, make_camera(*cam), dP.p, n, dOut.p, dF.p, dC.p, dCo.p, dT.p, tb, dCount.p, &n_trace, sc->knobs.cull_rho_scale, &B, nullptr));
    if (info) fill_cull_info(B, info);
    if (n_trace > n) {
        for (uint32_t m = 0; m < n; ++m) {
            may_hit[m] = 1;
            cand[4 * (size_t)m] = -2;
            cand[4 * (size_t)m + 1] = cand[4 * (size_t)m + 2] = cand[4 * (size_t)m + 3] = -1;
        }
        return MCPT_OK;
    }
    std::vector<int4> c(n);
    HIP_TRY(download(may_hit, dF, n));
    HIP_TRY(download(c.data(), dC, n));
    for (uint32_t m = 0; m < n; ++m) {
        const int32_t v[4] = {c[m].x, c[m].y, c[m].z, c[m].w};
        const bool walk = v[0] == kCandTraverse;
        for (int k = 0; k < 4; ++k) cand[4 * (size_t)m + k] = walk ? (k == 0 ? -2 : -1) : (v[k] == kCandNone ? -1 : ~v[k]);
    }
    return MCPT_OK;
}

int mcpt_debug_scene(mcpt_scene *sc, int kind, int64_t n, const float *in, float *out) {
    if (!sc || kind < 0 || kind > 1 || n < 0 || (n > 0 && (!in || !out))) return fail(MCPT_ERR_ARG, "mcpt_debug_scene: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x0fffffff) return fail(MCPT_ERR_ARG, "mcpt_debug_scene: too many rows for one call");
    const size_t n_in = kind == 0 ? 4 : 3, n_out = kind == 0 ? 10 : 3;
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> dI, dO;
    HIP_TRY(dO.alloc((size_t)n * n_out));
    HIP_TRY(upload(dI, in, (size_t)n * n_in));
    launch_debug_scene(sc->view, kind, (uint32_t)n, dI.p, dO.p, nullptr);
    HIP_TRY(download(out, dO, (size_t)n * n_out));
    return MCPT_OK;
}

}  // extern "C"
