// Feature buffers and the guided a-trous denoiser (include/mcpt.h: mcpt_render_aovs, mcpt_denoise, mcpt_render_denoised).
//
// AOV pass, per chunk of whole pixels (at most kAovChunkRays rays):
//   k_aov_keys      ray j -> (pixel, sample): pixel-major, so that a pixel's samples are neighbours and in sample order
//   k_camera_rays   the renderer's camera-ray generator (mcpt_camera_rays)
//   k_trace_closest the scene's closest-hit traversal (mcpt_intersect)
//   k_aov_resolve   hit -> per-sample record {albedo.rgb, depth} {normal.xyz, hit}
//   k_aov_fold      one lane per pixel: the samples folded in sample order into the 8-float AOV record
// With centre features (mcpt_feature_opts) k_centre_rays (csrc/mcpt_kernels.hip) takes the place of the first two, at one ray per pixel.
// With specular_depth > 0 (mcpt_render_aovs_ex) k_aov_chain takes k_aov_resolve's place: a sample whose hit is a Dirac (mirror or glass)
// vertex continues, compacted into the next ray list, which k_trace_closest traces; at most specular_depth more steps, then k_aov_fold.
// Denoise (csrc/mcpt_denoise.h has the arithmetic, shared with the CPU build the tests compare against):
//   k_dn_prep       demodulation, scaled variance, depth gradient -> 32-byte records {e.rgb, v} {n.xyz, z}
//   k_dn_atrous     one iteration (step 2^i), 16 x 16 pixel blocks, two 16-byte loads per tap, ping-pong between two record buffers
//   k_dn_remod      out = e * A (or the colour, for a pixel that passes through)
//   k_dn_feedback   the same of the records after iteration k, with their variance: the history of a feedback sequence (mcpt_denoise_feedback)
//   k_dn_variance   the luminance variance of the mean from the moments of k_accumulate<true> (mcpt_render_denoised)
//   k_dn_variance_map  the same from each pixel's own sample count (an adaptive frame: mcpt_render_adaptive_guided)
#include <hip/hip_runtime.h>

#include "mcpt_chain.h"
#include "mcpt_denoise.h"

namespace mcpt {

namespace {

constexpr int kB = 256;
constexpr int kTile = 16;  // k_dn_* blocks: kTile x kTile pixels
inline uint32_t nblocks(uint32_t n) { return (n + kB - 1) / kB; }

__global__ __launch_bounds__(kB) void k_aov_keys(uint32_t p0, uint32_t n, int32_t aov_spp, uint32_t *__restrict__ pixel, uint32_t *__restrict__ sample) {
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= n) return;
    pixel[j] = p0 + j / (uint32_t)aov_spp;
    sample[j] = j % (uint32_t)aov_spp;
}

// Per sample: albedo as the shading reads it (k_shade: uv from the recorded hit's barycentrics for textured triangles, Material.hpp:134-151
// for conductors; 1 for dielectrics, emitters and misses), the normal of k_shade flipped to face the ray, the hit distance.
__global__ __launch_bounds__(kB) void k_aov_resolve(DevScene S, uint32_t n, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                    const uint4 *__restrict__ hit, float4 *__restrict__ s0, float4 *__restrict__ s1) {
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= n) return;
    const uint4 h = hit[j];
    const int32_t prim = (int32_t)h.z;
    if (prim < 0) {
        s0[j] = make_float4(1.f, 1.f, 1.f, 0.f);
        s1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const double t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
    const uint32_t mat_bits = h.w;
    const float4 o4 = ray_o[j], d4 = ray_d[j];
    const f3 ro = mk3(o4.x, o4.y, o4.z), rd = mk3(d4.x, d4.y, d4.z);
    f3 nrm;
    f2 uv;
    hit_surface(S, prim, mat_bits, ro, rd, ro + rd * (float)t, nrm, uv);
    if (dot(nrm, rd) > 0) nrm = -nrm;
    float alb[3];
    hit_albedo(S.mats[mat_bits & kMatIndexMask], mat_bits, uv, alb);
    s0[j] = make_float4(alb[0], alb[1], alb[2], (float)t);
    s1[j] = make_float4(nrm.x, nrm.y, nrm.z, 1.f);
}

// One step of the specular chains (include/mcpt.h: mcpt_render_aovs_ex) for the n rays of a list whose samples have all followed b bounces:
// ray i belongs to sample j with throughput thr and summed distance tsum (chain_in / tsum_in; nullptr for the camera rays: j = i, thr = 1,
// tsum = 0).  A sample that stops writes its per-sample record s0[j], s1[j] as k_aov_resolve does; one that follows a Dirac bounce
// (b < max_b) appends its next ray and state to the next list (ballot + prefix count, one atomic per wave on n_next).
__global__ __launch_bounds__(kB) void k_aov_chain(DevScene S, uint32_t n, int32_t b, int32_t max_b, const float4 *__restrict__ ray_o,
                                                  const float4 *__restrict__ ray_d, const uint4 *__restrict__ hit,
                                                  const float4 *__restrict__ chain_in, const double *__restrict__ tsum_in,
                                                  float4 *__restrict__ s0, float4 *__restrict__ s1, float4 *__restrict__ next_o,
                                                  float4 *__restrict__ next_d, float4 *__restrict__ chain_out, double *__restrict__ tsum_out,
                                                  uint32_t *__restrict__ n_next) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    bool cont = false;  // (no early return: every lane takes part in the ballot)
    uint32_t j = i;
    float thr[3] = {1.f, 1.f, 1.f};
    double tsum = 0.0;
    f3 p2 = mk3(0, 0, 0), wi = mk3(0, 0, 1);
    if (i < n) {
        if (chain_in) {
            const float4 c = chain_in[i];
            thr[0] = c.x;
            thr[1] = c.y;
            thr[2] = c.z;
            j = __float_as_uint(c.w);
            tsum = tsum_in[i];
        }
        const uint4 h = hit[i];
        const int32_t prim = (int32_t)h.z;
        if (prim < 0) {
            s0[j] = make_float4(thr[0], thr[1], thr[2], 0.f);
            s1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const double t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
            tsum += t;
            const uint32_t mat_bits = h.w;
            const float4 o4 = ray_o[i], d4 = ray_d[i];
            const f3 ro = mk3(o4.x, o4.y, o4.z), rd = mk3(d4.x, d4.y, d4.z);
            const f3 p = ro + rd * (float)t;
            f3 nrm;
            f2 uv;
            hit_surface(S, prim, mat_bits, ro, rd, p, nrm, uv);
            const MaterialRec &M = S.mats[mat_bits & kMatIndexMask];
            const bool conductor = M.type == MCPT_SMOOTH_CONDUCTOR || M.type == MCPT_ROUGH_CONDUCTOR;
            cont = chain_continues(M, mat_bits, b, max_b);
            if (cont) {  // the bounce both chain passes take (csrc/mcpt_chain.h)
                const f3 wo = -rd;
                chain_bounce(M, rd, p, nrm, p2, wi);
                if (conductor)
                    for (int c = 0; c < 3; ++c) thr[c] *= mat_eval(M, wi, wo, nrm, c, uv, true);
            } else {
                if (dot(nrm, rd) > 0) nrm = -nrm;
                float alb[3];
                hit_albedo(M, mat_bits, uv, alb);
                s0[j] = make_float4(thr[0] * alb[0], thr[1] * alb[1], thr[2] * alb[2], (float)tsum);
                s1[j] = make_float4(nrm.x, nrm.y, nrm.z, 1.f);
            }
        }
    }
    const unsigned long long mask = __ballot(cont);
    if (mask == 0ull) return;
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(n_next, (uint32_t)__popcll(mask));
    base = __shfl(base, 0);
    if (cont) {
        const uint32_t k = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        next_o[k] = make_float4(p2.x, p2.y, p2.z, 0.f);
        next_d[k] = make_float4(wi.x, wi.y, wi.z, 0.f);
        chain_out[k] = make_float4(thr[0], thr[1], thr[2], __uint_as_float(j));
        tsum_out[k] = tsum;
    }
}

__global__ __launch_bounds__(kB) void k_aov_fold(uint32_t p0, uint32_t n_pix, int32_t aov_spp, const float4 *__restrict__ s0,
                                                 const float4 *__restrict__ s1, float *__restrict__ aov) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_pix) return;
    const float fn = (float)aov_spp;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f, zs = 0.f;
    int32_t hits = 0;
    const size_t base = (size_t)i * aov_spp;
    for (int32_t k = 0; k < aov_spp; ++k) {
        const float4 a = s0[base + k], b = s1[base + k];
        a0 += a.x / fn;
        a1 += a.y / fn;
        a2 += a.z / fn;
        n0 += b.x / fn;
        n1 += b.y / fn;
        n2 += b.z / fn;
        if (b.w > 0.f) {
            zs += a.w;
            ++hits;
        }
    }
    float *r = aov + (size_t)(p0 + i) * 8;
    r[0] = a0;
    r[1] = a1;
    r[2] = a2;
    r[3] = n0;
    r[4] = n1;
    r[5] = n2;
    r[6] = hits > 0 ? zs / (float)hits : 0.f;
    r[7] = (float)hits / fn;
}

__global__ __launch_bounds__(kB) void k_dn_variance(uint32_t n_px, const double *__restrict__ moments, int32_t n, float *__restrict__ var) {
    const uint32_t m = blockIdx.x * kB + threadIdx.x;
    if (m >= n_px) return;
    const double *mo = moments + (size_t)m * 6;
    var[m] = dn::luminance_variance(mo, mo + 3, (double)n);
}

// the same with each pixel's own sample count (an adaptive frame); a pixel without samples (unowned) gets 0
__global__ __launch_bounds__(kB) void k_dn_variance_map(uint32_t n_px, const double *__restrict__ moments, const int32_t *__restrict__ spp_map,
                                                         float *__restrict__ var) {
    const uint32_t m = blockIdx.x * kB + threadIdx.x;
    if (m >= n_px) return;
    const int32_t n = spp_map[m];
    const double *mo = moments + (size_t)m * 6;
    var[m] = n > 0 ? dn::luminance_variance(mo, mo + 3, (double)n) : 0.f;
}

__global__ __launch_bounds__(kTile *kTile) void k_dn_prep(int W, int H, const float *__restrict__ color, const float *__restrict__ variance,
                                                         const float *__restrict__ aov, dn::Rec *__restrict__ rec, float2 *__restrict__ grad) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    dn::Rec r;
    float g[2];
    dn::prep_pixel(W, H, x, y, color, variance, aov, r, g);
    const size_t m = (size_t)y * W + x;
    rec[m] = r;
    grad[m] = make_float2(g[0], g[1]);
}

__global__ __launch_bounds__(kTile *kTile) void k_dn_atrous(int W, int H, int step, dn::Opts o, const dn::Rec *__restrict__ in,
                                                           const float2 *__restrict__ grad, dn::Rec *__restrict__ out) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t m = (size_t)y * W + x;
    const float2 g2 = grad[m];
    const float g[2] = {g2.x, g2.y};
    auto load = [in](size_t q) {
        const float4 a = reinterpret_cast<const float4 *>(in + q)[0], b = reinterpret_cast<const float4 *>(in + q)[1];
        dn::Rec r;
        r.e[0] = a.x; r.e[1] = a.y; r.e[2] = a.z; r.v = a.w;
        r.n[0] = b.x; r.n[1] = b.y; r.n[2] = b.z; r.z = b.w;
        return r;
    };
    dn::Rec r;
    dn::atrous_pixel(W, H, x, y, step, o, load, g, r);
    out[m] = r;
}

__global__ __launch_bounds__(kB) void k_dn_remod(uint32_t n_px, const dn::Rec *__restrict__ rec, const float *__restrict__ color,
                                                 const float *__restrict__ aov, float *__restrict__ out) {
    const uint32_t m = blockIdx.x * kB + threadIdx.x;
    if (m >= n_px) return;
    dn::remod_pixel(m, rec[m], color, aov, out);
}

// One pixel per lane: the record after iteration k, the pixel's colour, variance and albedo in; fed colour and variance out.
__global__ __launch_bounds__(kB) void k_dn_feedback(uint32_t n_px, const dn::Rec *__restrict__ rec, const float *__restrict__ color,
                                                    const float *__restrict__ variance, const float *__restrict__ aov, float *__restrict__ fb_color,
                                                    float *__restrict__ fb_variance) {
    const uint32_t m = blockIdx.x * kB + threadIdx.x;
    if (m >= n_px) return;
    dn::feedback_pixel(m, rec[m], color, variance, aov, fb_color, fb_variance);
}

}  // namespace

void launch_aov_keys(uint32_t p0, uint32_t n, int32_t aov_spp, uint32_t *pixel, uint32_t *sample, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_aov_keys, dim3(nblocks(n)), dim3(kB), 0, st, p0, n, aov_spp, pixel, sample);
}

void launch_aov_resolve(const DevScene &S, uint32_t n, const float4 *ray_o, const float4 *ray_d, const uint4 *hit, float4 *s0, float4 *s1, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_aov_resolve, dim3(nblocks(n)), dim3(kB), 0, st, S, n, ray_o, ray_d, hit, s0, s1);
}

void launch_aov_chain(const DevScene &S, uint32_t n, int32_t b, int32_t max_b, const float4 *ray_o, const float4 *ray_d, const uint4 *hit,
                      const float4 *chain_in, const double *tsum_in, float4 *s0, float4 *s1, float4 *next_o, float4 *next_d, float4 *chain_out,
                      double *tsum_out, uint32_t *n_next, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_aov_chain, dim3(nblocks(n)), dim3(kB), 0, st, S, n, b, max_b, ray_o, ray_d, hit, chain_in, tsum_in, s0, s1, next_o, next_d,
                       chain_out, tsum_out, n_next);
}

void launch_aov_fold(uint32_t p0, uint32_t n_pix, int32_t aov_spp, const float4 *s0, const float4 *s1, float *aov, hipStream_t st) {
    if (n_pix == 0) return;
    hipLaunchKernelGGL(k_aov_fold, dim3(nblocks(n_pix)), dim3(kB), 0, st, p0, n_pix, aov_spp, s0, s1, aov);
}

void launch_dn_variance(uint32_t n_px, const double *moments, int32_t n, float *var, hipStream_t st) {
    if (n_px == 0) return;
    hipLaunchKernelGGL(k_dn_variance, dim3(nblocks(n_px)), dim3(kB), 0, st, n_px, moments, n, var);
}

void launch_dn_variance_map(uint32_t n_px, const double *moments, const int32_t *spp_map, float *var, hipStream_t st) {
    if (n_px == 0) return;
    hipLaunchKernelGGL(k_dn_variance_map, dim3(nblocks(n_px)), dim3(kB), 0, st, n_px, moments, spp_map, var);
}

void launch_denoise(int W, int H, const dn::Opts &o, const float *color, const float *variance, const float *aov, dn::Rec *rec0, dn::Rec *rec1,
                    float2 *grad, float *out, hipStream_t st) {
    launch_denoise_feedback(W, H, o, color, variance, aov, rec0, rec1, grad, out, 0, nullptr, nullptr, st);
}

void launch_denoise_feedback(int W, int H, const dn::Opts &o, const float *color, const float *variance, const float *aov, dn::Rec *rec0,
                             dn::Rec *rec1, float2 *grad, float *out, int k, float *fb_color, float *fb_variance, hipStream_t st) {
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), blk(kTile, kTile);
    const uint32_t n_px = (uint32_t)W * (uint32_t)H;
    hipLaunchKernelGGL(k_dn_prep, grid, blk, 0, st, W, H, color, variance, aov, rec0, grad);
    dn::Rec *buf[2] = {rec0, rec1};
    for (int i = 0; i < o.iterations; ++i) {
        hipLaunchKernelGGL(k_dn_atrous, grid, blk, 0, st, W, H, 1 << i, o, buf[i & 1], grad, buf[(i + 1) & 1]);
        if (i + 1 == k)  // (reads what iteration i + 1 reads; the next write to that buffer is iteration i + 2's, behind it on the stream)
            hipLaunchKernelGGL(k_dn_feedback, dim3(nblocks(n_px)), dim3(kB), 0, st, n_px, buf[(i + 1) & 1], color, variance, aov, fb_color, fb_variance);
    }
    hipLaunchKernelGGL(k_dn_remod, dim3(nblocks(n_px)), dim3(kB), 0, st, n_px, buf[o.iterations & 1], color, aov, out);
}

}  // namespace mcpt
