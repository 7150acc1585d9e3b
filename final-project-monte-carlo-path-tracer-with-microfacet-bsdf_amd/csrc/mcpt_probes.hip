// Light probes (include/mcpt.h: mcpt_query_probes, mcpt_probe_rays, mcpt_probe_shade, mcpt_bake_probe_grid and the host-only
// mcpt_sh_basis_host / mcpt_sh_irradiance_host / mcpt_probe_grid_points_host / mcpt_probe_shade_host).  csrc/mcpt_sh.h states the rule --
// basis, irradiance, grid lookup -- once; the whole-sphere first ray is sensor_ray's third branch (csrc/mcpt_sensor.h) and the projection
// fold k_accumulate_sh sits beside k_accumulate (csrc/mcpt_kernels.hip), launched by render_list at both of its accumulate sites.
//
// Kernels here, on the caller's stream:
//   k_probe_grid_points  one lane per probe: sh::grid_point into the scene-owned point buffer (mcpt_bake_probe_grid)
//   k_probe_shade        one lane per (point, normal): sh::probe_shade from the coefficient buffer; eight 108-byte rows are read per lane
//
// Probe visibility (mcpt_query_probe_depth, mcpt_probe_shade_visible, mcpt_bake_probe_volume and their host forms; csrc/mcpt_probe_depth.h
// states the rule).  Per chunk of the ray queries' staging buffers (QueryBufs, csrc/mcpt_host.h), on the caller's stream:
//   k_probe_depth_rays     one lane per (probe, sample): sensor_ray's whole-sphere ray straight into the staged float4 arrays, tmax = +inf
//   closest hits           launch_trace_closest on the staged chunk, as run_query (csrc/mcpt_rayquery.hip) runs it: no second tree walk
//   k_probe_depth_fold     one wave per probe, lane = texel of the 8 x 8 map: per block of 64 samples lane l prepares sample l (hit word,
//                          distance, the normal k_query_resolve reports, back-face flag; the block's back-face count is a ballot), then
//                          the wave walks the block in sample order with (d, r) broadcast from lane s by a wave-uniform lane read, and
//                          every lane adds to its texel's three sums in registers
//   k_probe_shade_visible  one lane per (point, normal): pd::shade_visible
// Every store is a plain vector store; nothing here uses atomics, LDS, scratch or inline assembly.
#include <cmath>

#include "mcpt_frame.h"
#include "mcpt_host.h"
#include "mcpt_probe_depth.h"
#include "mcpt_sh.h"

using namespace mcpt;

namespace mcpt {
namespace {

constexpr int kPbBlock = 256;  // 4 waves

__global__ __launch_bounds__(kPbBlock) void k_probe_grid_points(sh::Grid g, uint32_t n, float *__restrict__ points) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t nx = (uint32_t)g.dims[0], ny = (uint32_t)g.dims[1];
    const uint32_t ix = i % nx, r = i / nx;
    float p[3];
    sh::grid_point(g, (int32_t)ix, (int32_t)(r % ny), (int32_t)(r / ny), p);
    points[3 * (size_t)i] = p[0];
    points[3 * (size_t)i + 1] = p[1];
    points[3 * (size_t)i + 2] = p[2];
}

__global__ __launch_bounds__(kPbBlock) void k_probe_shade(sh::Grid g, const float *__restrict__ coef, uint32_t n, const float *__restrict__ points,
                                                        const float *__restrict__ normals, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const size_t q = 3 * (size_t)i;
    const float p[3] = {points[q], points[q + 1], points[q + 2]}, nr[3] = {normals[q], normals[q + 1], normals[q + 2]};
    float e[3];
    sh::probe_shade(g, coef, p, nr, e);
    out[q] = e[0];
    out[q + 1] = e[1];
    out[q + 2] = e[2];
}

// The whole-sphere first rays of probes i0 .. i0 + m - 1, samples k_first .. k_first + kc - 1 (absolute), probe-major into the staging.
__global__ __launch_bounds__(kPbBlock) void k_probe_depth_rays(const float *__restrict__ origins, uint32_t seed, uint32_t i0, uint32_t kc, uint32_t k_first,
                                                             uint32_t n, float4 *__restrict__ ray_o, float4 *__restrict__ ray_d) {
    const uint32_t g = blockIdx.x * kPbBlock + threadIdx.x;
    if (g >= n) return;
    const uint32_t pi = g / kc, s = g - pi * kc;
    f3 pos, dir;
    sensor_ray(SensorConst{origins, nullptr, kSensorSphere}, seed, i0 + pi, k_first + s, pos, dir);
    ray_o[g] = make_float4(pos.x, pos.y, pos.z, 0.f);
    ray_d[g] = make_float4(dir.x, dir.y, dir.z, INFINITY);
}

MCPT_DI float lane_read(float v, uint32_t lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane)); }

// load: the sums and counts of these probes continue what the buffers hold (accumulate, or a later chunk of one probe's samples).
__global__ __launch_bounds__(kPbBlock) void k_probe_depth_fold(DevScene S, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                             const uint4 *__restrict__ hit, uint32_t i0, uint32_t m, uint32_t kc, int load,
                                                             float max_distance, float *__restrict__ moments, int32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pi = blockIdx.x * (kPbBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pi >= m) return;  // (wave-uniform)
    const size_t i = (size_t)i0 + pi;
    float c[3];
    pd::texel_dir((int32_t)lane, c);
    float *dst = moments + (i * (size_t)pd::kTexels + lane) * 3;
    float W = 0.f, S1 = 0.f, S2 = 0.f;
    if (load) {
        W = dst[0];
        S1 = dst[1];
        S2 = dst[2];
    }
    const size_t base = (size_t)pi * kc;
    uint32_t back = 0;
    for (uint32_t kb = 0; kb < kc; kb += 64u) {
        const uint32_t cnt = kc - kb < 64u ? kc - kb : 64u;
        float dx = 0.f, dy = 0.f, dz = 0.f, r = max_distance;
        bool bf = false;
        if (lane < cnt) {
            const size_t g = base + kb + lane;
            const uint4 h = hit[g];
            const float4 d4 = ray_d[g];
            dx = d4.x, dy = d4.y, dz = d4.z;
            const int32_t prim = (int32_t)h.z;
            if (prim >= 0) {
                const double t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
                f3 nrm;
                if (prim < S.n_tri) {
                    const float4 q = *reinterpret_cast<const float4 *>(S.tri_shade + prim);  // {n.xyz, mat}
                    nrm = mk3(q.x, q.y, q.z);
                } else {
                    const float4 sp = *reinterpret_cast<const float4 *>(S.spheres + (prim - S.n_tri));  // {c.xyz, radius}
                    const float4 o4 = ray_o[g];
                    const f3 p = mk3(o4.x, o4.y, o4.z) + mk3(dx, dy, dz) * (float)t;
                    nrm = normalized(p - mk3(sp.x, sp.y, sp.z));
                }
                r = fminf((float)t, max_distance);
                bf = dot(nrm, mk3(dx, dy, dz)) > 0.f;
            }
        }
        back += (uint32_t)__popcll(__ballot(bf));
        for (uint32_t s = 0; s < cnt; ++s) {  // (a uniform bound: the tail of a short block is not walked)
            const float d[3] = {lane_read(dx, s), lane_read(dy, s), lane_read(dz, s)};
            pd::fold_sample(pd::fold_weight(c, d), lane_read(r, s), W, S1, S2);
        }
    }
    dst[0] = W;
    dst[1] = S1;
    dst[2] = S2;
    if (lane == 0) {
        int32_t *cn = counts + 2 * i;
        const int32_t n0 = load ? cn[0] : 0, b0 = load ? cn[1] : 0;
        cn[0] = n0 + (int32_t)kc;
        cn[1] = b0 + (int32_t)back;
    }
}

__global__ __launch_bounds__(kPbBlock) void k_probe_shade_visible(sh::Grid g, const float *__restrict__ coef, const float *__restrict__ moments,
                                                                const int32_t *__restrict__ counts, float normal_bias, float backface_max, uint32_t n,
                                                                const float *__restrict__ points, const float *__restrict__ normals,
                                                                float *__restrict__ out, float *__restrict__ weight_out) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const size_t q = 3 * (size_t)i;
    const float p[3] = {points[q], points[q + 1], points[q + 2]}, nr[3] = {normals[q], normals[q + 1], normals[q + 2]};
    float e[3], A;
    pd::shade_visible(g, coef, moments, counts, normal_bias, backface_max, p, nr, e, &A);
    out[q] = e[0];
    out[q + 1] = e[1];
    out[q + 2] = e[2];
    if (weight_out) weight_out[i] = A;
}

inline uint32_t probe_blocks(uint32_t n) { return (n + kPbBlock - 1) / kPbBlock; }

// The grid of a call, or the reason it is refused.
int check_grid(const std::string &w, const mcpt_probe_grid *grid, sh::Grid &g) {
    if (!grid) return fail(MCPT_ERR_ARG, w + ": null grid");
    if (grid->reserved[0] || grid->reserved[1] || grid->reserved[2]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = grid->origin[a];
        g.spacing[a] = grid->spacing[a];
        g.dims[a] = grid->dims[a];
        if (grid->dims[a] < 1) return fail(MCPT_ERR_ARG, w + ": every member of dims must be >= 1");
        if (!(grid->spacing[a] > 0.f) || !std::isfinite(grid->spacing[a])) return fail(MCPT_ERR_ARG, w + ": spacing must be positive and finite");
        n *= (int64_t)grid->dims[a];
        if (n > (int64_t)sh::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 27 probes");
    }
    return MCPT_OK;
}

int64_t grid_probes(const sh::Grid &g) { return (int64_t)g.dims[0] * g.dims[1] * g.dims[2]; }

// The refusals of mcpt_query_probes that depend on the parameters alone; mcpt_bake_probe_grid makes them before it touches the device.
int check_probe_params(const std::string &w, const mcpt_params &p, bool variance) {
    if (p.nranks > 1 || p.rank != 0) return fail(MCPT_ERR_ARG, w + ": nranks must be 1 and rank 0 (probes are not partitioned)");
    if (p.spp <= 0 || p.n_dir_sample <= 0 || !(p.rr_rate > 0.f)) return fail(MCPT_ERR_ARG, w + ": spp/n_dir_sample/rr_rate must be positive");
    if (variance && (p.spp < 2 || p.accumulate != 0 || p.spp_total != 0 || p.sample_offset != 0))
        return fail(MCPT_ERR_ARG, w + ": variance needs spp >= 2 and accumulate, spp_total and sample_offset 0");
    return MCPT_OK;
}

// A scene-owned buffer of at least n floats.  Enlarging frees the old allocation, which kernels of an earlier call enqueued on another
// stream may still be reading: wait on the host for the scene's last recorded query first.
hipError_t probe_grow(mcpt_scene *sc, DevBuf<float> &b, size_t n) {
    if (b.p && b.n >= n) return hipSuccess;
    const hipError_t e = query_settle(sc);
    if (e != hipSuccess) return e;
    sc->probes.allocations++;
    return b.alloc(n);
}

// The refusals of mcpt_query_probe_depth that depend on the parameters alone.
int check_depth_params(const std::string &w, const mcpt_probe_depth_params *p) {
    if (!p) return fail(MCPT_ERR_ARG, w + ": null depth params");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (p->spp <= 0 || p->sample_offset < 0 || (int64_t)p->sample_offset + (int64_t)p->spp > 0x7fffffff)
        return fail(MCPT_ERR_ARG, w + ": spp must be positive, sample_offset >= 0 and sample_offset + spp at most 2^31 - 1 (the int32 counts)");
    if (p->accumulate != 0 && p->accumulate != 1) return fail(MCPT_ERR_ARG, w + ": accumulate must be 0 or 1");
    if (!(p->max_distance > 0.f) || !std::isfinite(p->max_distance)) return fail(MCPT_ERR_ARG, w + ": max_distance must be positive and finite");
    return MCPT_OK;
}

int check_visibility(const std::string &w, const mcpt_probe_visibility *o) {
    if (!o) return fail(MCPT_ERR_ARG, w + ": null visibility options");
    if (o->reserved[0] || o->reserved[1]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (!(o->normal_bias >= 0.f) || !std::isfinite(o->normal_bias) || !(o->backface_max >= 0.f) || !std::isfinite(o->backface_max))
        return fail(MCPT_ERR_ARG, w + ": normal_bias and backface_max must be finite and not negative");
    return MCPT_OK;
}

}  // namespace
}  // namespace mcpt

extern "C" {

int mcpt_query_probes(mcpt_scene *sc, const mcpt_params *pp, int64_t n, const float *origins, const mcpt_probe_outputs *out, void *hip_stream,
                      mcpt_stats *stats) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_query_probes: ") + what); };
    if (!sc) return bad("null scene");
    if (!pp || !out) return bad("null params or out");
    const mcpt_params &p = *pp;
    if (n < 0 || n > (int64_t)sh::kMaxProbes) return bad("n must be in 0 .. (2^31 - 1) / 27");
    if (out->reserved) return bad("the reserved word must be null");
    const int pc = check_probe_params("mcpt_query_probes", p, out->variance != nullptr);
    if (pc != MCPT_OK) return pc;
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof *stats);
        return MCPT_OK;
    }
    if (!origins || !out->sh) return bad("null origins or sh");
    if (!on_device(origins, sc->device) || !on_device(out->sh, sc->device) || (out->radiance && !on_device(out->radiance, sc->device)) ||
        (out->variance && !on_device(out->variance, sc->device)))
        return bad("origins, sh, radiance and variance must be memory of the scene's device");
    float *radiance = out->radiance;
    if (!radiance) {  // the plain fold still runs: the scene's own buffer takes its place (with accumulate its content means nothing)
        HIP_TRY(hipSetDevice(sc->device));
        HIP_TRY(probe_grow(sc, sc->probes.radiance, (size_t)n * 3));
        radiance = sc->probes.radiance.p;
    }
    return sensor_radiance(sc, p, (uint32_t)n, SensorConst{origins, nullptr, kSensorSphere}, radiance, out->variance, out->sh, (hipStream_t)hip_stream, stats);
}

int mcpt_probe_rays(mcpt_scene *sc, uint32_t seed, int64_t n, const float *origins, const uint32_t *sensor, const uint32_t *sample, float *origins_out,
                    float *dirs_out) {
    if (!sc || n < 0 || (n > 0 && (!origins || !sensor || !sample || !origins_out || !dirs_out))) return fail(MCPT_ERR_ARG, "mcpt_probe_rays: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_probe_rays: too many rays for one call");
    size_t m = 0;  // the probes the pairs name: rows 0 .. max(sensor) of origins
    for (int64_t j = 0; j < n; ++j) m = std::max<size_t>(m, (size_t)sensor[j] + 1);
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> dPo;
    DevBuf<uint32_t> dI, dS;
    DevBuf<float4> dO, dD;
    HIP_TRY(dO.alloc(n));
    HIP_TRY(dD.alloc(n));
    HIP_TRY(upload(dPo, origins, m * 3));
    HIP_TRY(upload(dI, sensor, n));
    HIP_TRY(upload(dS, sample, n));
    launch_sensor_rays(SensorConst{dPo.p, nullptr, kSensorSphere}, seed, (uint32_t)n, dI.p, dS.p, dO.p, dD.p, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<float4> o(n), d(n);
    HIP_TRY(download(o.data(), dO, n));
    HIP_TRY(download(d.data(), dD, n));
    for (int64_t j = 0; j < n; ++j) {
        origins_out[3 * j] = o[j].x, origins_out[3 * j + 1] = o[j].y, origins_out[3 * j + 2] = o[j].z;
        dirs_out[3 * j] = d[j].x, dirs_out[3 * j + 1] = d[j].y, dirs_out[3 * j + 2] = d[j].z;
    }
    return MCPT_OK;
}

int mcpt_probe_shade(mcpt_scene *sc, const mcpt_probe_grid *grid, const float *coef, int64_t n, const float *points, const float *normals, float *out,
                     void *hip_stream) {
    const std::string w = "mcpt_probe_shade";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (n < 0 || n > 0x7fffffff / 3) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 3");
    if (n == 0) return MCPT_OK;
    if (!coef || !points || !normals || !out) return fail(MCPT_ERR_ARG, w + ": null sh, points, normals or out");
    if (!on_device(coef, sc->device) || !on_device(points, sc->device) || !on_device(normals, sc->device) || !on_device(out, sc->device))
        return fail(MCPT_ERR_ARG, w + ": sh, points, normals and out must be memory of the scene's device");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_probe_shade, dim3(probe_blocks((uint32_t)n)), dim3(kPbBlock), 0, (hipStream_t)hip_stream, g, coef, (uint32_t)n, points, normals, out);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_bake_probe_grid(mcpt_scene *sc, const mcpt_probe_grid *grid, const mcpt_params *pp, float *coef, void *hip_stream, mcpt_stats *stats) {
    const std::string w = "mcpt_bake_probe_grid";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (!pp || !coef) return fail(MCPT_ERR_ARG, w + ": null params or sh");
    const int pc = check_probe_params(w, *pp, false);
    if (pc != MCPT_OK) return pc;
    if (!on_device(coef, sc->device)) return fail(MCPT_ERR_ARG, w + ": sh must be memory of the scene's device");
    const uint32_t n = (uint32_t)grid_probes(g);
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    HIP_TRY(probe_grow(sc, sc->probes.points, (size_t)n * 3));
    hipLaunchKernelGGL(k_probe_grid_points, dim3(probe_blocks(n)), dim3(kPbBlock), 0, (hipStream_t)hip_stream, g, n, sc->probes.points.p);
    HIP_TRY(hipGetLastError());
    const mcpt_probe_outputs out{coef, nullptr, nullptr, nullptr};
    return mcpt_query_probes(sc, pp, n, sc->probes.points.p, &out, hip_stream, stats);
}

int mcpt_query_probe_depth(mcpt_scene *sc, const mcpt_probe_depth_params *pp, int64_t n, const float *origins, float *moments, int32_t *counts,
                           void *hip_stream, mcpt_query_info *info) {
    const std::string w = "mcpt_query_probe_depth";
    if (info) std::memset(info, 0, sizeof *info);
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    const int pc = check_depth_params(w, pp);
    if (pc != MCPT_OK) return pc;
    if (n < 0 || n > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 192");
    if (n == 0) return MCPT_OK;
    if (!origins || !moments || !counts) return fail(MCPT_ERR_ARG, w + ": null origins, moments or counts");
    if (!on_device(origins, sc->device) || !on_device(moments, sc->device) || !on_device(counts, sc->device))
        return fail(MCPT_ERR_ARG, w + ": origins, moments and counts must be memory of the scene's device");
    const mcpt_probe_depth_params &p = *pp;
    const hipStream_t st = (hipStream_t)hip_stream;
    mcpt_query_info qi;
    std::memset(&qi, 0, sizeof qi);
    HIP_TRY(hipSetDevice(sc->device));
    // A chunk holds whole probes when a probe's samples fit it (their sums never leave the registers), else whole 64-sample blocks of one
    // probe (the sums pass through `moments` between launches).  Either way a texel's additions run in sample order.
    const uint64_t chunk = std::max<uint32_t>(sc->knobs.query_chunk, 64u);
    const uint64_t spp = (uint64_t)p.spp;
    const bool whole = spp <= chunk;
    const uint64_t per = whole ? std::min<uint64_t>((uint64_t)n, chunk / spp) : 1;  // probes per launch
    const uint64_t kmax = whole ? spp : chunk / 64 * 64;                               // samples of a probe per launch
    RetryList rl;
    const int sr = query_stage(sc, (uint32_t)(per * kmax), st, qi, rl);
    if (sr != MCPT_OK) return sr;
    QueryBufs &Q = sc->query;
    for (uint64_t i0 = 0; i0 < (uint64_t)n; i0 += per) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(per, (uint64_t)n - i0);
        for (uint64_t k0 = 0; k0 < spp; k0 += kmax) {
            const uint32_t kc = (uint32_t)std::min<uint64_t>(kmax, spp - k0), rays = m * kc;
            hipLaunchKernelGGL(k_probe_depth_rays, dim3(probe_blocks(rays)), dim3(kPbBlock), 0, st, origins, p.seed, (uint32_t)i0, kc,
                               (uint32_t)p.sample_offset + (uint32_t)k0, rays, Q.ray_o.p, Q.ray_d.p);
            launch_trace_closest(sc->view, rays, nullptr, Q.ray_o.p, Q.ray_d.p, Q.hit.p, rl, st);
            hipLaunchKernelGGL(k_probe_depth_fold, dim3((m + kPbBlock / 64 - 1) / (kPbBlock / 64)), dim3(kPbBlock), 0, st, sc->view, Q.ray_o.p, Q.ray_d.p, Q.hit.p,
                               (uint32_t)i0, m, kc, (p.accumulate || k0 > 0) ? 1 : 0, p.max_distance, moments, counts);
            qi.launches++;
        }
    }
    const int fr = query_finish(sc, st, qi);
    if (fr != MCPT_OK) return fr;
    if (info) *info = qi;
    return MCPT_OK;
}

int mcpt_probe_shade_visible(mcpt_scene *sc, const mcpt_probe_grid *grid, const float *coef, const float *moments, const int32_t *counts,
                             const mcpt_probe_visibility *opts, int64_t n, const float *points, const float *normals, float *out, float *weight_out,
                             void *hip_stream) {
    const std::string w = "mcpt_probe_shade_visible";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (grid_probes(g) > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 192 probes");
    const int vc = check_visibility(w, opts);
    if (vc != MCPT_OK) return vc;
    if (n < 0 || n > 0x7fffffff / 3) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 3");
    if (n == 0) return MCPT_OK;
    if (!coef || !moments || !counts || !points || !normals || !out) return fail(MCPT_ERR_ARG, w + ": null sh, moments, counts, points, normals or out");
    if (!on_device(coef, sc->device) || !on_device(moments, sc->device) || !on_device(counts, sc->device) || !on_device(points, sc->device) ||
        !on_device(normals, sc->device) || !on_device(out, sc->device) || (weight_out && !on_device(weight_out, sc->device)))
        return fail(MCPT_ERR_ARG, w + ": sh, moments, counts, points, normals, out and weight_out must be memory of the scene's device");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_probe_shade_visible, dim3(probe_blocks((uint32_t)n)), dim3(kPbBlock), 0, (hipStream_t)hip_stream, g, coef, moments, counts,
                       opts->normal_bias, opts->backface_max, (uint32_t)n, points, normals, out, weight_out);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_bake_probe_volume(mcpt_scene *sc, const mcpt_probe_grid *grid, const mcpt_params *pp, const mcpt_probe_depth_params *dp, float *coef,
                           float *moments, int32_t *counts, void *hip_stream, mcpt_stats *stats) {
    const std::string w = "mcpt_bake_probe_volume";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (grid_probes(g) > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 192 probes");
    if (!pp || !coef || !moments || !counts) return fail(MCPT_ERR_ARG, w + ": null params, sh, moments or counts");
    const int pc = check_probe_params(w, *pp, false);
    if (pc != MCPT_OK) return pc;
    const int dc = check_depth_params(w, dp);
    if (dc != MCPT_OK) return dc;
    if (!on_device(coef, sc->device) || !on_device(moments, sc->device) || !on_device(counts, sc->device))
        return fail(MCPT_ERR_ARG, w + ": sh, moments and counts must be memory of the scene's device");
    const int rc = mcpt_bake_probe_grid(sc, grid, pp, coef, hip_stream, stats);
    if (rc != MCPT_OK) return rc;
    return mcpt_query_probe_depth(sc, dp, grid_probes(g), sc->probes.points.p, moments, counts, hip_stream, nullptr);
}

int mcpt_scene_probe_buffers(const mcpt_scene *sc, int64_t *floats, int64_t *allocations) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_probe_buffers: null scene");
    if (floats) *floats = (int64_t)(sc->probes.points.n + sc->probes.radiance.n);
    if (allocations) *allocations = sc->probes.allocations;
    return MCPT_OK;
}

int mcpt_sh_basis_host(int64_t n, const float *dirs, float *basis) {
    if (n < 0 || (n > 0 && (!dirs || !basis))) return fail(MCPT_ERR_ARG, "mcpt_sh_basis_host: n < 0, or null dirs or basis");
    for (int64_t i = 0; i < n; ++i) sh::sh9_basis(dirs + 3 * i, basis + 9 * i);
    return MCPT_OK;
}

int mcpt_sh_irradiance_host(int64_t n, const float *coef, const float *normals, float *out) {
    if (n < 0 || (n > 0 && (!coef || !normals || !out))) return fail(MCPT_ERR_ARG, "mcpt_sh_irradiance_host: n < 0, or null sh, normals or out");
    for (int64_t i = 0; i < n; ++i) sh::sh9_irradiance(coef + 27 * i, normals + 3 * i, out + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_grid_points_host(const mcpt_probe_grid *grid, float *points) {
    const std::string w = "mcpt_probe_grid_points_host";
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (!points) return fail(MCPT_ERR_ARG, w + ": null points");
    size_t i = 0;
    for (int32_t iz = 0; iz < g.dims[2]; ++iz)
        for (int32_t iy = 0; iy < g.dims[1]; ++iy)
            for (int32_t ix = 0; ix < g.dims[0]; ++ix, ++i) sh::grid_point(g, ix, iy, iz, points + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_shade_host(const mcpt_probe_grid *grid, const float *coef, int64_t n, const float *points, const float *normals, float *out) {
    const std::string w = "mcpt_probe_shade_host";
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (n < 0 || (n > 0 && (!coef || !points || !normals || !out))) return fail(MCPT_ERR_ARG, w + ": n < 0, or null sh, points, normals or out");
    for (int64_t i = 0; i < n; ++i) sh::probe_shade(g, coef, points + 3 * i, normals + 3 * i, out + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_depth_dirs_host(float *dirs) {
    if (!dirs) return fail(MCPT_ERR_ARG, "mcpt_probe_depth_dirs_host: null dirs");
    for (int32_t j = 0; j < pd::kTexels; ++j) pd::texel_dir(j, dirs + 3 * j);
    return MCPT_OK;
}

int mcpt_probe_depth_texel_host(int64_t n, const float *v, int32_t *texel) {
    if (n < 0 || (n > 0 && (!v || !texel))) return fail(MCPT_ERR_ARG, "mcpt_probe_depth_texel_host: n < 0, or null v or texel");
    for (int64_t i = 0; i < n; ++i) texel[i] = pd::texel_of(v + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_depth_fold_host(int64_t n, int32_t spp, const float *dirs, const float *r, const uint8_t *backfacing, int32_t accumulate, float *moments,
                               int32_t *counts) {
    const std::string w = "mcpt_probe_depth_fold_host";
    if (n < 0 || n > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 192");
    if (spp <= 0) return fail(MCPT_ERR_ARG, w + ": spp must be positive");
    if (accumulate != 0 && accumulate != 1) return fail(MCPT_ERR_ARG, w + ": accumulate must be 0 or 1");
    if (n > 0 && (!dirs || !r || !backfacing || !moments || !counts)) return fail(MCPT_ERR_ARG, w + ": null dirs, r, backfacing, moments or counts");
    if (accumulate)
        for (int64_t i = 0; i < n; ++i)
            if (counts[2 * i] < 0 || (int64_t)counts[2 * i] + spp > 0x7fffffff) return fail(MCPT_ERR_ARG, w + ": spp does not fit the int32 counts together with the existing ones");
    float c[pd::kTexels][3];
    for (int32_t j = 0; j < pd::kTexels; ++j) pd::texel_dir(j, c[j]);
    for (int64_t i = 0; i < n; ++i) {
        const size_t s0 = (size_t)i * (size_t)spp;
        for (int32_t j = 0; j < pd::kTexels; ++j) {
            float *m3 = moments + ((size_t)i * pd::kTexels + j) * 3;
            float W = accumulate ? m3[0] : 0.f, S1 = accumulate ? m3[1] : 0.f, S2 = accumulate ? m3[2] : 0.f;
            for (int32_t k = 0; k < spp; ++k) pd::fold_sample(pd::fold_weight(c[j], dirs + 3 * (s0 + k)), r[s0 + k], W, S1, S2);
            m3[0] = W;
            m3[1] = S1;
            m3[2] = S2;
        }
        int32_t back = 0;
        for (int32_t k = 0; k < spp; ++k) back += backfacing[s0 + k] ? 1 : 0;
        counts[2 * i] = (accumulate ? counts[2 * i] : 0) + spp;
        counts[2 * i + 1] = (accumulate ? counts[2 * i + 1] : 0) + back;
    }
    return MCPT_OK;
}

int mcpt_probe_shade_visible_host(const mcpt_probe_grid *grid, const float *coef, const float *moments, const int32_t *counts,
                                  const mcpt_probe_visibility *opts, int64_t n, const float *points, const float *normals, float *out, float *weight_out) {
    const std::string w = "mcpt_probe_shade_visible_host";
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (grid_probes(g) > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 192 probes");
    const int vc = check_visibility(w, opts);
    if (vc != MCPT_OK) return vc;
    if (n < 0 || (n > 0 && (!coef || !moments || !counts || !points || !normals || !out)))
        return fail(MCPT_ERR_ARG, w + ": n < 0, or null sh, moments, counts, points, normals or out");
    for (int64_t i = 0; i < n; ++i)
        pd::shade_visible(g, coef, moments, counts, opts->normal_bias, opts->backface_max, points + 3 * i, normals + 3 * i, out + 3 * i,
                          weight_out ? weight_out + i : nullptr);
    return MCPT_OK;
}

}  // extern "C"
