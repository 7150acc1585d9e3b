// Light probes (include/mcpt.h: mcpt_query_probes, mcpt_probe_rays, mcpt_probe_shade, mcpt_bake_probe_grid and the host-only
// mcpt_sh_basis_host / mcpt_sh_irradiance_host / mcpt_probe_grid_points_host / mcpt_probe_shade_host).  csrc/mcpt_sh.h states the rule --
// basis, irradiance, grid lookup -- once; the whole-sphere first ray is sensor_ray's third branch (csrc/mcpt_sensor.h) and the projection
// fold k_accumulate_sh sits beside k_accumulate (csrc/mcpt_kernels.hip), launched by render_list at both of its accumulate sites.
//
// Kernels here, on the caller's stream:
//   k_probe_grid_points  one lane per probe: sh::grid_point into the scene-owned point buffer (mcpt_bake_probe_grid)
//   k_probe_shade        one lane per (point, normal): sh::probe_shade from the coefficient buffer; eight 108-byte rows are read per lane
// Every store is a plain vector store; nothing here uses LDS, scratch or inline assembly.
#include <cmath>

#include "mcpt_frame.h"
#include "mcpt_host.h"
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

}  // extern "C"
