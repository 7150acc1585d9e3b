// Lightmap baking (include/mcpt.h: mcpt_lightmap_texels, mcpt_lightmap_scatter, mcpt_bake_lightmap, and the host-only
// mcpt_lightmap_texels_host / mcpt_lightmap_dilate_host).  csrc/mcpt_lightmap.h states the rule -- coverage, sensor, dilation -- once;
// the kernels and the host loops below only decide WHICH (triangle, texel) pairs that rule is asked about, and in what order.
//
// Texels of one object, all on the caller's stream, reading the live TriShade / TriGeom records:
//   k_lm_count     one lane per triangle: the 8 x 8-texel tiles its chart's bounding box touches (lm::tile_box), 0 for a chart that is
//                  degenerate, not finite or off the map; one extra lane writes the 0 that makes the scan's last entry the total
//   hipcub scan    exclusive sum of the counts (64-bit); the host reads the total: the number of (triangle, tile) items
//   k_lm_fill      owner plane = lm::kNoOwner
//   k_lm_raster    one WAVE per item, found by a wave-uniform bisection of the scan (scalar loads); lane = texel of the tile; lm::cover;
//                  atomicMin of the global primitive id into the owner plane.  A large triangle is spread over as many waves as it has
//                  tiles, a mesh of tiny triangles costs a wave or two per triangle.  At most kLmChunk items per launch.
//   hipcub select  the texels with an owner, in texel order, straight into the caller's `texel`; the host reads the count n
//   k_lm_resolve   one lane per sensor: the owner's barycentrics again (lm::cover), prim, bary, origin (lm::point) and normal
// Scatter:
//   k_lm_scatter   image[texel[i]] = values[i], coverage 1 (both planes cleared first)
//   k_lm_dilate    one lane per texel, lm::dilate_texel from one plane into the other; the first plane is chosen so that the last round
//                  ends in the caller's image
// Every store is a plain vector store; nothing here uses LDS, scratch or inline assembly.
#include <hipcub/hipcub.hpp>

#include <climits>

#include "mcpt_host.h"
#include "mcpt_lightmap.h"
#include "mcpt_move.h"

using namespace mcpt;

namespace mcpt {

namespace {

constexpr int kLmBlock = 256;                // 4 waves
constexpr int kLmWaves = kLmBlock / 64;
constexpr uint64_t kLmChunk = 1ull << 24;    // items per launch of k_lm_raster: 2^22 workgroups

inline uint32_t lm_blocks(uint64_t n) { return (uint32_t)((n + kLmBlock - 1) / kLmBlock); }

__global__ __launch_bounds__(kLmBlock) void k_lm_count(const TriShade *__restrict__ shade, int32_t n_tri, int32_t W, int32_t H,
                                                       unsigned long long *__restrict__ counts) {
    const uint32_t k = blockIdx.x * kLmBlock + threadIdx.x;
    if (k > (uint32_t)n_tri) return;
    unsigned long long c = 0;
    if (k < (uint32_t)n_tri) {
        int32_t tx0, ty0, ntx, nty;
        lm::tile_box(shade[k], W, H, tx0, ty0, ntx, nty);
        c = (unsigned long long)ntx * (unsigned long long)nty;
    }
    counts[k] = c;
}

__global__ __launch_bounds__(kLmBlock) void k_lm_fill(int32_t *__restrict__ owner, uint32_t n) {
    const uint32_t t = blockIdx.x * kLmBlock + threadIdx.x;
    if (t < n) owner[t] = lm::kNoOwner;
}

// scan: n_tri + 1 entries, scan[n_tri] = the number of items.  Items [base, end) belong to this launch.
__global__ __launch_bounds__(kLmBlock) void k_lm_raster(const TriShade *__restrict__ shade, int32_t first_tri, int32_t n_tri, int32_t W, int32_t H,
                                                        const unsigned long long *__restrict__ scan, unsigned long long base, unsigned long long end,
                                                        int32_t *__restrict__ owner) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: the bisection below runs on scalar loads
    const unsigned long long item = base + (unsigned long long)blockIdx.x * kLmWaves + wave;
    if (item >= end) return;
    // the last triangle whose first item is <= item (triangles without items share their successor's entry and are passed over)
    int32_t lo = 0, hi = n_tri - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        if (scan[mid] <= item) lo = mid;
        else hi = mid - 1;
    }
    const TriShade s = shade[lo];
    int32_t tx0, ty0, ntx, nty;
    lm::tile_box(s, W, H, tx0, ty0, ntx, nty);
    const unsigned long long local = item - scan[lo];
    if (ntx <= 0 || local >= (unsigned long long)ntx * (unsigned long long)nty) return;  // (cannot happen: the counts came from tile_box)
    const int32_t x = (tx0 + (int32_t)(local % (unsigned long long)ntx)) * lm::kTile + (lane & 7);
    const int32_t y = (ty0 + (int32_t)(local / (unsigned long long)ntx)) * lm::kTile + (lane >> 3);
    if (x >= W || y >= H) return;  // a tile cut by the map's edge
    double w1, w2;
    if (lm::cover(s, x, y, W, H, w1, w2)) atomicMin(owner + ((size_t)y * (size_t)W + (size_t)x), first_tri + lo);
}

struct LmOwned {
    __host__ __device__ __forceinline__ uint8_t operator()(const int32_t &o) const { return o != lm::kNoOwner ? 1 : 0; }
};

struct LmOut {
    int32_t *prim;
    float *bary, *origins, *normals;
};

__global__ __launch_bounds__(kLmBlock) void k_lm_resolve(const TriGeom *__restrict__ geom, const TriShade *__restrict__ shade, int32_t W, int32_t H,
                                                         int32_t flip, uint32_t n, const int32_t *__restrict__ texel,
                                                         const int32_t *__restrict__ owner, LmOut out) {
    const uint32_t i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t t = texel[i];
    const int32_t prim = owner[t];
    const TriShade s = shade[prim];
    double w1, w2;
    (void)lm::cover(s, t % W, t / W, W, H, w1, w2);  // (the test that made prim the owner: it succeeds again)
    const float u = (float)w1, v = (float)w2;
    if (out.prim) out.prim[i] = prim;
    if (out.bary) {
        out.bary[2 * (size_t)i] = u;
        out.bary[2 * (size_t)i + 1] = v;
    }
    if (out.origins) {
        float p[3];
        lm::point(geom[prim], u, v, p);
        out.origins[3 * (size_t)i] = p[0];
        out.origins[3 * (size_t)i + 1] = p[1];
        out.origins[3 * (size_t)i + 2] = p[2];
    }
    if (out.normals) {
        out.normals[3 * (size_t)i] = flip ? -s.n[0] : s.n[0];
        out.normals[3 * (size_t)i + 1] = flip ? -s.n[1] : s.n[1];
        out.normals[3 * (size_t)i + 2] = flip ? -s.n[2] : s.n[2];
    }
}

__global__ __launch_bounds__(kLmBlock) void k_lm_scatter(uint32_t n, const int32_t *__restrict__ texel, const float *__restrict__ values, uint32_t n_texels,
                                                         float *__restrict__ image, uint8_t *__restrict__ coverage) {
    const uint32_t i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = (uint32_t)texel[i];
    if (t >= n_texels) return;  // (the list is the caller's: an index off the map is ignored)
    image[3 * (size_t)t] = values[3 * (size_t)i];
    image[3 * (size_t)t + 1] = values[3 * (size_t)i + 1];
    image[3 * (size_t)t + 2] = values[3 * (size_t)i + 2];
    if (coverage) coverage[t] = 1;
}

__global__ __launch_bounds__(kLmBlock) void k_lm_dilate(int32_t W, int32_t H, const float *__restrict__ img, const uint8_t *__restrict__ cov,
                                                        float *__restrict__ img_out, uint8_t *__restrict__ cov_out) {
    const uint32_t t = blockIdx.x * kLmBlock + threadIdx.x;
    if (t >= (uint32_t)W * (uint32_t)H) return;
    float v[3];
    uint8_t c;
    lm::dilate_texel(W, H, (int32_t)(t % (uint32_t)W), (int32_t)(t / (uint32_t)W), img, cov, v, c);
    img_out[3 * (size_t)t] = v[0];
    img_out[3 * (size_t)t + 1] = v[1];
    img_out[3 * (size_t)t + 2] = v[2];
    cov_out[t] = c;
}

// ---- host side

// A scene-owned buffer of at least n entries.  Enlarging frees the old one, which an earlier call's kernels may still read: settle first.
template <typename T>
hipError_t lm_grow(mcpt_scene *sc, DevBuf<T> &b, size_t n) {
    if (b.p && b.n >= n) return hipSuccess;
    hipError_t e = query_settle(sc);
    if (e != hipSuccess) return e;
    sc->lightmap.grew = true;
    return b.alloc(n);
}

// Behind everything a call enqueued, even when a launch failed: whatever was enqueued still reads the scene (run_query, csrc/mcpt_rayquery.hip).
hipError_t lm_record(mcpt_scene *sc, hipStream_t st) {
    const hipError_t e = hipEventRecord(sc->query.done, st);
    if (e == hipSuccess) {
        sc->query.pending = true;
        sc->query.last_stream = st;
    }
    return e;
}

// Before a call touches the scene-owned buffers: the device is current, the event exists, and a call still running on another stream
// has finished with them (a buffer enlarged afterwards settles that call on the host instead: lm_grow).
int lm_begin(mcpt_scene *sc, hipStream_t st) {
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();  // an earlier, already reported failure of this thread must not be taken for one of this call
    QueryBufs &Q = sc->query;
    if (!Q.done.e) HIP_TRY(Q.done.create());
    if (Q.pending && st != Q.last_stream) HIP_TRY(hipStreamWaitEvent(st, Q.done, 0));
    return MCPT_OK;
}

// The checks every call shares, before any device work.
int lm_check(const std::string &w, const mcpt_scene *sc, const mcpt_lightmap_desc *d) {
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    if (!d) return fail(MCPT_ERR_ARG, w + ": null desc");
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (d->width < 1 || d->height < 1 || (int64_t)d->width * (int64_t)d->height > (int64_t)lm::kMaxTexels)
        return fail(MCPT_ERR_ARG, w + ": width and height must be >= 1 and width*height <= (2^31 - 1) / 3");
    if (d->object < 0 || (size_t)d->object >= sc->src.objects.size()) return fail(MCPT_ERR_ARG, w + ": object out of range");
    if (sc->src.objects[d->object].kind != MCPT_OBJ_MESH) return fail(MCPT_ERR_ARG, w + ": the object is a sphere (no UV chart)");
    if (sc->meta.n_instances > 0) return fail(MCPT_ERR_ARG, w + ": the scene is instanced");
    if (sc->src.objects[d->object].n_tri == INT_MAX) return fail(MCPT_ERR_ARG, w + ": too many triangles");
    return MCPT_OK;
}

size_t lm_temp_bytes(int32_t n_scan, int32_t n_texels) {
    size_t a = 0, b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, n_scan);
    (void)hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<int32_t>(0),
                                        hipcub::TransformInputIterator<uint8_t, LmOwned, const int32_t *>(nullptr, LmOwned()), (int32_t *)nullptr,
                                        (int32_t *)nullptr, n_texels);
    return std::max(a, b);
}

// mcpt_lightmap_texels after its checks, up to the count: the covered texels of the object into `texel`, in texel order.
int lm_list_texels(mcpt_scene *sc, const mcpt_lightmap_desc &d, int32_t *texel, int64_t &n, hipStream_t st) {
    LightmapBufs &L = sc->lightmap;
    const mcpt_object &o = sc->src.objects[d.object];
    const int32_t W = d.width, H = d.height, n_texels = W * H, n_tri = o.n_tri;
    const size_t temp_bytes = lm_temp_bytes(n_tri + 1, n_texels);
    const int rc = lm_begin(sc, st);
    if (rc != MCPT_OK) return rc;
    HIP_TRY(lm_grow(sc, L.counts, (size_t)n_tri + 1));
    HIP_TRY(lm_grow(sc, L.scan, (size_t)n_tri + 1));
    HIP_TRY(lm_grow(sc, L.owner, (size_t)n_texels));
    HIP_TRY(lm_grow(sc, L.temp, temp_bytes));
    HIP_TRY(lm_grow(sc, L.n_sel, 1));
    const TriShade *shade = sc->view.tri_shade + o.first_tri;
    hipLaunchKernelGGL(k_lm_count, dim3(lm_blocks((uint64_t)n_tri + 1)), dim3(kLmBlock), 0, st, shade, n_tri, W, H, L.counts.p);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(L.temp.p, tb, (const unsigned long long *)L.counts.p, L.scan.p, n_tri + 1, st);
    hipLaunchKernelGGL(k_lm_fill, dim3(lm_blocks((uint64_t)n_texels)), dim3(kLmBlock), 0, st, L.owner.p, (uint32_t)n_texels);
    unsigned long long items = 0;
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&items, L.scan.p + n_tri, sizeof items, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)lm_record(sc, st);
        HIP_TRY(e);
    }
    L.last_items = (int64_t)items;
    for (unsigned long long base = 0; base < items; base += kLmChunk) {
        const unsigned long long end = std::min(items, base + kLmChunk);
        hipLaunchKernelGGL(k_lm_raster, dim3((uint32_t)((end - base + kLmWaves - 1) / kLmWaves)), dim3(kLmBlock), 0, st, shade, o.first_tri, n_tri, W, H,
                           (const unsigned long long *)L.scan.p, base, end, L.owner.p);
    }
    e = hipGetLastError();
    tb = temp_bytes;
    if (e == hipSuccess)
        e = hipcub::DeviceSelect::Flagged(L.temp.p, tb, hipcub::CountingInputIterator<int32_t>(0),
                                          hipcub::TransformInputIterator<uint8_t, LmOwned, const int32_t *>(L.owner.p, LmOwned()), texel, L.n_sel.p, n_texels, st);
    int32_t n_sel = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&n_sel, L.n_sel.p, sizeof n_sel, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)lm_record(sc, st);
        HIP_TRY(e);
    }
    n = n_sel;
    return MCPT_OK;
}

// ... and the rows of the n listed sensors.  Records the event: this is the last thing mcpt_lightmap_texels enqueues.
int lm_resolve(mcpt_scene *sc, const mcpt_lightmap_desc &d, int64_t n, const int32_t *texel, const LmOut &out, hipStream_t st) {
    if (n > 0 && (out.prim || out.bary || out.origins || out.normals))
        hipLaunchKernelGGL(k_lm_resolve, dim3(lm_blocks((uint64_t)n)), dim3(kLmBlock), 0, st, sc->view.tri_geom, sc->view.tri_shade, d.width, d.height,
                           d.flip_normals ? 1 : 0, (uint32_t)n, texel, (const int32_t *)sc->lightmap.owner.p, out);
    const hipError_t le = hipGetLastError(), re = lm_record(sc, st);
    HIP_TRY(le);
    HIP_TRY(re);
    return MCPT_OK;
}

// mcpt_lightmap_scatter after its checks.
int lm_scatter(mcpt_scene *sc, int32_t W, int32_t H, int64_t n, const int32_t *texel, const float *values, int32_t dilate, float *image, uint8_t *coverage,
               hipStream_t st) {
    LightmapBufs &L = sc->lightmap;
    const size_t n_texels = (size_t)W * (size_t)H;
    const int rc = lm_begin(sc, st);
    if (rc != MCPT_OK) return rc;
    if (dilate > 0) {
        HIP_TRY(lm_grow(sc, L.plane, n_texels * 3));
        HIP_TRY(lm_grow(sc, L.cov[1], n_texels));
        if (!coverage) HIP_TRY(lm_grow(sc, L.cov[0], n_texels));
    }
    if (dilate > 0 && !coverage) coverage = L.cov[0].p;
    // the planes of the ping-pong; the scatter goes to the one from which `dilate` rounds end in the caller's
    float *img[2] = {image, L.plane.p};
    uint8_t *cov[2] = {coverage, L.cov[1].p};
    int cur = dilate & 1;
    hipError_t e = hipMemsetAsync(img[cur], 0, n_texels * 3 * sizeof(float), st);
    if (e == hipSuccess && cov[cur]) e = hipMemsetAsync(cov[cur], 0, n_texels, st);
    if (e == hipSuccess) {
        if (n > 0) hipLaunchKernelGGL(k_lm_scatter, dim3(lm_blocks((uint64_t)n)), dim3(kLmBlock), 0, st, (uint32_t)n, texel, values, (uint32_t)n_texels, img[cur], cov[cur]);
        for (int32_t r = 0; r < dilate; ++r, cur ^= 1)
            hipLaunchKernelGGL(k_lm_dilate, dim3(lm_blocks((uint64_t)n_texels)), dim3(kLmBlock), 0, st, W, H, (const float *)img[cur], (const uint8_t *)cov[cur],
                               img[cur ^ 1], cov[cur ^ 1]);
        e = hipGetLastError();
    }
    const hipError_t re = lm_record(sc, st);
    HIP_TRY(e);
    HIP_TRY(re);
    return MCPT_OK;
}

bool lm_on_device(const mcpt_scene *sc, const void *p) { return !p || on_device(p, sc->device); }

}  // namespace
}  // namespace mcpt

extern "C" {

int mcpt_lightmap_texels(mcpt_scene *sc, const mcpt_lightmap_desc *d, const mcpt_lightmap_texels_out *out, int64_t *n_out, void *hip_stream) {
    const std::string w = "mcpt_lightmap_texels";
    const int c = lm_check(w, sc, d);
    if (c != MCPT_OK) return c;
    if (!out || !out->texel || !n_out) return fail(MCPT_ERR_ARG, w + ": null out, texel or n_out");
    if (!on_device(out->texel, sc->device) || !lm_on_device(sc, out->prim) || !lm_on_device(sc, out->bary) || !lm_on_device(sc, out->origins) ||
        !lm_on_device(sc, out->normals))
        return fail(MCPT_ERR_ARG, w + ": an output is not memory of the scene's device");
    hipStream_t st = (hipStream_t)hip_stream;
    int64_t n = 0;
    *n_out = 0;
    int rc = lm_list_texels(sc, *d, out->texel, n, st);
    if (rc != MCPT_OK) return rc;
    rc = lm_resolve(sc, *d, n, out->texel, LmOut{out->prim, out->bary, out->origins, out->normals}, st);
    if (rc != MCPT_OK) return rc;
    *n_out = n;
    return MCPT_OK;
}

int mcpt_lightmap_scatter(mcpt_scene *sc, const mcpt_lightmap_desc *d, int64_t n, const int32_t *texel, const float *values, int32_t dilate, float *image,
                          uint8_t *coverage, void *hip_stream) {
    const std::string w = "mcpt_lightmap_scatter";
    const int c = lm_check(w, sc, d);
    if (c != MCPT_OK) return c;
    if (dilate < 0) return fail(MCPT_ERR_ARG, w + ": dilate must be >= 0");
    if (n < 0 || n > (int64_t)d->width * d->height) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. width*height");
    if (!image || (n > 0 && (!texel || !values))) return fail(MCPT_ERR_ARG, w + ": null image, texel or values");
    if (!on_device(image, sc->device) || !lm_on_device(sc, coverage) || (n > 0 && (!on_device(texel, sc->device) || !on_device(values, sc->device))))
        return fail(MCPT_ERR_ARG, w + ": texel, values, image and coverage must be memory of the scene's device");
    return lm_scatter(sc, d->width, d->height, n, texel, values, dilate, image, coverage, (hipStream_t)hip_stream);
}

int mcpt_bake_lightmap(mcpt_scene *sc, const mcpt_lightmap_desc *d, const mcpt_params *pp, int32_t dilate, float *image, uint8_t *coverage, float *variance,
                       void *hip_stream, mcpt_lightmap_info *info, mcpt_stats *stats) {
    const std::string w = "mcpt_bake_lightmap";
    if (info) std::memset(info, 0, sizeof *info);
    const int c = lm_check(w, sc, d);
    if (c != MCPT_OK) return c;
    if (!pp || !image) return fail(MCPT_ERR_ARG, w + ": null params or image");
    const mcpt_params &p = *pp;
    if (dilate < 0) return fail(MCPT_ERR_ARG, w + ": dilate must be >= 0");
    if (p.nranks > 1 || p.rank != 0) return fail(MCPT_ERR_ARG, w + ": nranks must be 1 and rank 0");
    if (p.spp <= 0 || p.n_dir_sample <= 0 || !(p.rr_rate > 0.f)) return fail(MCPT_ERR_ARG, w + ": spp/n_dir_sample/rr_rate must be positive");
    if (p.sample_offset != 0 || p.spp_total != 0 || p.accumulate != 0)
        return fail(MCPT_ERR_ARG, w + ": sample_offset, spp_total and accumulate must be 0 (compose progressive bakes from texels, query_radiance and scatter)");
    if (variance && p.spp < 2) return fail(MCPT_ERR_ARG, w + ": variance needs spp >= 2");
    if (!on_device(image, sc->device) || !lm_on_device(sc, coverage) || !lm_on_device(sc, variance))
        return fail(MCPT_ERR_ARG, w + ": image, coverage and variance must be memory of the scene's device");
    hipStream_t st = (hipStream_t)hip_stream;
    LightmapBufs &L = sc->lightmap;
    L.grew = false;
    if (stats) std::memset(stats, 0, sizeof *stats);
    HIP_TRY(hipSetDevice(sc->device));
    Clock::time_point t0 = Clock::now();
    HIP_TRY(lm_grow(sc, L.texel, (size_t)d->width * (size_t)d->height));
    int64_t n = 0;
    int rc = lm_list_texels(sc, *d, L.texel.p, n, st);
    if (rc != MCPT_OK) return rc;
    const size_t rows = (size_t)std::max<int64_t>(n, 1) * 3;
    hipError_t ge = lm_grow(sc, L.origins, rows);
    if (ge == hipSuccess) ge = lm_grow(sc, L.normals, rows);
    if (ge == hipSuccess) ge = lm_grow(sc, L.radiance, rows);
    if (ge == hipSuccess && variance) ge = lm_grow(sc, L.variance, rows);
    if (ge != hipSuccess) {
        (void)lm_record(sc, st);
        HIP_TRY(ge);
    }
    rc = lm_resolve(sc, *d, n, L.texel.p, LmOut{nullptr, nullptr, L.origins.p, L.normals.p}, st);
    if (rc != MCPT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    const double ms_texels = ms_since(t0);
    t0 = Clock::now();
    if (n > 0) {
        const mcpt_sensor_buffers sensors{L.origins.p, L.normals.p, MCPT_SENSOR_HEMISPHERE, {0, 0, 0}};
        const mcpt_sensor_outputs so{L.radiance.p, variance ? L.variance.p : nullptr};
        rc = mcpt_query_radiance(sc, pp, n, &sensors, &so, hip_stream, stats);
        if (rc != MCPT_OK && rc != MCPT_ERR_OVERFLOW) return rc;
    }
    const double ms_radiance = ms_since(t0);
    t0 = Clock::now();
    int rs = lm_scatter(sc, d->width, d->height, n, L.texel.p, L.radiance.p, dilate, image, coverage, st);
    if (rs == MCPT_OK && variance) rs = lm_scatter(sc, d->width, d->height, n, L.texel.p, L.variance.p, 0, variance, nullptr, st);
    if (rs != MCPT_OK) return rs;
    HIP_TRY(hipStreamSynchronize(st));
    if (info) {
        info->n_texels = n;
        info->items = L.last_items;
        info->grew = L.grew ? 1 : 0;
        info->ms_texels = ms_texels;
        info->ms_radiance = ms_radiance;
        info->ms_scatter = ms_since(t0);
    }
    return rc;  // (MCPT_ERR_OVERFLOW of the radiance leg: the map is written, the message is mcpt_query_radiance's)
}

int mcpt_lightmap_texels_host(const mcpt_scene_desc *desc, const mcpt_lightmap_desc *d, int32_t *texel, int32_t *prim, float *bary, float *origins,
                              float *normals, int64_t *n_out) {
    const std::string w = "mcpt_lightmap_texels_host";
    if (!desc || !d || !n_out) return fail(MCPT_ERR_ARG, w + ": null desc, lightmap or n_out");
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (d->width < 1 || d->height < 1 || (int64_t)d->width * (int64_t)d->height > (int64_t)lm::kMaxTexels)
        return fail(MCPT_ERR_ARG, w + ": width and height must be >= 1 and width*height <= (2^31 - 1) / 3");
    if (!desc->objects || d->object < 0 || d->object >= desc->n_objects) return fail(MCPT_ERR_ARG, w + ": object out of range");
    const mcpt_object &o = desc->objects[d->object];
    if (o.kind != MCPT_OBJ_MESH) return fail(MCPT_ERR_ARG, w + ": the object is a sphere (no UV chart)");
    if (!desc->triangles || o.first_tri < 0 || o.n_tri <= 0 || o.first_tri > desc->n_triangles - o.n_tri)
        return fail(MCPT_ERR_ARG, w + ": mesh triangle range out of bounds");
    const int32_t W = d->width, H = d->height;
    // the records as build_host_scene (csrc/mcpt_scene.cpp) writes them
    std::vector<TriGeom> geom(o.n_tri);
    std::vector<TriShade> shade(o.n_tri);
    std::vector<int32_t> owner((size_t)W * H, lm::kNoOwner);
    for (int32_t k = 0; k < o.n_tri; ++k) {
        const mcpt_triangle &t = desc->triangles[o.first_tri + k];
        const mv::V3 v0 = mv::ld(t.v0);
        const mv::TriDerived D = mv::derive_triangle(v0, mv::ld(t.v1), mv::ld(t.v2));
        std::memset(&geom[k], 0, sizeof(TriGeom));
        mv::store_geom(geom[k], v0, D);
        TriShade &s = shade[k];
        std::memset(&s, 0, sizeof s);
        s.n[0] = D.n.x, s.n[1] = D.n.y, s.n[2] = D.n.z;
        for (int q = 0; q < 2; ++q) s.t0[q] = t.t0[q], s.t1[q] = t.t1[q], s.t2[q] = t.t2[q];
        int32_t tx0, ty0, ntx, nty;
        lm::tile_box(s, W, H, tx0, ty0, ntx, nty);
        for (int32_t y = ty0 * lm::kTile; y < std::min(H, (ty0 + nty) * lm::kTile); ++y)
            for (int32_t x = tx0 * lm::kTile; x < std::min(W, (tx0 + ntx) * lm::kTile); ++x) {
                double w1, w2;
                int32_t &own = owner[(size_t)y * W + x];
                if (lm::cover(s, x, y, W, H, w1, w2)) own = std::min(own, o.first_tri + k);
            }
    }
    int64_t n = 0;
    for (int32_t tx = 0; tx < W * H; ++tx) {
        if (owner[tx] == lm::kNoOwner) continue;
        const int32_t k = owner[tx] - o.first_tri;
        double w1, w2;
        (void)lm::cover(shade[k], tx % W, tx / W, W, H, w1, w2);
        const float u = (float)w1, v = (float)w2;
        if (texel) texel[n] = tx;
        if (prim) prim[n] = owner[tx];
        if (bary) bary[2 * n] = u, bary[2 * n + 1] = v;
        if (origins) lm::point(geom[k], u, v, origins + 3 * n);
        if (normals)
            for (int q = 0; q < 3; ++q) normals[3 * n + q] = d->flip_normals ? -shade[k].n[q] : shade[k].n[q];
        ++n;
    }
    *n_out = n;
    return MCPT_OK;
}

int mcpt_lightmap_dilate_host(int32_t W, int32_t H, int64_t n, const int32_t *texel, const float *values, int32_t dilate, float *image, uint8_t *coverage) {
    const std::string w = "mcpt_lightmap_dilate_host";
    if (W < 1 || H < 1 || (int64_t)W * (int64_t)H > (int64_t)lm::kMaxTexels) return fail(MCPT_ERR_ARG, w + ": width and height must be >= 1 and width*height <= (2^31 - 1) / 3");
    if (dilate < 0) return fail(MCPT_ERR_ARG, w + ": dilate must be >= 0");
    if (n < 0 || n > (int64_t)W * H) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. width*height");
    if (!image || (n > 0 && (!texel || !values))) return fail(MCPT_ERR_ARG, w + ": null image, texel or values");
    const size_t n_texels = (size_t)W * H;
    std::vector<float> img[2] = {std::vector<float>(n_texels * 3, 0.f), std::vector<float>(dilate > 0 ? n_texels * 3 : 0)};
    std::vector<uint8_t> cov[2] = {std::vector<uint8_t>(n_texels, 0), std::vector<uint8_t>(dilate > 0 ? n_texels : 0)};
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t t = (uint32_t)texel[i];
        if (t >= n_texels) continue;
        for (int q = 0; q < 3; ++q) img[0][3 * (size_t)t + q] = values[3 * i + q];
        cov[0][t] = 1;
    }
    int cur = 0;
    for (int32_t r = 0; r < dilate; ++r, cur ^= 1)
        for (int32_t y = 0; y < H; ++y)
            for (int32_t x = 0; x < W; ++x) {
                const size_t t = (size_t)y * W + x;
                lm::dilate_texel(W, H, x, y, img[cur].data(), cov[cur].data(), &img[cur ^ 1][3 * t], cov[cur ^ 1][t]);
            }
    std::memcpy(image, img[cur].data(), n_texels * 3 * sizeof(float));
    if (coverage) std::memcpy(coverage, cov[cur].data(), n_texels);
    return MCPT_OK;
}

}  // extern "C"
