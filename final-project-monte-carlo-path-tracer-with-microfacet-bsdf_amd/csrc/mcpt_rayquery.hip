// Ray queries on device memory (include/mcpt.h: mcpt_query_closest, mcpt_query_occluded): rays are read from and results written to
// the memory of the scene's device, on the caller's stream, through staging buffers the scene owns (QueryBufs, csrc/mcpt_host.h).
//
// Per chunk of at most MCPT_QUERY_CHUNK rays, all on the caller's stream:
//   k_query_pack       the caller's tight n*3 arrays -> the traversal's float4 ray arrays; the direction's .w carries tmax (+inf without
//                      one), the layout of a shadow-queue entry.  One lane per ray: a wave reads 768 contiguous bytes of each array.
//   closest hits       launch_trace_closest (csrc/mcpt_kernels.hip) on the staged chunk: the refill kernel, every stack flavour, the
//                      retrace and the LDS-resident flavour, exactly as mcpt_intersect runs them.  No second copy of the loop.
//   k_query_resolve    {t, prim} hit + ray + live records -> the outputs the caller asked for.  The tmax filter first, on the finished
//                      closest hit; for triangles the test that recorded the hit is repeated for (u, v) (hit_points, csrc/mcpt_temporal.hip).
//   k_query_occluded   the any-hit query: one lane per staged ray, traverse<true, ...>(.., tmax, .., found = true), i.e. the kOccluder
//                      walk alone, which ends at the first primitive with t - tmax <= -EPSILON.  k_query_occluded_retrace: the rays of a
//                      retry-flavour launch that lost a stack entry, again with the scratch stack.
// Small scenes: k_query_occluded's SMALL instantiation has no LDS prologue; it walks the global arrays (which exist for every scene)
// with the 8-entry stack of the small flavour, the plain walk the checking build runs on those scenes too.
//
// Radiance at sensors in device memory (mcpt_query_radiance, mcpt_sensor_rays) is at the end of the file: the entry points alone; their
// kernels sit beside k_primary in csrc/mcpt_kernels.hip, the first ray of a sensor's sample in csrc/mcpt_sensor.h.
#include <cfloat>
#include <cmath>

#include "mcpt_frame.h"
#include "mcpt_host.h"
#include "mcpt_stack_dispatch.h"
#include "mcpt_traverse.h"

using namespace mcpt;

namespace mcpt {

namespace {

inline uint32_t query_blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

MCPT_DI double query_hit_t(const uint4 &h) { return __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x)); }

__global__ __launch_bounds__(kBlock) void k_query_pack(uint32_t n, const float *__restrict__ origins, const float *__restrict__ dirs,
                                                       const float *__restrict__ tmax, float4 *__restrict__ ray_o, float4 *__restrict__ ray_d) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t j = 3 * (size_t)i;
    ray_o[i] = make_float4(origins[j], origins[j + 1], origins[j + 2], 0.f);
    ray_d[i] = make_float4(dirs[j], dirs[j + 1], dirs[j + 2], tmax ? tmax[i] : INFINITY);
}

// The object of triangle `prim`: the last mesh range whose first triangle is <= prim (the bisection of k_move_objects).
MCPT_DI int32_t query_object_of(const int32_t *__restrict__ starts, const int32_t *__restrict__ objs, int32_t n_ranges, int32_t prim) {
    int32_t lo = 0, hi = n_ranges - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= prim) lo = mid;
        else hi = mid - 1;
    }
    return objs[lo];
}

// Which outputs are wanted is a wave-uniform branch on the pointers; every store is a plain vector store.
__global__ __launch_bounds__(kBlock) void k_query_resolve(DevScene S, uint32_t n, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                          const uint4 *__restrict__ hit, int has_tmax, const int32_t *__restrict__ starts,
                                                          const int32_t *__restrict__ objs, int32_t n_ranges, QueryOut out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint4 h = hit[i];
    const float4 d4 = ray_d[i];
    int32_t prim = (int32_t)h.z;
    double t = query_hit_t(h);
    // the occluder rule of leaf_step (csrc/mcpt_traverse.h) with dist = tmax, on the finished closest hit
    const bool ok = prim >= 0 && (!has_tmax || t - (double)d4.w <= -(double)kEps);
    if (!ok) {
        t = DBL_MAX;
        prim = -1;
    }
    if (out.t) out.t[i] = t;
    if (out.prim) out.prim[i] = prim;
    if (!(out.object || out.uv || out.normal || out.point)) return;
    int32_t object = -1;
    float uf = 0.f, vf = 0.f;
    f3 nrm = mk3(0.f, 0.f, 0.f), p = mk3(0.f, 0.f, 0.f);
    if (ok) {
        const float4 o4 = ray_o[i];
        const f3 ro = mk3(o4.x, o4.y, o4.z), rd = mk3(d4.x, d4.y, d4.z);
        if (prim < S.n_tri) {
            if (out.uv || out.point) {
                const TriGeom g = S.tri_geom[prim];
                double tt, u, v;
                if (tri_hit(g, make_ray(ro, rd), tt, u, v)) {  // (the test that recorded the hit: it succeeds again)
                    uf = (float)u;
                    vf = (float)v;
                }
                p = mk3(g.v0[0] + (g.e1x * uf + g.e2xy[0] * vf), g.v0[1] + (g.e1yz[0] * uf + g.e2xy[1] * vf), g.v0[2] + (g.e1yz[1] * uf + g.e2z * vf));
            }
            if (out.normal) {
                const float4 q = *reinterpret_cast<const float4 *>(S.tri_shade + prim);  // {n.xyz, mat}
                nrm = mk3(q.x, q.y, q.z);
            }
            if (out.object) object = query_object_of(starts, objs, n_ranges, prim);
        } else {
            const int32_t k = prim - S.n_tri;  // a sphere's slot is its object index
            object = k;
            if (out.normal || out.point) {
                const float4 c = *reinterpret_cast<const float4 *>(S.spheres + k);  // {c.xyz, radius}
                p = ro + rd * (float)t;
                nrm = normalized(p - mk3(c.x, c.y, c.z));
            }
        }
    }
    if (out.object) out.object[i] = object;
    if (out.uv) {
        out.uv[2 * (size_t)i] = uf;
        out.uv[2 * (size_t)i + 1] = vf;
    }
    if (out.normal) {
        out.normal[3 * (size_t)i] = nrm.x;
        out.normal[3 * (size_t)i + 1] = nrm.y;
        out.normal[3 * (size_t)i + 2] = nrm.z;
    }
    if (out.point) {
        out.point[3 * (size_t)i] = p.x;
        out.point[3 * (size_t)i + 1] = p.y;
        out.point[3 * (size_t)i + 2] = p.z;
    }
}

// Any-hit: `found = true` skips the window walk, so only the kOccluder walk runs and `visible` is "no primitive with t - tmax <= -EPSILON".
// PREP (the dispatch's small-scene slot): the plain walk over the global arrays with STK = kSmallStk entries; no LDS copy of the scene.
template <int STK, bool MARK, bool PREP>
__global__ __launch_bounds__(kBlock) void k_query_occluded(DevScene S, uint32_t n, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                           uint8_t *__restrict__ occluded, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kBlock + tid;
    if (i >= n) return;
    const float4 o = ray_o[i], d = ray_d[i];
    const Ray r = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z));
    const TraceResult tr = traverse<true, STK, MARK, false>(S, r, d.w, stk, tid, /*found=*/true);
    if (MARK && tr.dropped) retry_append(rl, i);  // (undecided: k_query_occluded_retrace)
    else occluded[i] = tr.visible ? 0 : 1;
}

__global__ __launch_bounds__(kBlock) void k_query_occluded_retrace(DevScene S, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                                   uint8_t *__restrict__ occluded, RetryList rl) {
    __shared__ int32_t stk[1][kBlock];
    const uint32_t n = min(*rl.count, rl.cap);
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const uint32_t i = rl.items[k];
        const float4 o = ray_o[i], d = ray_d[i];
        const Ray r = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z));
        const TraceResult tr = traverse_scratch<true>(S, r, d.w, stk, threadIdx.x, /*found=*/true);
        occluded[i] = tr.visible ? 0 : 1;
    }
    retry_finish(rl);
}

}  // namespace

void launch_query_pack(uint32_t n, const float *origins, const float *dirs, const float *tmax, float4 *ray_o, float4 *ray_d, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_query_pack, dim3(query_blocks(n)), dim3(kBlock), 0, s, n, origins, dirs, tmax, ray_o, ray_d);
}

void launch_query_resolve(const DevScene &S, uint32_t n, const float4 *ray_o, const float4 *ray_d, const uint4 *hit, bool has_tmax, const int32_t *starts,
                          const int32_t *objs, int32_t n_ranges, const QueryOut &out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_query_resolve, dim3(query_blocks(n)), dim3(kBlock), 0, s, S, n, ray_o, ray_d, hit, has_tmax ? 1 : 0, starts, objs, n_ranges, out);
}

void launch_query_occluded(const DevScene &S, uint32_t n, const float4 *ray_o, const float4 *ray_d, uint8_t *occluded, const RetryList &rl, hipStream_t s) {
    if (n == 0) return;
    const dim3 g(query_blocks(n)), b(kBlock);
    MCPT_STACK_DISPATCH(S.height, k_query_occluded, hipLaunchKernelGGL(k_query_occluded_retrace, dim3(kRetraceGrid), b, 0, s, S, ray_o, ray_d, occluded, rl), g, b, 0,
                        s, S, n, ray_o, ray_d, occluded, rl);
}

}  // namespace mcpt

namespace {

// The table of mesh triangle-range starts for the object lookup, in ascending order of the first triangle: m starts, then the m objects.
void build_range_table(const SceneSource &S, std::vector<int32_t> &table) {
    std::vector<std::pair<int32_t, int32_t>> r;
    for (size_t o = 0; o < S.objects.size(); ++o)
        if (S.objects[o].kind == MCPT_OBJ_MESH) r.emplace_back(S.objects[o].first_tri, (int32_t)o);
    std::sort(r.begin(), r.end());
    const size_t m = r.size();
    table.assign(2 * std::max<size_t>(m, 1), 0);
    for (size_t k = 0; k < m; ++k) {
        table[k] = r[k].first;
        table[std::max<size_t>(m, 1) + k] = r[k].second;
    }
    if (m == 0) table[1] = -1;  // (no mesh: no triangle can be hit)
}

}  // namespace

namespace mcpt {

// Makes the scene's staging buffers hold `chunk` rays on stream st (QueryBufs, csrc/mcpt_host.h): growth behind query_settle, the wait
// for a query on another stream, the range table.  rl: the retry list of the chunk's launches.  Shared by the ray queries and
// mcpt_query_probe_depth (csrc/mcpt_probes.hip); whatever is enqueued afterwards is closed with query_finish.
int query_stage(mcpt_scene *sc, uint32_t chunk, hipStream_t st, mcpt_query_info &qi, RetryList &rl) {
    QueryBufs &Q = sc->query;
    const bool need_retry = stack_uses_retry(sc->view.height);
    if (!Q.table_valid) build_range_table(sc->src, Q.h_ranges);
    const bool grow = Q.ray_o.n < chunk || Q.ray_d.n < chunk || Q.hit.n < chunk || (need_retry && Q.retry.cap[0] < chunk) || Q.ranges.n < Q.h_ranges.size() || !Q.done.e;
    if (grow) {
        HIP_TRY(query_settle(sc));  // the buffers about to be freed may still be read by an earlier query
        if (!Q.done.e) HIP_TRY(Q.done.create());
        HIP_TRY(Q.ray_o.alloc(chunk));
        HIP_TRY(Q.ray_d.alloc(chunk));
        HIP_TRY(Q.hit.alloc(chunk));
        if (need_retry && Q.retry.cap[0] < chunk) {
            HIP_TRY(Q.retry.ctl.alloc(8));
            HIP_TRY(hipMemsetAsync(Q.retry.ctl.p, 0, 8 * sizeof(uint32_t), st));  // (the lists are empty between launches: zero again is the same state)
            HIP_TRY(Q.retry.items[0].alloc(chunk));
            Q.retry.cap[0] = chunk;
        }
        if (Q.ranges.n < Q.h_ranges.size()) {
            HIP_TRY(Q.ranges.alloc(Q.h_ranges.size()));
            Q.table_valid = false;
        }
        qi.grew = 1;
    }
    // a query on another stream may still be using the staging buffers
    if (Q.pending && st != Q.last_stream) HIP_TRY(hipStreamWaitEvent(st, Q.done, 0));
    if (!Q.table_valid) {  // (first call, and after mcpt_scene_add_objects, which has waited for every earlier query: a blocking copy, done before anything below is enqueued)
        HIP_TRY(hipMemcpy(Q.ranges.p, Q.h_ranges.data(), Q.h_ranges.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        Q.table_valid = true;
    }
    rl = need_retry ? Q.retry.list(0) : RetryList{nullptr, nullptr, nullptr, 0u};
    return MCPT_OK;
}

// Records QueryBufs::done behind what a call enqueued on st since query_stage, and reports the staging's size.
int query_finish(mcpt_scene *sc, hipStream_t st, mcpt_query_info &qi) {
    QueryBufs &Q = sc->query;
    const hipError_t le = hipGetLastError();
    // behind the kernels even when a launch failed: whatever was enqueued still reads the scene
    const hipError_t re = hipEventRecord(Q.done, st);
    if (re == hipSuccess) {
        Q.pending = true;
        Q.last_stream = st;
    }
    HIP_TRY(le);
    HIP_TRY(re);
    qi.staged_bytes = (int64_t)(Q.ray_o.bytes() + Q.ray_d.bytes() + Q.hit.bytes() + Q.ranges.bytes() + Q.retry.items[0].bytes() + Q.retry.ctl.bytes());
    return MCPT_OK;
}

}  // namespace mcpt

namespace {

// Both queries after their argument checks.  occluded != nullptr: the any-hit query; else closest hits into `hits`.
int run_query(mcpt_scene *sc, int64_t n, const mcpt_ray_buffers &rays, const mcpt_hit_buffers *hits, uint8_t *occluded, hipStream_t st, mcpt_query_info *info) {
    mcpt_query_info qi;
    std::memset(&qi, 0, sizeof qi);
    HIP_TRY(hipSetDevice(sc->device));
    QueryBufs &Q = sc->query;
    const uint32_t chunk = (uint32_t)std::min<int64_t>(n, (int64_t)sc->knobs.query_chunk);
    RetryList rl;
    const int sc_rc = query_stage(sc, chunk, st, qi, rl);
    if (sc_rc != MCPT_OK) return sc_rc;
    const int32_t n_ranges = (int32_t)(Q.h_ranges.size() / 2);
    for (int64_t base = 0; base < n; base += chunk) {
        const uint32_t m = (uint32_t)std::min<int64_t>(chunk, n - base);
        launch_query_pack(m, rays.origins + 3 * base, rays.dirs + 3 * base, rays.tmax ? rays.tmax + base : nullptr, Q.ray_o.p, Q.ray_d.p, st);
        if (occluded) {
            launch_query_occluded(sc->view, m, Q.ray_o.p, Q.ray_d.p, occluded + base, rl, st);
        } else {
            launch_trace_closest(sc->view, m, nullptr, Q.ray_o.p, Q.ray_d.p, Q.hit.p, rl, st);
            const QueryOut out{hits->t ? hits->t + base : nullptr,           hits->prim ? hits->prim + base : nullptr,
                               hits->object ? hits->object + base : nullptr, hits->uv ? hits->uv + 2 * base : nullptr,
                               hits->normal ? hits->normal + 3 * base : nullptr, hits->point ? hits->point + 3 * base : nullptr};
            launch_query_resolve(sc->view, m, Q.ray_o.p, Q.ray_d.p, Q.hit.p, rays.tmax != nullptr, Q.ranges.p, Q.ranges.p + n_ranges, n_ranges, out, st);
        }
        qi.launches++;
    }
    const int fr = query_finish(sc, st, qi);
    if (fr != MCPT_OK) return fr;
    if (info) *info = qi;
    return MCPT_OK;
}

// The checks both calls share, before any device work.  0: go on; 1: n == 0, nothing to do; < 0: -(error code).
int check_rays(const char *who, const mcpt_scene *sc, int64_t n, const mcpt_ray_buffers *rays, bool need_tmax, mcpt_query_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    const std::string w(who);
    if (!sc) return -fail(MCPT_ERR_ARG, w + ": null scene");
    if (n < 0 || n > 0x7fffffff) return -fail(MCPT_ERR_ARG, w + ": n must be in 0 .. 2^31 - 1");
    if (n == 0) return 1;
    if (!rays || !rays->origins || !rays->dirs) return -fail(MCPT_ERR_ARG, w + ": null rays, origins or dirs");
    if (need_tmax && !rays->tmax) return -fail(MCPT_ERR_ARG, w + ": tmax is required");
    if (!on_device(rays->origins, sc->device) || !on_device(rays->dirs, sc->device) || (rays->tmax && !on_device(rays->tmax, sc->device)))
        return -fail(MCPT_ERR_ARG, w + ": origins, dirs and tmax must be memory of the scene's device");
    return 0;
}

}  // namespace

extern "C" {

int mcpt_query_closest(mcpt_scene *sc, int64_t n, const mcpt_ray_buffers *rays, const mcpt_hit_buffers *hits, void *hip_stream, mcpt_query_info *info) {
    const int c = check_rays("mcpt_query_closest", sc, n, rays, false, info);
    if (c < 0) return -c;
    if (hits && !hits->t && !hits->prim && !hits->object && !hits->uv && !hits->normal && !hits->point) return fail(MCPT_ERR_ARG, "mcpt_query_closest: every hit pointer is null");
    if (c == 1) return MCPT_OK;
    if (!hits) return fail(MCPT_ERR_ARG, "mcpt_query_closest: null hits");
    const void *outs[6] = {hits->t, hits->prim, hits->object, hits->uv, hits->normal, hits->point};
    for (const void *p : outs)
        if (p && !on_device(p, sc->device)) return fail(MCPT_ERR_ARG, "mcpt_query_closest: an output is not memory of the scene's device");
    return run_query(sc, n, *rays, hits, nullptr, (hipStream_t)hip_stream, info);
}

int mcpt_query_occluded(mcpt_scene *sc, int64_t n, const mcpt_ray_buffers *rays, uint8_t *occluded, void *hip_stream, mcpt_query_info *info) {
    const int c = check_rays("mcpt_query_occluded", sc, n, rays, true, info);
    if (c < 0) return -c;
    if (c == 1) return MCPT_OK;
    if (!occluded) return fail(MCPT_ERR_ARG, "mcpt_query_occluded: null occluded");
    if (!on_device(occluded, sc->device)) return fail(MCPT_ERR_ARG, "mcpt_query_occluded: occluded is not memory of the scene's device");
    return run_query(sc, n, *rays, nullptr, occluded, (hipStream_t)hip_stream, info);
}

// Radiance at sensors: a frame of n pixels whose first rays come from the caller's arrays (csrc/mcpt_sensor.h) instead of a camera.
// render_list does the work -- workspace and pass sizing, regeneration, pipelined passes, the fold in sample order, the moments -- on the
// scene's own buffers with the caller's `radiance` as the framebuffer and no pixel list.  It reads the geometry, which ray queries in
// flight only read as well, and none of the staging buffers the ray-query event guards: there is nothing to settle first.
int mcpt_query_radiance(mcpt_scene *sc, const mcpt_params *pp, int64_t n, const mcpt_sensor_buffers *sensors, const mcpt_sensor_outputs *out,
                        void *hip_stream, mcpt_stats *stats) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_query_radiance: ") + what); };
    if (!sc) return bad("null scene");
    if (!pp || !sensors || !out) return bad("null params, sensors or out");
    const mcpt_params &p = *pp;
    if (n < 0 || n > 0x7fffffff / 3) return bad("n must be in 0 .. (2^31 - 1) / 3");
    if (sensors->kind != MCPT_SENSOR_RAY && sensors->kind != MCPT_SENSOR_HEMISPHERE) return bad("unknown sensor kind");
    if (sensors->reserved[0] || sensors->reserved[1] || sensors->reserved[2]) return bad("reserved words must be 0");
    if (p.nranks > 1 || p.rank != 0) return bad("nranks must be 1 and rank 0 (sensors are not partitioned)");
    if (p.spp <= 0 || p.n_dir_sample <= 0 || !(p.rr_rate > 0.f)) return bad("spp/n_dir_sample/rr_rate must be positive");
    if (out->variance && (p.spp < 2 || p.accumulate != 0 || p.spp_total != 0 || p.sample_offset != 0))
        return bad("variance needs spp >= 2 and accumulate, spp_total and sample_offset 0");
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof *stats);
        return MCPT_OK;
    }
    if (!sensors->origins || !sensors->dirs || !out->radiance) return bad("null origins, dirs or radiance");
    if (!on_device(sensors->origins, sc->device) || !on_device(sensors->dirs, sc->device) || !on_device(out->radiance, sc->device) ||
        (out->variance && !on_device(out->variance, sc->device)))
        return bad("origins, dirs, radiance and variance must be memory of the scene's device");
    return sensor_radiance(sc, p, (uint32_t)n, SensorConst{sensors->origins, sensors->dirs, sensors->kind}, out->radiance, out->variance, nullptr,
                           (hipStream_t)hip_stream, stats);
}

}  // extern "C"

namespace mcpt {

int sensor_radiance(mcpt_scene *sc, const mcpt_params &p, uint32_t ns, const SensorConst &sn, float *radiance, float *variance, float *sh,
                    hipStream_t st, mcpt_stats *stats) {
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();  // an earlier, already reported failure of this thread must not be taken for one of this call
    const Clock::time_point t0 = Clock::now();
    double *moments = nullptr;
    if (variance) {
        HIP_TRY(sc->shared.sensor_moments.alloc((size_t)ns * 6));
        moments = sc->shared.sensor_moments.p;
        HIP_TRY(hipMemsetAsync(moments, 0, (size_t)ns * 6 * sizeof(double), st));
    }
    if (!p.accumulate) {
        HIP_TRY(hipMemsetAsync(radiance, 0, (size_t)ns * 3 * sizeof(float), st));
        if (sh) HIP_TRY(hipMemsetAsync(sh, 0, (size_t)ns * 27 * sizeof(float), st));
    }
    const float spp_total = (float)(p.spp_total > 0 ? p.spp_total : p.spp);
    const ShSink sink{sn, p.seed, sh};
    Totals rt;
    const int rc = render_list(sc, sn, p, nullptr, nullptr, ns, p.sample_offset, p.spp, spp_total, radiance, moments, st, t0, rt, sh ? &sink : nullptr);
    if (rc != MCPT_OK) return rc;
    if (variance) {
        launch_sensor_variance(ns, p.spp, moments, variance, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    const uint64_t samples = (uint64_t)ns * (uint64_t)p.spp;
    if (stats) fill_stats(stats, samples, samples, p.n_dir_sample, rt, t0);
    sc->last_cont_traced = rt.cont_traced;  // (mcpt_scene_ray_counts)
    sc->last_cont_shared = rt.cont_shared;
    sc->last_pc_samples = rt.pc_samples;  // (mcpt_scene_primary_conductor_counts)
    sc->last_pc_rays = rt.pc_rays;
    if (rt.overflow) return fail(MCPT_ERR_OVERFLOW, "some paths outran the clamp stack (raise params.max_depth)");
    return MCPT_OK;
}

}  // namespace mcpt

extern "C" {

int mcpt_sensor_rays(mcpt_scene *sc, int32_t kind, uint32_t seed, int64_t n, const float *origins, const float *dirs, const uint32_t *sensor,
                     const uint32_t *sample, float *origins_out, float *dirs_out) {
    if (!sc || n < 0 || (n > 0 && (!origins || !dirs || !sensor || !sample || !origins_out || !dirs_out))) return fail(MCPT_ERR_ARG, "mcpt_sensor_rays: bad argument");
    if (kind != MCPT_SENSOR_RAY && kind != MCPT_SENSOR_HEMISPHERE) return fail(MCPT_ERR_ARG, "mcpt_sensor_rays: unknown sensor kind");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_sensor_rays: too many rays for one call");
    size_t m = 0;  // the sensors the pairs name: rows 0 .. max(sensor) of origins and dirs
    for (int64_t j = 0; j < n; ++j) m = std::max<size_t>(m, (size_t)sensor[j] + 1);
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> dPo, dPd;
    DevBuf<uint32_t> dI, dS;
    DevBuf<float4> dO, dD;
    HIP_TRY(dO.alloc(n));
    HIP_TRY(dD.alloc(n));
    HIP_TRY(upload(dPo, origins, m * 3));
    HIP_TRY(upload(dPd, dirs, m * 3));
    HIP_TRY(upload(dI, sensor, n));
    HIP_TRY(upload(dS, sample, n));
    launch_sensor_rays(SensorConst{dPo.p, dPd.p, kind}, seed, (uint32_t)n, dI.p, dS.p, dO.p, dD.p, nullptr);
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

}  // extern "C"
