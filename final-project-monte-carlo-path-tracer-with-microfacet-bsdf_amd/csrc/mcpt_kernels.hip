// HIP kernels of the wavefront path tracer for gfx950 (MI355X, CDNA4; 64-wide wavefronts).
//
// Pipeline per wavefront iteration (host loop in mcpt_wavefront.hip):
//   k_shade          one lane per path record: resolves the pending vertex (direct-light sum, continuation
//                    hit), finishes the path or pushes a clamp-stack level, samples the BSDF at the next vertex and
//                    emits a vertex record + at most one continuation ray; survivors are stream-compacted into
//                    the next list with ballot/popcount wave-aggregated atomics.
//   k_primary        camera ray + closest hit for new samples, fused (one primary ray feeds the three channel
//                    paths); sky misses and depth-0 emitter hits are finished here and never become records, and so are first hits
//                    on smooth conductors without direct light, whose reflected ray the kernel walks itself (primary_sample).
//   k_direct         direct lighting, one lane per (vertex, light sample); non-zero samples enter the shadow queue.
//   k_trace_closest  closest hit for continuation rays.
//   k_trace_shadow   shadow queue (persistent grid): the distance-equality visibility of Scene.cpp:75.
//   k_accumulate     per pass: framebuffer[m] += rgb/spp in sample order (Renderer.cpp:80).
//
// Reference logic covered: Renderer.cpp:39-80, Scene.cpp:19-37,56-184, BVH.cpp:95-135,
// Bounds3.hpp:95-108, Triangle.hpp:71-76,193-196,222-252, Sphere.hpp:26-48, Material.hpp:26-408.
#include <algorithm>
#include <cfloat>
#include <cstdlib>

#include "mcpt_direct.h"
#include "mcpt_kernels.h"
#include "mcpt_stack_dispatch.h"
#include "mcpt_traverse.h"

namespace mcpt {

namespace {

#ifndef MCPT_SHADE_BLOCK
#define MCPT_SHADE_BLOCK 512
#endif
constexpr int kShadeBlock = MCPT_SHADE_BLOCK;  // k_shade: larger workgroups = fewer allocation atomics per hot counter

// Block-aggregated queue allocation.  Up to kMaxAlloc counters are served by ONE round of atomics per
// workgroup (lane k of wave 0 adds the block total of request k), instead of one returning atomic per
// wave and counter: the hot counters are the only cross-workgroup contention points of the pipeline.
// Must be called by every thread of the block (it contains barriers).
constexpr int kMaxAlloc = 10;
constexpr int kMaxWaves = 16;
struct BlockAllocShared {
    uint32_t cnt[kMaxWaves][kMaxAlloc];  // in: requests of wave w; out (after the first barrier): requests of the waves before w
    uint32_t base[kMaxAlloc];
};

// begin: ballots, per-wave counts to LDS, one barrier, then lanes 0..N-1 of wave 0 issue the atomics and publish the
// bases.  end: second barrier, per-lane indices.  Work that does not need the indices can sit between the two calls:
// the other waves then compute while wave 0 waits for its atomics to return.
template <int N>
MCPT_DI void block_alloc_begin(BlockAllocShared &sh, const bool (&want)[N], const uint32_t (&mult)[N], uint32_t *const (&counter)[N],
                               const bool (&subtract)[N], uint32_t (&prefix)[N]) {
    static_assert(N <= kMaxAlloc, "too many allocation requests");
    const uint32_t n_waves = blockDim.x >> 6;
    const uint32_t lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned long long mask = __ballot(want[k]);
        prefix[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (lane == 0) sh.cnt[wave][k] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (threadIdx.x == (unsigned)k) {  // lanes 0..N-1 of wave 0 issue their atomics in the same instruction
            uint32_t total = 0;
            for (uint32_t w = 0; w < n_waves; ++w) {  // counts -> exclusive prefix over the waves, in place
                const uint32_t c = sh.cnt[w][k];
                sh.cnt[w][k] = total;
                total += c;
            }
            uint32_t base = 0;
            if (total) {
                const uint32_t amount = total * mult[k];
                base = subtract[k] ? (atomicSub(counter[k], amount) - amount) : atomicAdd(counter[k], amount);
            }
            sh.base[k] = base;
        }
    }
}

template <int N>
MCPT_DI void block_alloc_end(BlockAllocShared &sh, const uint32_t (&mult)[N], const uint32_t (&prefix)[N], uint32_t (&index)[N]) {
    const uint32_t wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) index[k] = sh.base[k] + (sh.cnt[wave][k] + prefix[k]) * mult[k];
}

MCPT_DI f3 ld3(float4 v) { return mk3(v.x, v.y, v.z); }

// (An XCD-aware block-id remap -- cdna_hip_programming.md T1: every XCD gets a contiguous eighth of the rays, so that neighbouring
// pixels share one L2 -- was measured 24 % SLOWER on the chess frame (3380 vs 4440 Msamples/s): hardware block ids are dealt
// round-robin to the XCDs, which spreads the cheap sky tiles and the expensive glass tiles evenly over them; a contiguous eighth per
// XCD turns the frame's spatial cost variation into XCD load imbalance.  The scene fits every L2 anyway.)

// ------------------------------------------------------------------------------------------------
// Small scenes (the Cornell configurations: 31-34 nodes, 32 triangles, 3 spheres, 7 KB in all): the SMALL instantiations of the
// traversal kernels copy nodes, TriGeom and sphere records into LDS once per workgroup and repoint their by-value DevScene at the
// copy, so every node visit and primitive test reads LDS instead of the vector cache; the traversal stack is 8 entries (trees of up
// to 9 levels).  A wave-uniform template flavour: there is no LDS / global select inside the loop (that select is what sank
// the top-of-tree staging experiment on the chess scene).  The pointers are generic ones derived from __shared__
// arrays; after inlining the compiler's address-space inference turns the loads into ds_read_b128 (tools/kernel_resources.py shows
// no flat_load in the SMALL kernels' loops).
// ------------------------------------------------------------------------------------------------
// (limits: kSmall* in mcpt_kernels.h; mcpt_scene_create decides `DevScene::small` from them)
struct alignas(16) SmallGeomLds {
    uint4 nodes[kSmallNodes * 4];  // Node records (64 B), or QNode records (32 B) in the first half
    TriGeom tri[kSmallTris];
    SphereRec sph[kSmallSphereSlots];
};
struct alignas(16) SmallLightLds {
    MaterialRec mats[kSmallMats];
    LightRec lights[kSmallLights];
    LightNode nodes[kSmallLightNodes];
    LightTri tris[kSmallLightTris];
};
MCPT_DI void lds_copy16(void *dst, const void *src, uint32_t n16) {  // n16 16-byte words, by the whole workgroup
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint4 *g = reinterpret_cast<const uint4 *>(src);
    for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) d[i] = g[i];
}
// (the caller's __syncthreads follows: a kernel that stages both blocks pays for one barrier)
MCPT_DI void stage_small_geom(DevScene &S, SmallGeomLds &L) {
    // Quantised nodes become "prepared" nodes (node_visit, NF = 2): the 16-bit grid coordinates as floats relative to the grid origin,
    // x' = (float)q * cell, in the layout of Node.  Float nodes are copied as they are.  (Every node pointer the SMALL kernels follow ends up
    // as an LDS pointer or null on every path, so that the address-space inference sees no global / LDS mix.)
    const bool quant = S.qnodes != nullptr;
    if (quant) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)S.n_inner; i += blockDim.x) {
            const uint4 *q = reinterpret_cast<const uint4 *>(S.qnodes + i);
            const uint4 a = q[0], b = q[1];
            const float cx = S.q_cell[0], cy = S.q_cell[1], cz = S.q_cell[2];
            float4 *o = reinterpret_cast<float4 *>(L.nodes) + 4 * i;
            o[0] = make_float4((float)(a.x & 0xffffu) * cx, (float)(a.x >> 16) * cy, (float)(a.y & 0xffffu) * cz, (float)(a.y >> 16) * cx);
            o[1] = make_float4((float)(a.z & 0xffffu) * cy, (float)(a.z >> 16) * cz, (float)(a.w & 0xffffu) * cx, (float)(a.w >> 16) * cy);
            o[2] = make_float4((float)(b.x & 0xffffu) * cz, (float)(b.x >> 16) * cx, (float)(b.y & 0xffffu) * cy, (float)(b.y >> 16) * cz);
            o[3] = make_float4(__int_as_float((int32_t)b.z), __int_as_float((int32_t)b.w), 0.f, 0.f);
        }
    } else {
        lds_copy16(L.nodes, S.nodes, (uint32_t)S.n_inner * (uint32_t)(sizeof(Node) / 16));
    }
    S.nodes = reinterpret_cast<const Node *>(L.nodes);
    S.pnodes = quant ? reinterpret_cast<const float4 *>(L.nodes) : nullptr;
    lds_copy16(L.tri, S.tri_geom, (uint32_t)S.n_tri * (uint32_t)(sizeof(TriGeom) / 16));
    lds_copy16(L.sph, S.spheres, (uint32_t)S.n_sphere_slots * (uint32_t)(sizeof(SphereRec) / 16));
    S.tri_geom = L.tri;
    S.spheres = L.sph;
}
MCPT_DI void stage_small_lights(DevScene &S, SmallLightLds &L) {
    lds_copy16(L.mats, S.mats, (uint32_t)S.n_mats * (uint32_t)(sizeof(MaterialRec) / 16));
    lds_copy16(L.lights, S.lights, (uint32_t)S.n_lights * (uint32_t)(sizeof(LightRec) / 16));
    lds_copy16(L.nodes, S.light_nodes, (uint32_t)S.n_light_nodes * (uint32_t)(sizeof(LightNode) / 16));
    lds_copy16(L.tris, S.light_tris, (uint32_t)S.n_light_tris * (uint32_t)(sizeof(LightTri) / 16));
    S.mats = L.mats;
    S.lights = L.lights;
    S.light_nodes = L.nodes;
    S.light_tris = L.tris;
}

template <int STK, bool RETRY, bool SMALL>
__global__ __launch_bounds__(kBlock) void k_trace_closest(DevScene S, uint32_t n_host, const uint32_t *__restrict__ n_dev,
                                                          const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                          uint4 *__restrict__ hit, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    if constexpr (SMALL) {
        __shared__ SmallGeomLds small_geom;
        stage_small_geom(S, small_geom);
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const uint32_t n = n_dev ? *n_dev : n_host;
    // grid-stride: when the length is only known on the device the host sizes the grid from an estimate
    for (uint32_t i = blockIdx.x * kBlock + tid; i < n; i += gridDim.x * kBlock) {
        const Ray r = make_ray(ld3(ray_o[i]), ld3(ray_d[i]));
        const TraceResult tr = traverse<false, STK, RETRY, SMALL>(S, r, 0.f, stk, tid);
        if (RETRY && tr.dropped) retry_append(rl, i);
        else hit[i] = pack_hit(tr.t, tr.prim, tr.mat_bits);
    }
}

// The rays k_trace_closest / k_trace_closest_refill put on their retrace list, with the scratch stack.
__global__ __launch_bounds__(kBlock) void k_retrace_closest(DevScene S, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                            uint4 *__restrict__ hit, RetryList rl) {
    __shared__ int32_t stk[1][kBlock];
    const uint32_t n = min(*rl.count, rl.cap);
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const uint32_t i = rl.items[k];
        const Ray r = make_ray(ld3(ray_o[i]), ld3(ray_d[i]));
        const TraceResult tr = traverse_scratch<false>(S, r, 0.f, stk, threadIdx.x);
        hit[i] = pack_hit(tr.t, tr.prim, tr.mat_bits);
    }
    retry_finish(rl);
}

// k_trace_closest with lane refill.  Rays of one wave finish at different times (59 % lane utilisation with one ray per lane,
// profiles/r02_traversal_stats.txt).  Here a wave owns a chunk of kRaysPerLane x 64 consecutive rays and, at the top of every round
// of the speculative loop, lanes whose ray has finished store its hit and -- once at least kRefillMin lanes are idle -- take the next
// rays of the chunk (ballot + prefix count: no atomics, no persistent grid: the grid is still one workgroup per 1024 rays).
// The common configuration only (quantised nodes, no instancing); the rays of the chunk that have a zero direction component are traced
// by the generic path before the loop starts (round 3: tracing them inside a refill, with the rest of the wave parked in the middle of
// its own walks, lost the rest of the chunk when a refill handed out nothing but such rays -- tests/test_gpu_small_scene.py has the
// case).  The walk itself is traverse_loop's, piece by piece (csrc/mcpt_traverse.h): quantised or prepared nodes, the plain slab test.
#ifndef MCPT_REFILL_MIN
#define MCPT_REFILL_MIN 16
#endif
#ifndef MCPT_RAYS_PER_LANE
#define MCPT_RAYS_PER_LANE 4
#endif
constexpr uint32_t kRaysPerLane = MCPT_RAYS_PER_LANE, kRefillMin = MCPT_REFILL_MIN;
// Occupancy: the refill state costs registers.  Round 2: 79 VGPRs unconstrained (6 waves per SIMD); bounded to 7 waves (72 VGPRs, 14 spilled)
// was the optimum then: frame 4617 (one ray per lane) -> 4645 (unconstrained) -> 4695 (7 waves) -> 4620 (8 waves, 42 spills).  Round 3 moved the
// generic walk of zero-component rays out of the loop, which freed registers: 69 VGPRs unconstrained, 64 with 4 spills at 8 waves -- frame
// +0.6..1.1 % over 7 waves (A/B on one box: 4847 -> 4888); 8 rays per lane instead of 4: +0.5 %, refill threshold 8 instead of 16: +0.1 %.
// (Stacks deeper than 20 entries: LDS bounds the occupancy below 7 anyway, so no register bound there.)
#ifndef MCPT_REFILL_WAVES
#define MCPT_REFILL_WAVES 8
#endif
template <int STK, bool RETRY, bool SMALL>
__global__ __launch_bounds__(kBlock, (STK <= 20 ? MCPT_REFILL_WAVES : 1)) void k_trace_closest_refill(DevScene S, uint32_t n_host, const uint32_t *__restrict__ n_dev,
                                                                 const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                                 uint4 *__restrict__ hit, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    if constexpr (SMALL) {
        __shared__ SmallGeomLds small_geom;
        stage_small_geom(S, small_geom);
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const uint32_t wave = (uint32_t)tid >> 6;
    const uint32_t n = n_dev ? *n_dev : n_host;
    constexpr uint32_t kChunk = 64u * kRaysPerLane;
    for (uint32_t chunk = blockIdx.x * (kBlock / 64) + wave; (unsigned long long)chunk * kChunk < n; chunk += gridDim.x * (kBlock / 64)) {
        uint32_t next = chunk * kChunk;
        const uint32_t end = min(n, next + kChunk);
        int32_t my = -1;  // index of the ray this lane is tracing
        Ray r = make_ray(mk3(0, 0, 0), mk3(0, 0, 1));
        QRay qr = make_qray(S, r);
        TraceState st;
        trace_reset(st, false);
        Walk<STK, false, RETRY> w{StackMem{stk, nullptr, tid}};
        // Rays with a zero direction component (non-finite reciprocals: rare) need the NaN-faithful slab chain, which the loop below
        // does not carry.  They are traced first, by the generic path, with the whole wave at one place (a wave without such a ray
        // pays for four direction loads per lane, which the refills below then find in the cache); the refill skips them.
        for (uint32_t k = 0; k < kRaysPerLane; ++k) {
            const uint32_t idx = next + k * 64u + lane_id();
            bool odd = false;
            Ray ro = r;
            if (idx < end) {
                ro = make_ray(ld3(ray_o[idx]), ld3(ray_d[idx]));
                odd = !ray_is_plain(ro);
            }
            if (__any(odd)) {
                if (odd) {
                    const TraceResult tr = traverse<false, STK, RETRY, SMALL>(S, ro, 0.f, stk, tid);
                    if (RETRY && tr.dropped) retry_append(rl, idx);
                    else hit[idx] = pack_hit(tr.t, tr.prim, tr.mat_bits);
                }
            }
        }
        while (true) {
            // ---- finished lanes: store, refill
            const bool idle = w.idle();
            if (idle && my >= 0) {
                if (RETRY && st.dropped) retry_append(rl, (uint32_t)my);  // (k_retrace_closest traces it again)
                else hit[my] = pack_hit(st.best_t, st.best_prim, st.best_mat);
                my = -1;
            }
            const unsigned long long im = __ballot(idle);
            const uint32_t n_idle = (uint32_t)__popcll(im);
            if (next < end && n_idle >= kRefillMin) {
                const uint32_t idx = next + __builtin_amdgcn_mbcnt_hi((uint32_t)(im >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)im, 0u));
                if (idle && idx < end) {
                    r = make_ray(ld3(ray_o[idx]), ld3(ray_d[idx]));
                    if (ray_is_plain(r)) {  // (the others were traced before the loop: the lane stays idle and is refilled again)
                        my = (int32_t)idx;
                        qr = make_qray(S, r);
                        trace_reset(st, false);
                        walk_start<true, false>(w, S, r, INFINITY);
                    }
                }
                next += n_idle;
            }
            if (!__any(my >= 0)) {
                if (next < end) continue;  // every ray just handed out had been traced before the loop: hand out the next ones
                break;
            }
            // ---- one round of the speculative loop (traverse_loop): inner nodes until the vote, then the parked leaf
            while (true) {
                if (w.cur >= 0) descend<kClosest>(w, node_visit<(SMALL ? 2 : 1), true>(S, r, qr, w.cur), 0.f, st);
                if (__popcll(__ballot(w.leaf == kNoWork && w.cur >= 0)) <= kLeafVote) break;
            }
            leaf_step<kClosest>(w, S, r, 0.f, st);
        }
    }
}

// Queue position -> entry of the sharded shadow queue (Counters): positions [0, pf[K]) are the entries whose light sample was found, shard
// by shard; the next pw[K] positions the others.  pf / pw: exclusive prefix sums of the shards' counts (K + 1 values each, in LDS).
MCPT_DI void shadow_prefix(const Counters *counters, int next_idx, uint32_t *pf, uint32_t *pw) {  // all threads of the workgroup call it
    if (threadIdx.x < 64) {
        const uint32_t t = threadIdx.x;
        uint32_t cf = t < kShadowShards ? counters->n_shadow[next_idx][t].v : 0u;
        uint32_t cw = t < kShadowShards ? counters->n_shadow_w[next_idx][t].v : 0u;
        uint32_t sf = cf, sw = cw;
        for (int o = 1; o < 64; o <<= 1) {  // inclusive scan over the wave
            const uint32_t a = (uint32_t)__shfl_up((int)sf, o), b = (uint32_t)__shfl_up((int)sw, o);
            if ((int)t >= o) {
                sf += a;
                sw += b;
            }
        }
        if (t < kShadowShards) {
            pf[t] = sf - cf;
            pw[t] = sw - cw;
        }
        if (t == kShadowShards - 1u) {
            pf[kShadowShards] = sf;
            pw[kShadowShards] = sw;
        }
    }
    __syncthreads();
}
MCPT_DI uint32_t shadow_entry(const uint32_t *pf, const uint32_t *pw, uint32_t i, uint32_t region, bool &found) {
    const uint32_t nf = pf[kShadowShards];
    found = i < nf;
    const uint32_t *p = found ? pf : pw;
    const uint32_t j = found ? i : i - nf;
    uint32_t s = 0;  // the largest shard index with p[s] <= j (an empty shard shares its prefix with the next one: the later one wins)
    for (uint32_t step = kShadowShards / 2; step; step >>= 1)
        if (p[s + step] <= j) s += step;
    const uint32_t off = j - p[s];
    return found ? s * region + off : (s + 1u) * region - 1u - off;
}

// Shadow queue consumer: a fixed grid strides over the queue, whose length is only known on the device.
// Items [0, n_found) are the front of the arrays (light sample already found: occluder search only), the next n_window
// items are read from the back (window search first), so that the long occluder searches fill whole waves.
template <int STK, bool RETRY, bool SMALL>
__global__ __launch_bounds__(kBlock) void k_trace_shadow(DevScene S, const Counters *__restrict__ counters, int next_idx, uint32_t cap,
                                                         const float4 *__restrict__ shq_o, const float4 *__restrict__ shq_d,
                                                         float *__restrict__ contrib, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    __shared__ uint32_t pf[kShadowShards + 1], pw[kShadowShards + 1];
    const int tid = threadIdx.x;
    if constexpr (SMALL) {  // (made visible by the barrier at the end of shadow_prefix)
        __shared__ SmallGeomLds small_geom;
        stage_small_geom(S, small_geom);
    }
    shadow_prefix(counters, next_idx, pf, pw);
    const uint32_t n = pf[kShadowShards] + pw[kShadowShards];
    const uint32_t region = shadow_region(cap);
    for (uint32_t i = blockIdx.x * kBlock + tid; i < n; i += gridDim.x * kBlock) {
        bool found;
        const uint32_t e = shadow_entry(pf, pw, i, region, found);
        const float4 o = shq_o[e], d = shq_d[e];
        const Ray r = make_ray(ld3(o), ld3(d));
        const TraceResult tr = traverse<true, STK, RETRY, SMALL>(S, r, d.w, stk, tid, found);
        if (RETRY && tr.dropped) retry_append(rl, i);  // (undecided: k_retrace_shadow)
        else if (!tr.visible) contrib[__float_as_uint(o.w)] = 0.f;  // Scene.cpp:74-79: an invisible sample adds nothing
    }
}

// The shadow rays k_trace_shadow put on its retrace list (queue positions), with the scratch stack.
__global__ __launch_bounds__(kBlock) void k_retrace_shadow(DevScene S, const Counters *__restrict__ counters, int next_idx, uint32_t cap,
                                                           const float4 *__restrict__ shq_o, const float4 *__restrict__ shq_d,
                                                           float *__restrict__ contrib, RetryList rl) {
    __shared__ int32_t stk[1][kBlock];
    __shared__ uint32_t pf[kShadowShards + 1], pw[kShadowShards + 1];
    shadow_prefix(counters, next_idx, pf, pw);
    const uint32_t region = shadow_region(cap);
    const uint32_t n = min(*rl.count, rl.cap);
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const uint32_t i = rl.items[k];
        bool found;
        const uint32_t e = shadow_entry(pf, pw, i, region, found);
        const float4 o = shq_o[e], d = shq_d[e];
        const Ray r = make_ray(ld3(o), ld3(d));
        const TraceResult tr = traverse_scratch<true>(S, r, d.w, stk, threadIdx.x, found);
        if (!tr.visible) contrib[__float_as_uint(o.w)] = 0.f;
    }
    retry_finish(rl);
}

// ------------------------------------------------------------------------------------------------
// Path keys
// ------------------------------------------------------------------------------------------------
// s -> (position in the pixel list, sample index within the pass): s / s_pass and s % s_pass, by shift and mask when s_pass is a
// power of two (a uniform branch; a 32-bit division by a run-time value costs ~25 vector instructions per lane)
MCPT_DI void split_sample(const RenderConst &C, int q, uint32_t s, uint32_t &pl, uint32_t &k) {
    const uint32_t sp = (uint32_t)(q ? C.s_pass[1] : C.s_pass[0]);
    const int sh = q ? C.s_pass_shift[1] : C.s_pass_shift[0];
    if (sh >= 0) {
        pl = s >> sh;
        k = s & (sp - 1u);
    } else {
        pl = s / sp;
        k = s - pl * sp;
    }
}

MCPT_DI void path_key(const RenderConst &C, uint32_t pid, int q, RngKey &key, int &ch) {
    if (C.mode == 0) {
        const uint32_t s = pid / 3u;
        ch = (int)(pid - 3u * s);
        uint32_t pl, k;
        split_sample(C, q, s, pl, k);
        key.pixel = C.pixel_list ? C.pixel_list[pl] : pl;
        key.sample = (uint32_t)(q ? C.sample_offset[1] : C.sample_offset[0]) + k;
    } else {
        ch = C.key_channel[pid];
        key.pixel = C.key_pixel[pid];
        key.sample = C.key_sample[pid];
    }
    key.seed = C.seed;
    key.stream = (uint32_t)ch;
}

// ------------------------------------------------------------------------------------------------
// Camera rays, Renderer.cpp:44-76
// ------------------------------------------------------------------------------------------------
MCPT_DI f3 mat3_mul(const float *M, f3 v) {
    return mk3(M[0] * v.x + (M[1] * v.y + M[2] * v.z), M[3] * v.x + (M[4] * v.y + M[5] * v.z), M[6] * v.x + (M[7] * v.y + M[8] * v.z));
}

// The ray of pixel (i, j) for the four uniforms u: pixel jitter (u[0], u[1]) and lens sample (u[2] radius, u[3] angle).  kCentre: the caller
// passes u = {0.5, 0.5, 0, 0}, the pixel centre through the centre of the lens, and the lens angle theta = 0 takes the bits
// mcpt_sincosf(0.f) gives -- sin +0.f, cos 1.f (csrc/mcpt_fmath.h: kd = 0, r = 0, sn = r + r * (z * ps) = +0, cs = 1 + 0) -- without the
// call; every other expression is the one of the sampled ray, in its order.
template <bool kCentre>
MCPT_DI void camera_ray_from(const CameraConst &cam, int i, int j, const float (&u)[4], f3 &pos, f3 &dir) {
    const f3 eye = mk3(cam.eye[0], cam.eye[1], cam.eye[2]);
    const float x = (1 - 2 * (i + u[0]) / (float)cam.width) * cam.aspect * cam.scale;
    const float y = (1 - 2 * (j + u[1]) / (float)cam.height) * cam.scale;
    if (cam.use_dof) {
        const f3 focal_point = mk3(x, y, 1) * cam.focal_distance;
        const float r = cam.aperture_radius * sqrtf(u[2]);
        const float theta = 2 * kPi * u[3];
        float st = 0.f, ct = 1.f;
        if (!kCentre) mcpt_sincosf(theta, &st, &ct);  // Renderer.cpp:59-60
        const float dx = r * ct;
        const float dy = r * st;
        pos = eye + mat3_mul(cam.orient, mk3(dx, dy, 0));
        dir = normalized(focal_point - mk3(dx, dy, 0));
    } else {
        dir = normalized(mk3(x, y, 1));
        pos = eye;
    }
    dir = mat3_mul(cam.orient, dir);  // Renderer.cpp:76
}

// The camera ray of render sample k of pixel m: the uniforms of Philox stream 3.
MCPT_DI void camera_ray(const CameraConst &cam, uint32_t seed, uint32_t m, uint32_t k, f3 &pos, f3 &dir) {
    const int i = (int)(m % (uint32_t)cam.width), j = (int)(m / (uint32_t)cam.width);
    RngKey rk{seed, m, k, 3u};
    float u[4];
    rng_block(rk, 0u, 0u, u);
    camera_ray_from<false>(cam, i, j, u, pos, dir);
}

// The camera ray of sample s and its closest hit among the pixel's candidate primitives, when it has a short list (csrc/mcpt_cull.hip);
// returns false when the ray has to walk the tree.
MCPT_DI bool primary_ray(const DevScene &S, const CameraConst &cam, const RenderConst &C, int q, uint32_t s, f3 &pos, f3 &dir, TraceResult &tr) {
    uint32_t pl, ks;
    split_sample(C, q, s, pl, ks);
    const uint32_t m = C.pixel_list ? C.pixel_list[pl] : pl;
    const uint32_t k = (uint32_t)(q ? C.sample_offset[1] : C.sample_offset[0]) + ks;
    camera_ray(cam, C.seed, m, k, pos, dir);
    const int4 cd = C.pixel_cand ? C.pixel_cand[pl] : make_int4(kCandTraverse, 0, 0, 0);
    if (cd.x == kCandTraverse) return false;
    // every primitive a ray of this pixel can hit is in the list: test those, with the traversal's tie rule
    const Ray r = make_ray(pos, dir);
    const int32_t cs[4] = {cd.x, cd.y, cd.z, cd.w};
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        if (cs[q4] == kCandNone) continue;
        const int32_t prim = ~cs[q4];
        double t = 0;
        uint32_t mb;
        if (leaf_hit(S, prim, r, t, mb) && (t < tr.t || (t == tr.t && prim > tr.prim))) {
            tr.t = t;
            tr.prim = prim;
            tr.mat_bits = mb;
        }
    }
    return true;
}

// (k_primary and k_primary_retrace, which finish the closest hit of a new sample, follow direct_is_zero below: they call it.)

// mcpt_cast_rays: caller-supplied rays, one fresh record per ray; the rays are traced by k_trace_closest.
__global__ __launch_bounds__(kBlock) void k_generate_explicit(Wave next, Counters *c, int next_idx, uint32_t n) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j == 0) {
        c->n_paths[next_idx].v = n;
        c->n_rays[next_idx].v = n;
        c->free_head.v += n;  // the first n ring entries hold slots 0 .. n-1 (record j owns slot j)
    }
    if (j >= n) return;
    next.rec0[j] = make_uint4(j, j, kFresh, j);
}

__global__ __launch_bounds__(kBlock) void k_camera_rays(CameraConst cam, uint32_t seed, uint32_t n, const uint32_t *pixel,
                                                        const uint32_t *sample, float4 *o, float4 *d) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    f3 pos, dir;
    camera_ray(cam, seed, pixel[j], sample[j], pos, dir);
    o[j] = make_float4(pos.x, pos.y, pos.z, 0.f);
    d[j] = make_float4(dir.x, dir.y, dir.z, 0.f);
}

// The centre rays of pixels p0 .. p0+n-1 (mcpt_centre_rays; the feature passes with centre 1): one lane per pixel, no key arrays, no Philox.
__global__ __launch_bounds__(kBlock) void k_centre_rays(CameraConst cam, uint32_t p0, uint32_t n, float4 *o, float4 *d) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t m = p0 + j;
    const float u[4] = {0.5f, 0.5f, 0.f, 0.f};
    f3 pos, dir;
    camera_ray_from<true>(cam, (int)(m % (uint32_t)cam.width), (int)(m / (uint32_t)cam.width), u, pos, dir);
    o[j] = make_float4(pos.x, pos.y, pos.z, 0.f);
    d[j] = make_float4(dir.x, dir.y, dir.z, 0.f);
}

// `start`: initial value of the ring's head counter (0; a test hook starts it just below 2^32 to exercise the wrap).
__global__ __launch_bounds__(kBlock) void k_init_free(uint32_t *free_slots, Counters *c, uint32_t pool, uint32_t start, uint32_t mask) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < pool) free_slots[(start + j) & mask] = j;
    if (j == 0) {
        c->n_paths[0].v = c->n_paths[1].v = 0;
        c->n_rays[0].v = c->n_rays[1].v = 0;
        c->free_head.v = start;
        c->free_tail.v = start + pool;
        c->n_prays[0].v = c->n_prays[1].v = 0;
        c->n_brays[0].v = c->n_brays[1].v = 0;
        c->pc_samples.v = c->pc_rays.v = 0;
        c->live[0].v = c->live[1].v = 0;
        for (uint32_t k = 0; k < kShadowShards; ++k) {
            c->n_shadow[0][k].v = c->n_shadow[1][k].v = 0;
            c->n_shadow_w[0][k].v = c->n_shadow_w[1][k].v = 0;
        }
        c->n_direct[0].v = c->n_direct[1].v = 0;
        c->pushes.v = 0;
        c->overflow.v = 0;
        c->ended.v = 0;
        c->shared.v = 0;
        c->last_shadow = 0;
        c->tot_shaded = c->tot_direct = c->tot_shadow = c->tot_cont = c->tot_iterations = c->tot_pushes = c->tot_ended = c->tot_shared = c->tot_pc_samples = c->tot_pc_rays = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// Light sampling: Scene::sampleLight (Scene.cpp:23-37) -> MeshTriangle::Sample (Triangle.hpp:193-196)
// -> BVHAccel::Sample/getSample (BVH.cpp:118-135) -> Triangle::Sample (Triangle.hpp:71-76).
// u = {light choice, triangle pick, x, y}.  Returns false when no light was selected.
// ------------------------------------------------------------------------------------------------
MCPT_DI bool sample_light(const DevScene &S, const float u[4], f3 &x_l, f3 &n_l, f3 &emit, float &pdf, int32_t &prim) {
    float area_sum = S.light_area_sum;  // Scene.cpp:24-27: the sum over the emitters in insertion order (computed once, on the host)
    const float p = u[0] * area_sum;
    area_sum = 0.f;
    for (int k = 0; k < S.n_lights; ++k) {
        const LightRec L = S.lights[k];
        area_sum += L.area;
        if (p <= area_sum) {
            const MaterialRec &m = S.mats[L.mat];
            if (L.kind == MCPT_OBJ_MESH) {
                float pp = sqrtf(u[1]) * L.root_area;  // BVH.cpp:132 (the biased pick is reproduced)
                int32_t ref = L.root;
                while (ref >= 0) {  // BVH.cpp:118-129
                    const LightNode N = S.light_nodes[ref];
                    if (pp < N.left_area) {
                        ref = N.left;
                    } else {
                        pp = pp - N.left_area;
                        ref = N.right;
                    }
                }
                const LightTri T = S.light_tris[~ref];
                const float x = sqrtf(u[2]), y = u[3];  // Triangle.hpp:72
                const f3 v0 = mk3(T.v0[0], T.v0[1], T.v0[2]), v1 = mk3(T.v1[0], T.v1[1], T.v1[2]), v2 = mk3(T.v2[0], T.v2[1], T.v2[2]);
                x_l = (v0 * (1.0f - x) + v1 * (x * (1.0f - y))) + v2 * (x * y);
                n_l = mk3(T.n[0], T.n[1], T.n[2]);
                prim = T.prim;
                pdf = 1.0f / T.area;   // Triangle.hpp:75
                pdf *= T.area;         // BVH.cpp:121
                pdf /= L.root_area;    // BVH.cpp:134
                emit = mk3(m.emit[0], m.emit[1], m.emit[2]);  // Triangle.hpp:195
            } else {  // Sphere::Sample, Sphere.hpp:64-74 (leaves pos.emit untouched: zero here)
                const SphereRec s = S.spheres[L.root];
                const float theta = (float)(2.0 * (double)kPi * (double)u[2]), phi = kPi * u[3];
                float sph, cph, sth, cth;
                mcpt_sincosf(phi, &sph, &cph);
                mcpt_sincosf(theta, &sth, &cth);
                const f3 dir = mk3(cph, sph * cth, sph * sth);
                x_l = mk3(s.c[0], s.c[1], s.c[2]) + dir * s.radius;
                n_l = dir;
                prim = S.n_tri + L.root;
                pdf = 1.0f / L.area;
                emit = mk3(0.f, 0.f, 0.f);
            }
            return true;
        }
    }
    return false;
}

// ------------------------------------------------------------------------------------------------
// direct_is_zero: true only if EVERY light sample at this vertex has eval() == 0 exactly, so that
// Scene::directLighting (Scene.cpp:56-82) returns +0 whatever the draws and the visibilities are.
//   * no emitter in the scene;
//   * a conductor seen from inside: directLighting is called with isReflect = false (Scene.cpp:115-116) and
//     eval(.., false) returns 0 for both conductor types (Material.hpp:355-357,396-399);
//   * a Dirac BSDF (Material.hpp:375-403) is non-zero only if h.N >= 1 - EPSILON, which in float means h.N >= 1 - 1.01e-4 exactly (see the
//     total-internal-reflection rule below): the half vector lies within acos(1 - 1.01e-4) = 0.014213 rad of N, its part tangential to
//     N is at most s = 0.014212 of its length.  Reflection: ws is the mirror image of wo about h, so it lies within 2 * 0.014213 =
//     0.0285 rad of the mirror direction r = 2 (N.wo) N - wo, whatever the index.  Refraction (dielectric seen from inside, ws outside):
//     h is the direction of hv = -ws - ior wo, so |ws_t + ior wo_t| = |hv_t| <= s |hv| <= s (1 + ior) =: d.  The Snell direction has
//     r_t = -ior wo_t with |r_t| = sqrt(sin2) <= 0.9 behind the gate sin2 < 0.81, so ws_t lies within d of r_t in the unit disc.  Lifting
//     the straight segment from r_t to ws_t onto the hemisphere stretches it by at most 1 / sqrt(1 - rho^2) at radius rho <= 0.9 + t after
//     a length t, hence  angle(ws, r) <= asin(0.9 + d) - asin(0.9).  That bound GROWS with the index (ior 1.9: 0.106, 2.353: 0.126, 2.5:
//     0.1327, 3: 0.156, 5: 0.279 rad; beyond ior 6.03 it does not exist, 0.9 + d >= 1), so the constant tolerance holds up to a limit only:
//     the rule claims a refraction vertex for  0 < ior <= kConeMaxIor = 2.5  and declines above (and for an index that is not a number).
//     Every index below one is covered too: the proof uses nothing but |hv| <= 1 + ior.  The shipped presets reach 2.353 (iorA 1.3,
//     iorB 0.2, blue).  tests/test_direct_cone_cpu.py measures the farthest passing ws per index: 0.062 rad at 2.353, above 0.15 from 4.5.
//     Every light sample lies inside the cone of half-angle asin(R / D) around the direction to the centre of the
//     emitters' bounding sphere (radius R, distance D > 1.01 R).  If r is farther from that cone than the tolerance
//     (0.06 rad for reflection: 2.1x its bound; 0.15 rad for refraction: 1.13x its bound at ior 2.5, 0.017 rad to spare against float
//     roundings of 1e-6) no sample can give a non-zero eval.
//   * the half-space rule, for EVERY material (emitters_behind): all emitters lie behind the tangent plane of the vertex.
//     k_direct evaluates eval(ws, wo, n, isReflect = !inside) with ws = normalized(x_l - q) and inside = (wo.n < 0).  If the float value
//     ws.n it computes is < 0, every branch of mat_eval returns 0.f at its first test:
//       rough reflect  (wo.n >= 0): (ws.n)(wo.n) <= 0 -- negative, or -0 when wo.n is +-0 (then `inside` is false and the product is a zero);
//       Dirac reflect  (wo.n >= 0): the same product is the first operand of its `||`, h is never looked at;
//       rough refract  (wo.n <  0): conductors return 0 outright, dielectrics on (ws.n)(wo.n) >= 0 -- positive, or +0 on underflow;
//       Dirac refract  (wo.n <  0): conductors or the same product in its `||`, whatever h is.
//     Then c = emit * 0 * (ws.n) * (-ws.n_l) / dist^2 / pdf / n_dir is +-0 and not NaN: emit and pdf are finite and positive, the two
//     cosines are finite, and dist exceeds the slack, which is >= 1e-5 * R >= 1e-8 (the host pads R by 1e-3), so dist^2 is a normal
//     number.  Margin: the exact emitters lie within r of the centre c, and R = 1.001 r + 1e-3 >= r (mcpt_scene.cpp).  With unit
//     roundoff u = 2^-24, D = |L|, |n| <= 1 + 2u:  a sampled x_l leaves the emitters' hull by at most 6u (|c| + r) (three rounded
//     products and two sums of coordinates of that size; a sphere sample by less);  fl(x_l - q) errs by u |x_l - q|, its normalisation
//     by 4u per component and the dot product with n by 3u, together 8u (D + r) in units of length;  this test's own L = fl(c - q) and
//     n.L err by 4u D.  So the computed ws.n is negative whenever  n.L < -(r + 6u (|c| + r) + 12u (D + r)),  which
//     n.L < -(R + kHalfspaceSlack * (|c|_1 + R + |L|_1))  implies with kHalfspaceSlack = 1e-5 >= 10 x 12u = 7.2e-7 to spare (the
//     1-norms are upper bounds of |c| and D that cost no square root).  The distance gate D > 1.01 R of the cone rule stays in front.
//   * total internal reflection: a Dirac dielectric seen from inside (wo.N < 0) is evaluated with isReflect = false, and with
//     eta = ior when ws.N > 0 (ws.N <= 0 returns 0 on the product of the cosines).  h is the direction of hv = -ws - ior wo, whose part
//     tangential to N is at least ior |wo_t| - |ws| long, while |hv| <= |ws| + ior |wo|.  `h.N >= 1 - EPSILON` in float means
//     h.N >= 1 - 1.01e-4 exactly (h = normalized(hv) and its dot product with N err by less than 16u = 1e-6 together, u = 2^-24), so
//     |hv_t| <= sin(acos(1 - 1.01e-4)) |hv| = 0.014212 |hv|, i.e.  ior |wo_t| <= |ws| + 0.014212 (|ws| + ior |wo|).  ws is normalised in
//     k_direct and wo = -rd is a normalised ray direction: both are 1 to within 2u, and N is a normalised float normal.  With
//     sin2 = ior^2 |wo_t|^2 as computed below (relative error < 1e-6) no light sample can pass if
//     sin2 > 1.001 (1 + 0.0143 (1 + ior))^2:  0.0143 for 0.014212 and the factor 1.001 leave 6e-4 relative to the square root, 600 x
//     what the roundings and the 2u of the lengths can move it.  The rule does not look at the emitters, but it stays behind the
//     distance gate D > 1.01 R like the others: the gate is what keeps dist^2 a normal number, so that c = emit * 0 * ... is +-0 and
//     not NaN.  (Measured, profiles/direct_tir_stats.txt: 78 % of the Dirac vertices of the chess frame whose samples are all zero and
//     that the cone rule leaves are of this kind; the cone rule cannot see them, it needs a Snell direction.)
// tests: the -DMCPT_CHECK_DIRECT_SKIP build evaluates the skipped vertices anyway and counts non-zero contributions.
// ------------------------------------------------------------------------------------------------
MCPT_DI bool emitters_behind(const DevScene &S, f3 n, f3 L) {
    return dot(n, L) < -(S.light_plane[0] + S.light_plane[1] * (fabsf(L.x) + (fabsf(L.y) + fabsf(L.z))));
}

// The factor on the total-internal-reflection bound: 1.001, or what the checking build's knob MCPT_TIR_BOUND_SCALE made of it.
MCPT_DI float tir_bound_factor(const DevScene &S) {
#ifdef MCPT_TEST_HOOKS
    return S.tir_bound_factor;
#else
    return 1.001f;
#endif
}

// The cone rule's refraction half is proven up to this index (see above); beyond it the rule declines.
constexpr float kConeMaxIor = 2.5f;

// cos and sin of a cone tolerance and the slack on the cosine that goes with it: the constants, or those of the angle and the slack
// scaled by the checking build's knob MCPT_CONE_TOL_SCALE.  Returns the slack.
MCPT_DI float cone_tolerance(const DevScene &S, float angle, float c, float s, float &cm, float &sm) {
    cm = c;
    sm = s;
#ifdef MCPT_TEST_HOOKS
    if (S.cone_tol_scale != 1.f) {
        cm = cosf(angle * S.cone_tol_scale);
        sm = sinf(angle * S.cone_tol_scale);
        return 1e-3f * S.cone_tol_scale;
    }
#endif
    return 1e-3f;
}

// kHalfspace = false / kTir = false: without the half-space rule / the total-internal-reflection rule (the statistics build lists those
// vertices to count them, see k_direct).  by_tir (statistics and checking builds): the total-internal-reflection rule claims the vertex.
template <bool kHalfspace = true, bool kTir = true>
MCPT_DI bool direct_is_zero(const DevScene &S, const MaterialRec &m, f3 q, f3 n, f3 wo, bool inside, int ch, bool *by_tir = nullptr) {
    if (S.n_lights == 0) return true;
    const bool conductor = (m.type == MCPT_SMOOTH_CONDUCTOR || m.type == MCPT_ROUGH_CONDUCTOR);
    if (inside && conductor) return true;
    if (!kHalfspace && !m.isDirac) return false;
    const f3 L = mk3(S.light_center[0], S.light_center[1], S.light_center[2]) - q;
    const float D2 = dot(L, L), R = S.light_radius;
    if (!(D2 > R * R * 1.0201f)) return false;
    if (kHalfspace && emitters_behind(S, n, L)) return true;  // (cheap: before the cone test's square roots and divisions)
    if (!m.isDirac) return false;
    const float D = sqrtf(D2);
    const float sl = R / D, cl = sqrtf(1.0f - sl * sl);
    f3 r;
    float cm, sm, slack;
    if (!inside) {
        r = n * (2 * dot(n, wo)) - wo;
        slack = cone_tolerance(S, 0.06f, 0.99820054f, 0.05996400f, cm, sm);  // cos(0.06), sin(0.06)
    } else {
        const float ior = get_ior(m, ch);
        const float won = dot(wo, n);
        const f3 wot = wo - n * won;
        const float sin2 = ior * ior * dot(wot, wot);
        if (!(sin2 < 0.81f)) {  // no Snell direction for the cone test; beyond total internal reflection no sample can pass (see above)
            const float b = 1.0f + 0.0143f * (1.0f + ior);
            const bool tir = sin2 > tir_bound_factor(S) * (b * b);
            if (by_tir) *by_tir = tir;
            return kTir && tir;
        }
        if (!(ior <= kConeMaxIor)) return false;  // the 0.15 rad below is not proven for this index
        r = wot * (-ior) + n * sqrtf(1.0f - sin2);
        slack = cone_tolerance(S, 0.15f, 0.98877108f, 0.14943813f, cm, sm);  // cos(0.15), sin(0.15)
    }
    const float rl = norm(r);
    if (!(rl > 0.5f && rl < 2.0f)) return false;
    const float cos_a = dot(r, L) / (rl * D);
    return cos_a < (cl * cm - sl * sm) - slack;
}

// ------------------------------------------------------------------------------------------------
// New samples: what follows the camera ray (k_primary, k_primary_retrace)
// ------------------------------------------------------------------------------------------------
// block_alloc for per-lane counts of 0..3: the lane gets cnt[k] consecutive entries of counter k, index[k] is the first.  Two ballots per
// request (bit 0, bit 1), one where the caller says that the count is 0 or 1 (two_bits[k] false, a literal: the branch folds).
template <int N>
MCPT_DI void block_alloc_counts(BlockAllocShared &sh, const uint32_t (&cnt)[N], const bool (&two_bits)[N], uint32_t *const (&counter)[N],
                                uint32_t (&index)[N]) {
    static_assert(N <= kMaxAlloc, "too many allocation requests");
    const uint32_t n_waves = blockDim.x >> 6;
    const uint32_t lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t prefix[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned long long m0 = __ballot((cnt[k] & 1u) != 0u);
        uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
        uint32_t tot = (uint32_t)__popcll(m0);
        if (two_bits[k]) {
            const unsigned long long m1 = __ballot((cnt[k] & 2u) != 0u);
            pre += 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
            tot += 2u * (uint32_t)__popcll(m1);
        }
        prefix[k] = pre;
        if (lane == 0) sh.cnt[wave][k] = tot;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (threadIdx.x == (unsigned)k) {  // lanes 0..N-1 of wave 0 issue their atomics in the same instruction
            uint32_t total = 0;
            for (uint32_t w = 0; w < n_waves; ++w) {  // counts -> exclusive prefix over the waves, in place
                const uint32_t c = sh.cnt[w][k];
                sh.cnt[w][k] = total;
                total += c;
            }
            sh.base[k] = total ? atomicAdd(counter[k], total) : 0u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) index[k] = sh.base[k] + sh.cnt[wave][k] + prefix[k];
}

// The short path below is compiled out of the checking build and the statistics build: there k_shade lists vertices for k_direct that the
// regular build skips (need_direct, the marks of the rules), and a first vertex finished here would be missing from those lists.
#if defined(MCPT_CHECK_DIRECT_SKIP) || defined(MCPT_TRAVERSAL_STATS)
constexpr bool kPrimaryConductor = false;
#else
constexpr bool kPrimaryConductor = true;
#endif

// A new sample, from its camera ray on (all lanes of the workgroup call it; `valid` lanes hold a sample, `walk`: its closest hit is still to
// be found, by trace(ray); otherwise `tr` has it):
//   miss (Scene.cpp:88-95) ............ result[3 channels] = environment, no records
//   depth-0 emitter (Scene.cpp:102-107)  result[3 channels] = clamp(0,1, emission * |wo.n|), no records
//   smooth conductor, no direct light .. the short path, see below
//   any other surface ................. one ray + hit entry, three fresh path records, three clamp-stack slots
//
// The short path (RenderConst::primary_conductor).  A first hit on a smooth conductor seen from outside, where direct_is_zero holds for
// the three channels, is a vertex at which the channel lanes of k_shade do nothing that depends on the channel but one Philox block:
// mat_sample returns n, mat_fresnel 1, u0[3] < 1 always reflects, no light sample is evaluated, so p2 and wi are functions of (p, n, wo)
// alone and each channel either ends on roulette with l_dir = kr * 0 or continues along (p2, wi) with its own eval.  All of that is done
// here, in the lane that owns the sample, with k_shade's expressions: the vertex is set up once instead of three times (the textured
// floor's double-precision tri_hit included), and the lane walks the reflected ray itself -- the reflections of a pixel's samples are as
// coherent as its camera rays.  If that ray leaves the scene the surviving channels are finished with the expressions of k_shade's
// resolve branch; nothing leaves the kernel but three results.  If it hits, the ray and its hit go to a back entry of the ray arrays
// (k_trace_closest only walks the front) and every surviving channel gets the record k_shade would have written for it: depth 0,
// kNoDirect, kr, {eval, -1, 0, slot}, with a slot popped from the ring.  The survivors' records are adjacent and name one ray entry, so
// k_shade's ray sharing goes on applying at the next conductor.  (Seen from inside the conductor rule of direct_is_zero would hold as well;
// those rare samples take the ordinary path, which keeps l_dir's double-precision form out of this kernel.)
// The second walk is a second trip through the loop around the ONE trace() call, left early by the waves that have no reflected ray: a
// second inlined copy of the traversal loop costs the hot kernels 6-8 % (Walk, mcpt_traverse.h).
// A reflected ray that loses a stack entry (retry flavour) puts its sample on the retrace list like a camera ray that does: nothing of the
// short path has been written by then, and k_primary_retrace does the whole sample again.
// Counters: see Counters::pc_samples / pc_rays; the vertices finished here are added to `ended`, the records that ride on a sibling's
// ray to `shared`, so that every total of mcpt_stats is what k_shade would have made it.
// kNoEmitter (the indirect-only probes, mcpt_query_probes_ex: only instantiations of the sensor kernels select it): a first ray whose
// closest hit is an emitter contributes 0 in place of the depth-0 rule.
template <bool kCountPrims, bool kNoEmitter = false, class Trace>
MCPT_DI void primary_sample(const DevScene &S, const RenderConst &C, const Wave &next, int next_idx, int q, uint32_t s, bool valid, bool walk, f3 pos,
                            f3 dir, TraceResult tr, BlockAllocShared &sh, const RetryList &rl, Trace trace) {
    float *const result = q ? C.result[1] : C.result[0];
    bool go = valid && walk;
    // Registers: a lane on the short path keeps nothing of its camera ray.  From the end of the first trip on, (pos, dir) are its reflected
    // ray and, after the second trip, `tr` that ray's hit; what it carries besides is `spx` and, per surviving channel, eval and kr.
    uint32_t spx = 0;  // bit c: channel c survives roulette at the first vertex; kShort: the sample is on the short path
    constexpr uint32_t kShort = 8u;
    float ev[3] = {0.f, 0.f, 0.f}, kr[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int trip = 0; trip < (kPrimaryConductor ? 2 : 1); ++trip) {
        const Ray r = make_ray(pos, dir);
        if (go) {
            tr = trace(r);
            if (tr.dropped) {  // the sample is finished by k_primary_retrace, from its camera ray on (the scratch stack loses no entry)
                retry_append(rl, s);
                valid = false;
            }
        }
        if (trip != 0) break;
#ifdef MCPT_TRAVERSAL_STATS
        if (kCountPrims && S.dbg) {  // how many DIFFERENT primitives the 64 primary rays of a wave hit: what a wave-shared (packet) walk would have to visit at least
            const int myp = (valid && tr.prim >= 0) ? tr.prim : -2;
            bool first = myp >= 0;
            for (int l = 0; l < 64; ++l) {
                const int op = __shfl(myp, l);
                if ((uint32_t)l < lane_id() && op == myp) first = false;
            }
            const unsigned long long m = __ballot(first), mh = __ballot(myp >= 0);
            if (lane_id() == 0 && mh) {
                atomicAdd(&S.dbg[14], (unsigned long long)__popcll(m));
                atomicAdd(&S.dbg[15], 1ull);
            }
        }
#endif
        go = false;
        if (kPrimaryConductor && C.primary_conductor && valid && tr.prim >= 0 && !(tr.mat_bits >> 31)) {
            const MaterialRec &m = S.mats[(int)(tr.mat_bits & kMatIndexMask)];
            if (m.type == MCPT_SMOOTH_CONDUCTOR) {
                // ---- vertex set-up: k_shade's (the texture coordinates follow below, for the samples that need them)
                const f3 p = pos + dir * (float)tr.t;  // Triangle.hpp:245 / Ray.hpp:21; Sphere.hpp:40 (t0 is a float)
                f3 n;
                if (tr.prim < S.n_tri) {
                    const TriShade &ts = S.tri_shade[tr.prim];
                    n = mk3(ts.n[0], ts.n[1], ts.n[2]);
                } else {
                    const SphereRec &sr = S.spheres[tr.prim - S.n_tri];
                    n = normalized(p - mk3(sr.c[0], sr.c[1], sr.c[2]));
                }
                const f3 wo = -dir;
                // A smooth material's mat_sample is n whatever the two uniforms are (Scene.cpp:109), a conductor's kr is 1 (Scene.cpp:110)
                // and u0[3] = k / 2^24 with k < 2^24 is below it: isReflect (Scene.cpp:123), always.  So the next ray is one for the channels.
                // (kr here, in front of every store, with k_shade's arguments: the compiler still knows m.type and folds the call.)
                const f3 mfn = mat_sample(m, n, 0.f, 0.f);
#pragma unroll
                for (int c = 0; c < 3; ++c) kr[c] = mat_fresnel(m, dir, mfn, c);  // Scene.cpp:110
                const f3 qv = p + n * kEps;          // Scene.cpp:114
                const bool inside = dot(wo, n) < 0;  // Scene.cpp:115
                if (!inside && direct_is_zero(S, m, qv, n, wo, inside, 0) && direct_is_zero(S, m, qv, n, wo, inside, 1) &&
                    direct_is_zero(S, m, qv, n, wo, inside, 2)) {
                    spx = kShort;
                    // roulette: the keys of paths 3 s + c differ in the stream (= channel) alone
                    // (Registers: `s`, the pass parity and the seed go through an empty asm, so that the compiler cannot move what depends on
                    // neither the hit nor the trip in front of the loop and carry it through the traversal: the pixel's indices and
                    // addresses, the reciprocal of the pass size, the ten round keys of Philox and the address of the results cost the
                    // kernel 20 VGPRs.  The seed in a vector register: added to one in a scalar register the round constants would each
                    // need a vector register, and those are hoisted as well.)
                    uint32_t s_key = s, seed = C.seed;
                    int q_key = q;
                    asm volatile("" : "+v"(s_key), "+v"(seed), "+s"(q_key));
                    RngKey key;
                    int ch0;
                    path_key(C, 3u * s_key, q_key, key, ch0);
                    key.seed = seed;
#pragma unroll 1  // (three inlined Philox blocks side by side cost the kernel registers)
                    for (int c = 0; c < 3; ++c) {
                        key.stream = (uint32_t)c;
                        float u0[4];
                        rng_block(key, 0u, 0u, u0);
                        if (!(u0[2] >= C.rr_rate)) spx |= 1u << c;  // Scene.cpp:121,129
                    }
                    // a channel that ends on roulette: Scene.cpp:129-131 with l_dir = kr * 0 (Scene.cpp:116-119; k_shade's ends_here), returned
                    // unclamped; depth 0, nothing to unwind.  (Should the reflected ray lose a stack entry, k_primary_retrace writes it again.)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (!((spx >> c) & 1u)) (q_key ? C.result[1] : C.result[0])[(size_t)s_key * 3 + c] = kr[c] * 0.f;
                    if (spx & 7u) {
                        f2 uv{0.f, 0.f};
                        if (tr.prim < S.n_tri && (tr.mat_bits & kMatTextured)) {  // Triangle.hpp:248
                            const TriShade &ts = S.tri_shade[tr.prim];
                            double t3, u, v;
                            if (tri_hit(S.tri_geom[tr.prim], r, t3, u, v)) {
                                const float a = (float)(1 - u - v), b = (float)u, c = (float)v;
                                uv.x = a * ts.t0[0] + b * ts.t1[0] + c * ts.t2[0];
                                uv.y = a * ts.t0[1] + b * ts.t1[1] + c * ts.t2[1];
                            }
                        }
                        const f3 p2 = (dot(wo, mfn) < 0) ? (p - n * kEps) : (p + n * kEps);  // Scene.cpp:124-128
                        const f3 wi = mat_reflect(wo, mfn);                                  // Scene.cpp:132
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            if ((spx >> c) & 1u) ev[c] = mat_eval(m, wi, wo, n, c, uv, true);
                        pos = p2;
                        dir = wi;
                        go = true;
                    }
                }
            }
        }
        if (!__any(go)) break;
    }

    bool surface = false;  // the ordinary path
    uint32_t n_rec = 0;    // records the short path hands on (the reflected ray hit something)
    const uint32_t surv = spx & 7u;
    const bool sp = valid && (spx & kShort);
    if (sp) {
        if (surv == 0u) {  // every channel ended on roulette: written at set-up
        } else if (tr.prim >= 0) {
            n_rec = (uint32_t)__popc(surv);
        } else {
            const f3 env3 = sample_env(S, dir);  // Scene.cpp:145-149 (one look-up: the three channels read the components of one colour)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if ((surv >> c) & 1u) {
                    const float l_dir = kr[c] * 0.f;  // Scene.cpp:116-119 with l_dir == 0 (k_shade: the resolve of a kNoDirect record)
                    const float l_ind = comp(env3, c) * ev[c] * C.inv_rr;
                    result[(size_t)s * 3 + c] = clampf(0, 15, l_dir) + clampf(0, 5, l_ind);
                }
            }
        }
    } else if (valid) {
        if (tr.prim < 0) {
            const f3 env = sample_env(S, dir);
            result[(size_t)s * 3 + 0] = env.x;
            result[(size_t)s * 3 + 1] = env.y;
            result[(size_t)s * 3 + 2] = env.z;
        } else {
            const int mat = (int)(tr.mat_bits & kMatIndexMask);
            if constexpr (kNoEmitter) {
                if (tr.mat_bits >> 31) {
                    result[(size_t)s * 3 + 0] = 0.f;
                    result[(size_t)s * 3 + 1] = 0.f;
                    result[(size_t)s * 3 + 2] = 0.f;
                } else {
                    surface = true;
                }
            } else if (tr.mat_bits >> 31) {  // depth-0 emitter, Scene.cpp:102-107
                const MaterialRec &M = S.mats[mat];
                f3 n;
                if (tr.prim < S.n_tri) {
                    const TriShade ts = S.tri_shade[tr.prim];
                    n = mk3(ts.n[0], ts.n[1], ts.n[2]);
                } else {
                    const SphereRec sr = S.spheres[tr.prim - S.n_tri];
                    const f3 p = pos + dir * (float)tr.t;
                    n = normalized(p - mk3(sr.c[0], sr.c[1], sr.c[2]));
                }
                const float c = fabsf(dot(-dir, n));
                result[(size_t)s * 3 + 0] = clampf(0, 1, M.emit[0] * c);
                result[(size_t)s * 3 + 1] = clampf(0, 1, M.emit[1] * c);
                result[(size_t)s * 3 + 2] = clampf(0, 1, M.emit[2] * c);
            } else {
                surface = true;
            }
        }
    }
    const uint32_t n_surv = sp ? (uint32_t)__popc(surv) : 0u;
    const uint32_t n_slots = surface ? 3u : n_rec;
    // (The four statistics of the short path ride in the workgroup's one round of atomics although nobody takes an index from them: added
    // once per wave instead, 4 x as many atomics on four addresses, the frame lost 5 % and the other streams' kernels slowed down with it.)
    const uint32_t cnt[9] = {surface ? 1u : 0u,
                             n_slots,
                             C.track_live ? n_slots : 0u,  // that many more unfinished paths of this pass
                             n_rec,
                             n_rec ? 1u : 0u,
                             sp ? 3u - (C.first_fill ? 0u : n_rec) : 0u,          // first vertices shaded here that k_bookkeep does not see as records of list `next`
                             (C.share_rays && n_surv) ? n_surv - 1u : 0u,         // survivors beyond the first ride on its ray
                             n_surv ? (C.share_rays ? 1u : n_surv) : 0u,          // (sharing off: counted as a ray each, as k_shade would have stored them)
                             sp ? 1u : 0u};
    const bool two_bits[9] = {false, true, true, true, false, true, true, true, false};
    uint32_t *const ctr[9] = {&C.counters->n_prays[next_idx].v, &C.counters->free_head.v, &C.counters->live[q].v,
                              &C.counters->n_paths[next_idx].v, &C.counters->n_brays[next_idx].v, &C.counters->ended.v,
                              &C.counters->shared.v, &C.counters->pc_rays.v, &C.counters->pc_samples.v};
    uint32_t idx[9];
    block_alloc_counts<9>(sh, cnt, two_bits, ctr, idx);
    if (surface) {
        // the ray is already traced: it goes to the back of the ray arrays, away from the continuation rays that k_shade appends
        // at the front for k_trace_closest.  The three channel paths get no records: k_shade derives them from the sample entry.
        const uint32_t k = idx[0], ri = C.ray_cap - 1u - k;
        next.ray_o[ri] = make_float4(pos.x, pos.y, pos.z, 0.f);
        next.ray_d[ri] = make_float4(dir.x, dir.y, dir.z, 0.f);
        next.hit[ri] = pack_hit(tr.t, tr.prim, tr.mat_bits);
        next.fresh[k] = make_uint2(s | (q ? 0x80000000u : 0u), idx[1]);
    } else if (n_rec) {
        // the reflected ray, traced as well: a back entry of its own region, below those of the samples issued in this iteration
        const uint32_t ri = C.back2_base - idx[4];
        next.ray_o[ri] = make_float4(pos.x, pos.y, pos.z, 0.f);
        next.ray_d[ri] = make_float4(dir.x, dir.y, dir.z, 0.f);
        next.hit[ri] = pack_hit(tr.t, tr.prim, tr.mat_bits);
        uint32_t j = idx[3], ring = idx[1];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if ((surv >> c) & 1u) {
                const uint32_t slot = C.free_slots[ring & C.free_mask];
                next.rec0[j] = make_uint4(3u * s + (uint32_t)c, ri, kNoDirect | (q ? kPassBit : 0u), __float_as_uint(kr[c]));
                next.rec1[j] = make_float4(ev[c], -1.f, 0.f, __uint_as_float(slot));
                ++j;
                ++ring;
            }
        }
    }
}

// k_primary: Renderer.cpp:44-79 up to the first Scene::intersect of castRay (Scene.cpp:87) for new samples.
// The three channel paths of a sample share the primary ray, so it is generated and traced once.
template <int STK, bool RETRY, bool SMALL>
__global__ __launch_bounds__(kBlock) void k_primary(DevScene S, CameraConst cam, RenderConst C, Wave next, int next_idx, int q,
                                                    uint32_t first_sample, uint32_t n_samples, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    __shared__ BlockAllocShared sh;
    if constexpr (SMALL) {
        __shared__ SmallGeomLds small_geom;
        stage_small_geom(S, small_geom);
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const uint32_t j = blockIdx.x * kBlock + tid;
    const bool valid = j < n_samples;
    const uint32_t s = first_sample + j;
    f3 pos = mk3(0, 0, 0), dir = mk3(0, 0, 1);
    TraceResult tr{DBL_MAX, -1, 0u, false, false};
    const bool walk = valid && !primary_ray(S, cam, C, q, s, pos, dir, tr);
    primary_sample<true>(S, C, next, next_idx, q, s, valid, walk, pos, dir, tr, sh, rl,
                         [&](const Ray &r) { return traverse<false, STK, RETRY, SMALL>(S, r, 0.f, stk, tid); });
}

// The samples k_primary put on its retrace list: the same, with the scratch stack (a fixed grid strides over the list).
__global__ __launch_bounds__(kBlock) void k_primary_retrace(DevScene S, CameraConst cam, RenderConst C, Wave next, int next_idx, int q, RetryList rl) {
    __shared__ int32_t stk[1][kBlock];
    __shared__ BlockAllocShared sh;
    const uint32_t n = min(*rl.count, rl.cap);
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {  // uniform trip count per workgroup
        const uint32_t j = base + threadIdx.x;
        const bool valid = j < n;
        const uint32_t s = valid ? rl.items[j] : 0u;
        f3 pos = mk3(0, 0, 0), dir = mk3(0, 0, 1);
        TraceResult tr{DBL_MAX, -1, 0u, false, false};
        const bool walk = valid && !primary_ray(S, cam, C, q, s, pos, dir, tr);
        primary_sample<false>(S, C, next, next_idx, q, s, valid, walk, pos, dir, tr, sh, rl,
                              [&](const Ray &r) { return traverse_scratch<false>(S, r, 0.f, stk, threadIdx.x); });
        __syncthreads();  // `sh` is reused by the next round
    }
    retry_finish(rl);
}

// ------------------------------------------------------------------------------------------------
// Sensors (mcpt_query_radiance): k_primary and k_primary_retrace with the camera replaced by the caller's sensors.  Position `pl` of the
// list is sensor pl (no pixel list), so path_key gives the paths of its samples the key (seed, pl, sample, channel) by itself; a sensor
// has no candidate list, every first ray walks the tree.  Everything behind the first ray is primary_sample as it stands.
// ------------------------------------------------------------------------------------------------
MCPT_DI void sensor_sample_ray(const SensorConst &sn, const RenderConst &C, int q, uint32_t s, f3 &pos, f3 &dir) {
    uint32_t pl, ks;
    split_sample(C, q, s, pl, ks);
    sensor_ray(sn, C.seed, pl, (uint32_t)(q ? C.sample_offset[1] : C.sample_offset[0]) + ks, pos, dir);
}

// INDIRECT: primary_sample's kNoEmitter.
template <int STK, bool RETRY, bool SMALL, bool INDIRECT>
MCPT_DI void sensor_primary(DevScene &S, const SensorConst &sn, const RenderConst &C, const Wave &next, int next_idx, int q, uint32_t first_sample,
                            uint32_t n_samples, const RetryList &rl, int32_t (*stk)[kBlock], BlockAllocShared &sh) {
    if constexpr (SMALL) {
        __shared__ SmallGeomLds small_geom;
        stage_small_geom(S, small_geom);
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const uint32_t j = blockIdx.x * kBlock + tid;
    const bool valid = j < n_samples;
    const uint32_t s = first_sample + j;
    f3 pos = mk3(0, 0, 0), dir = mk3(0, 0, 1);
    const TraceResult tr{DBL_MAX, -1, 0u, false, false};
    if (valid) sensor_sample_ray(sn, C, q, s, pos, dir);  // (a lane past the end holds no sample: its index names no sensor)
    primary_sample<true, INDIRECT>(S, C, next, next_idx, q, s, valid, valid, pos, dir, tr, sh, rl,
                                   [&](const Ray &r) { return traverse<false, STK, RETRY, SMALL>(S, r, 0.f, stk, tid); });
}

template <int STK, bool RETRY, bool SMALL>
__global__ __launch_bounds__(kBlock) void k_sensor_primary(DevScene S, SensorConst sn, RenderConst C, Wave next, int next_idx, int q,
                                                           uint32_t first_sample, uint32_t n_samples, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    __shared__ BlockAllocShared sh;
    sensor_primary<STK, RETRY, SMALL, false>(S, sn, C, next, next_idx, q, first_sample, n_samples, rl, stk, sh);
}

template <int STK, bool RETRY, bool SMALL>
__global__ __launch_bounds__(kBlock) void k_sensor_primary_indirect(DevScene S, SensorConst sn, RenderConst C, Wave next, int next_idx, int q,
                                                                    uint32_t first_sample, uint32_t n_samples, RetryList rl) {
    __shared__ int32_t stk[STK][kBlock];
    __shared__ BlockAllocShared sh;
    sensor_primary<STK, RETRY, SMALL, true>(S, sn, C, next, next_idx, q, first_sample, n_samples, rl, stk, sh);
}

template <bool INDIRECT>
MCPT_DI void sensor_primary_retrace(const DevScene &S, const SensorConst &sn, const RenderConst &C, const Wave &next, int next_idx, int q, const RetryList &rl,
                                    int32_t (*stk)[kBlock], BlockAllocShared &sh) {
    const uint32_t n = min(*rl.count, rl.cap);
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {  // uniform trip count per workgroup
        const uint32_t j = base + threadIdx.x;
        const bool valid = j < n;
        const uint32_t s = valid ? rl.items[j] : 0u;
        f3 pos = mk3(0, 0, 0), dir = mk3(0, 0, 1);
        const TraceResult tr{DBL_MAX, -1, 0u, false, false};
        if (valid) sensor_sample_ray(sn, C, q, s, pos, dir);
        primary_sample<false, INDIRECT>(S, C, next, next_idx, q, s, valid, valid, pos, dir, tr, sh, rl,
                                        [&](const Ray &r) { return traverse_scratch<false>(S, r, 0.f, stk, threadIdx.x); });
        __syncthreads();  // `sh` is reused by the next round
    }
    retry_finish(rl);
}

__global__ __launch_bounds__(kBlock) void k_sensor_primary_retrace(DevScene S, SensorConst sn, RenderConst C, Wave next, int next_idx, int q, RetryList rl) {
    __shared__ int32_t stk[1][kBlock];
    __shared__ BlockAllocShared sh;
    sensor_primary_retrace<false>(S, sn, C, next, next_idx, q, rl, stk, sh);
}

__global__ __launch_bounds__(kBlock) void k_sensor_primary_retrace_indirect(DevScene S, SensorConst sn, RenderConst C, Wave next, int next_idx, int q,
                                                                            RetryList rl) {
    __shared__ int32_t stk[1][kBlock];
    __shared__ BlockAllocShared sh;
    sensor_primary_retrace<true>(S, sn, C, next, next_idx, q, rl, stk, sh);
}

// mcpt_sensor_rays: the first ray of (sensor[j], sample[j]), one lane per pair.
__global__ __launch_bounds__(kBlock) void k_sensor_rays(SensorConst sn, uint32_t seed, uint32_t n, const uint32_t *__restrict__ sensor,
                                                        const uint32_t *__restrict__ sample, float4 *__restrict__ o, float4 *__restrict__ d) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    f3 pos, dir;
    sensor_ray(sn, seed, sensor[j], sample[j], pos, dir);
    o[j] = make_float4(pos.x, pos.y, pos.z, 0.f);
    d[j] = make_float4(dir.x, dir.y, dir.z, 0.f);
}

// The variance of each channel's mean from the moments k_accumulate<true> summed (s1 = sum v, s2 = sum v*v, in double and in sample
// order), one lane per (sensor, channel): max(s2/n - (s1/n)^2, 0) * n/(n-1) / n in double, rounded once to float.
__global__ __launch_bounds__(kBlock) void k_sensor_variance(uint32_t n3, int32_t spp, const double *__restrict__ moments, float *__restrict__ variance) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n3) return;
    const uint32_t i = g / 3u, c = g - 3u * i;
    const double n = (double)spp;
    const double s1 = moments[(size_t)i * 6 + c], s2 = moments[(size_t)i * 6 + 3 + c];
    const double mean = s1 / n;
    const double diff = s2 / n - mean * mean;
    const double pop = diff < 0.0 ? 0.0 : diff;  // (a NaN stays one: a sensor whose radiance is NaN has no variance to report)
    variance[g] = (float)(pop * n / (n - 1.0) / n);
}

// ------------------------------------------------------------------------------------------------
// k_shade: Scene::castRay (Scene.cpp:85-184) turned inside out.
//
// The recursion  L_d = clamp(0,15,l_dir_d) + clamp(0,5, L_{d+1} * f_d)  is not multiplicative (per-level
// clamps, unclamped early returns), so a path cannot carry a scalar throughput.  Each level that
// recurses pushes {clamp(0,15,l_dir), eval, |wo.n| (or -1 for Dirac), pdf} on a per-path clamp stack in
// HBM; when the path ends the stack is unwound with exactly the reference's float expressions.
// ------------------------------------------------------------------------------------------------
MCPT_DI float unwind(const RenderConst &C, uint32_t slot, uint32_t depth, float X) {
    for (int lvl = (int)depth - 1; lvl >= 0; --lvl) {
        const float4 e = C.stack[(size_t)lvl * C.pool + slot];
        float l_ind;
        if (e.z < 0.f) l_ind = X * e.y * C.inv_rr;            // Scene.cpp:137-138,164-165 (isDirac)
        else l_ind = X * e.y * e.z / e.w * C.inv_rr;           // Scene.cpp:140-143,167-170
        X = e.x + clampf(0, 5, l_ind);                         // Scene.cpp:180-183
    }
    return X;
}

__global__ __launch_bounds__(kShadeBlock, 8) void k_shade(DevScene S, RenderConst C, Wave cur, Wave next, Scratch Xs, int cur_idx) {
    __shared__ BlockAllocShared sh;
#ifdef MCPT_TRAVERSAL_STATS
    const long long t_wave0 = clock64();
#endif
    const uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x;
    // the grid is an upper bound; the list lengths live on the device.  Lanes [0, n_rec) take the records of the list, the next
    // 3 * n_new lanes the new samples (one lane per channel path).
    const uint32_t n_rec = C.counters->n_paths[cur_idx].v, n_new = C.counters->n_prays[cur_idx].v;
    const bool valid = i < n_rec + 3u * n_new;
    const bool is_new = valid && i >= n_rec;
    const int next_idx = cur_idx ^ 1;

    uint32_t pid = 0, slot = 0, depth = 0, ray_idx = 0;
    int ch = 0, pq = 0;  // pq: parity of the pass the path belongs to
    RngKey key{0, 0, 0, 0};
    bool do_shade = false, finished = false, pushed = false, overflow = false;
    float X = 0.f;
    double hit_t = 0;
    int32_t hit_prim = -1;
    uint32_t hit_mat = 0;
    float4 ro4 = make_float4(0.f, 0.f, 0.f, 0.f), rd4 = make_float4(0.f, 0.f, 1.f, 0.f);

    if (valid) {
        uint4 r0;
        if (is_new) {  // a new sample: {sample | parity, ring position of its slots}; its ray is entry ray_cap-1-k
            const uint32_t k = (i - n_rec) / 3u, c = (i - n_rec) % 3u;
            const uint2 f = cur.fresh[k];
            r0 = make_uint4((f.x & 0x7fffffffu) * 3u + c, C.ray_cap - 1u - k, kFresh | ((f.x >> 31) ? kPassBit : 0u),
                            C.free_slots[(f.y + c) & C.free_mask]);
        } else {
            r0 = cur.rec0[i];
        }
        const uint32_t flags = r0.z;
        float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f);
        pid = r0.x;
        depth = r0.z & 0xffffu;
        if (flags & kTerminate) {  // no ray, no BSDF terms: the record is rec0 alone, with the slot where the ray index would be
            slot = r0.y;
        } else if (flags & kFresh) {  // no BSDF terms either: rec0 alone, with the slot where kr would be
            ray_idx = r0.y;
            slot = r0.w;
        } else {
            r1 = cur.rec1[i];
            ray_idx = r0.y;
            slot = __float_as_uint(r1.w);
        }
        pq = (int)((flags >> 20) & 1u);
        // everything the record points to is requested at once, before any of it is looked at: the hit, and the ray itself (a surface hit
        // needs both vectors, a miss the direction: only a path that ends on the depth limit asks for nothing)
        uint4 h = make_uint4(0u, 0u, 0xffffffffu, 0u);
        if (!(flags & kTerminate)) {
            h = cur.hit[ray_idx];
            ro4 = cur.ray_o[ray_idx];
            rd4 = cur.ray_d[ray_idx];
        }
        path_key(C, pid, pq, key, ch);

        if (!(flags & kFresh)) {
            // ---- resolve the pending vertex: Scene.cpp:114-119 (l_dir), 129-149 / 156-176 (l_ind)
            float dl = 0.f;
            if (!(flags & kNoDirect)) {
                if (C.n_dir == 4) {  // one 16-byte request instead of four dwords; same sum, same order (Scene.cpp:76 `l_dir +=`)
                    const float4 c4 = reinterpret_cast<const float4 *>(cur.contrib)[i];
                    dl = (((dl + c4.x) + c4.y) + c4.z) + c4.w;
                } else if ((C.n_dir & 3) == 0) {  // (32 light samples, as the README labels the chess render: 8 requests instead of 32)
                    const float4 *c4 = reinterpret_cast<const float4 *>(cur.contrib) + (size_t)i * (uint32_t)(C.n_dir >> 2);
                    for (int k = 0; k < (C.n_dir >> 2); ++k) {
                        const float4 v = c4[k];
                        dl = (((dl + v.x) + v.y) + v.z) + v.w;
                    }
                } else {
                    for (int k = 0; k < C.n_dir; ++k) dl += cur.contrib[(size_t)i * C.n_dir + k];  // Scene.cpp:76 `l_dir +=`, in order
                }
            }
            const float kr = __uint_as_float(r0.w);
            const float l_dir = (flags & kInside) ? (float)((1. - (double)kr) * (double)dl) : kr * dl;
            if (flags & kTerminate) {
                X = l_dir;  // Scene.cpp:129-131,156-158: returned unclamped
                finished = true;
            } else {
                hit_t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
                hit_prim = (int32_t)h.z;
                hit_mat = h.w;
                const bool surface = hit_prim >= 0 && !(hit_mat >> 31);  // Scene.cpp:135,162
                if (!surface) {
                    const f3 wi = ld3(rd4);
                    const float env = comp(sample_env(S, wi), ch);  // Scene.cpp:145-149,172-176
                    const float l_ind = env * r1.x * C.inv_rr;
                    X = clampf(0, 15, l_dir) + clampf(0, 5, l_ind);
                    finished = true;
                } else if ((int)depth >= C.max_depth) {
                    X = clampf(0, 15, l_dir);  // clamp stack exhausted: drop the indirect term, report it
                    finished = true;
                    overflow = true;
                } else {
                    C.stack[(size_t)depth * C.pool + slot] = make_float4(clampf(0, 15, l_dir), r1.x, r1.y, r1.z);
                    depth += 1;
                    pushed = true;
                    do_shade = true;
                }
            }
        } else {
            hit_t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
            hit_prim = (int32_t)h.z;
            hit_mat = h.w;
            if (hit_prim < 0) {
                X = comp(sample_env(S, ld3(rd4)), ch);  // Scene.cpp:88-95
                finished = true;
            } else {
                do_shade = true;  // the depth-0 emitter test needs the normal; done below
            }
        }
    }

    // ---- vertex set-up for lanes that shade
    f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1), p = mk3(0, 0, 0), n = mk3(0, 0, 1), wo = mk3(0, 0, -1);
    f2 uv{0.f, 0.f};
    const int mat_id = (int)(hit_mat & kMatIndexMask);
    if (do_shade) {
        ro = ld3(ro4);
        rd = ld3(rd4);
        if (hit_prim < S.n_tri) {
            const TriShade ts = S.tri_shade[hit_prim];
            n = mk3(ts.n[0], ts.n[1], ts.n[2]);
            p = ro + rd * (float)hit_t;  // Triangle.hpp:245 / Ray.hpp:21
            if (hit_mat & kMatTextured) {  // Triangle.hpp:248: recompute the barycentrics of the recorded hit (the flag travels with the hit)
                double t, u, v;
                const Ray rr = make_ray(ro, rd);
                if (tri_hit(S.tri_geom[hit_prim], rr, t, u, v)) {
                    const float a = (float)(1 - u - v), b = (float)u, c = (float)v;
                    uv.x = a * ts.t0[0] + b * ts.t1[0] + c * ts.t2[0];
                    uv.y = a * ts.t0[1] + b * ts.t1[1] + c * ts.t2[1];
                }
            }
        } else {
            const SphereRec s = S.spheres[hit_prim - S.n_tri];
            p = ro + rd * (float)hit_t;  // Sphere.hpp:40 (t0 is a float)
            n = normalized(p - mk3(s.c[0], s.c[1], s.c[2]));
        }
        wo = -rd;
        if (depth == 0 && (hit_mat >> 31)) {  // Scene.cpp:102-107
            X = clampf(0, 1, S.mats[mat_id].emit[ch] * fabsf(dot(wo, n)));
            finished = true;
            do_shade = false;
        }
    }

    // ---- finish: unwind the clamp stack and publish the path value
    if (finished) {
        X = unwind(C, slot, depth, X);
        (pq ? C.result[1] : C.result[0])[pid] = X;
    }

    // ---- shade the new vertex: Scene.cpp:109-128,150-155
    const MaterialRec m = S.mats[mat_id];
    float u0[4] = {0.f, 0.f, 1.f, 0.f};
    if (do_shade) rng_block(key, depth, 0u, u0);
    const bool has_cont = do_shade && !(u0[2] >= C.rr_rate);  // Scene.cpp:121,129,156

    const f3 q = p + n * kEps;                       // Scene.cpp:114
    const bool inside = dot(wo, n) < 0;              // Scene.cpp:115
#if defined(MCPT_TRAVERSAL_STATS) && !defined(MCPT_CHECK_DIRECT_SKIP)
    // statistics build: the vertices only the half-space rule or only the total-internal-reflection rule would skip stay on the list,
    // marked, so that k_direct can count them
    bool by_tir = false, past_gate = false;  // past_gate: a Dirac dielectric seen from inside beyond the refraction gate sin2 < 0.81
    const bool zero_direct = do_shade && direct_is_zero<false, false>(S, m, q, n, wo, inside, ch, &by_tir);
    if (do_shade && m.isDirac && inside) {
        const f3 wot = wo - n * dot(wo, n);
        past_gate = !(get_ior(m, ch) * get_ior(m, ch) * dot(wot, wot) < 0.81f);
    }
#elif defined(MCPT_CHECK_DIRECT_SKIP)
    bool by_tir = false;  // claimed by the total-internal-reflection rule (k_direct's counters)
    const bool past_gate = false;
    const bool zero_direct = do_shade && direct_is_zero(S, m, q, n, wo, inside, ch, &by_tir);
#else
    const bool by_tir = false, past_gate = false;
    const bool zero_direct = do_shade && direct_is_zero(S, m, q, n, wo, inside, ch);
#endif
#if defined(MCPT_TRAVERSAL_STATS) || defined(MCPT_CHECK_DIRECT_SKIP)
    bool behind = false;  // the half-space rule on its own (k_direct's counters)
    if (do_shade && S.n_lights > 0) {
        const f3 L = mk3(S.light_center[0], S.light_center[1], S.light_center[2]) - q;
        behind = dot(L, L) > S.light_radius * S.light_radius * 1.0201f && emitters_behind(S, n, L);
    }
#else
    const bool behind = false;
#endif
#ifdef MCPT_CHECK_DIRECT_SKIP
    const bool need_direct = do_shade;  // checking build: evaluate the skipped vertices too (k_direct counts violations)
#else
    const bool need_direct = do_shade && !zero_direct;
#endif

    // one round of block-aggregated atomics: released slots, next-list records, continuation rays, the direct-
    // lighting work list, statistics.  The BSDF sampling below does not need the indices and runs while the
    // atomics are in flight.
    // A vertex where roulette ends the path and whose light samples all contribute zero returns l_dir = kr * 0
    // (Scene.cpp:129-131,156-158) with nothing left to wait for: the path is finished here instead of leaving a
    // record for the next iteration.
    const bool ends_here = do_shade && !has_cont && !need_direct;
    const bool done = finished || ends_here;
    // Shared continuation rays.  The channel paths of a sample read one incoming ray (the same ray_idx): the same p, n, wo and material.
    // At a smooth conductor the next ray does not depend on the channel either: mat_sample returns n, mat_fresnel exactly 1, u0[3] < 1
    // always reflects, so p2 and wi are functions of (p, n, wo) alone; only the roulette draw u0[2] differs.  The surviving siblings
    // therefore continue on ONE ray: the lowest such lane (the leader) requests and stores it, the others (followers, `lead` lanes above
    // it) point their records at it.  Siblings sit in adjacent lanes (fresh triples are lanes n_rec + 3k + c, compaction keeps the lane
    // order of a workgroup) and a ray has at most three records, so lanes -1 and -2 are all there is to look at; a group cut by a wave
    // boundary does not share.  Next iteration the records carry the same ray_idx again and the rule applies as long as they keep
    // meeting smooth conductors.  (Explicit paths, mcpt_cast_rays, have one ray per record: nothing ever matches.)
    uint32_t lead = 0;
    {
        const bool cand = has_cont && C.share_rays && m.type == MCPT_SMOOTH_CONDUCTOR;
        const uint32_t mine = cand ? ray_idx : 0xffffffffu;  // (0xffffffff is never a ray index: ray_cap entries, 32-bit)
        const uint32_t up1 = (uint32_t)__shfl_up((int)mine, 1), up2 = (uint32_t)__shfl_up((int)mine, 2);  // (lanes 0 / 0, 1 get their own value back)
        if (cand) lead = (lane_id() >= 2u && up2 == mine) ? 2u : ((lane_id() >= 1u && up1 == mine) ? 1u : 0u);
    }
    const bool want[10] = {done, do_shade && !ends_here, has_cont && lead == 0u, need_direct, pushed, overflow, done && C.track_live && pq == 0,
                           done && C.track_live && pq == 1, ends_here, lead != 0u};
    const uint32_t mult[10] = {1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u};
    uint32_t *const ctr[10] = {&C.counters->free_tail.v, &C.counters->n_paths[next_idx].v, &C.counters->n_rays[next_idx].v,
                               &C.counters->n_direct[next_idx].v, &C.counters->pushes.v, &C.counters->overflow.v,
                               &C.counters->live[0].v, &C.counters->live[1].v, &C.counters->ended.v, &C.counters->shared.v};
    const bool sub[10] = {false, false, false, false, false, false, true, true, false, false};
    uint32_t prefix[10], idx[10];
#ifdef MCPT_TRAVERSAL_STATS
    const long long tb0 = clock64();
#endif
    block_alloc_begin<10>(sh, want, mult, ctr, sub, prefix);
#ifdef MCPT_TRAVERSAL_STATS
    const long long tb1 = clock64();
#endif

    float kr = 0.f, ev = 0.f, aw = 0.f, pd = 0.f;
    f3 p2 = mk3(0, 0, 0), wi = mk3(0, 0, 1);
    if (do_shade) {
        const f3 mfn = mat_sample(m, n, u0[0], u0[1]);   // Scene.cpp:109
        kr = mat_fresnel(m, rd, mfn, ch);                // Scene.cpp:110
        const bool isReflect = u0[3] < kr;               // Scene.cpp:123
        if (isReflect) p2 = (dot(wo, mfn) < 0) ? (p - n * kEps) : (p + n * kEps);  // Scene.cpp:124-128
        else p2 = (dot(wo, mfn) < 0) ? (p + n * kEps) : (p - n * kEps);            // Scene.cpp:151-155
        if (has_cont) {
            wi = isReflect ? mat_reflect(wo, mfn) : mat_refract(m, rd, mfn, ch);   // Scene.cpp:132,159
            if (m.isDirac) {
                ev = mat_eval(m, wi, wo, n, ch, uv, isReflect);
                aw = -1.f;
            } else {
                aw = fabsf(dot(wo, n));
                mat_eval_pdf_rough(m, wi, wo, n, ch, uv, isReflect, ev, pd);  // Material::eval and ::pdf sharing h and D
            }
        }
    }

#ifdef MCPT_TRAVERSAL_STATS
    const long long tb2 = clock64();
#endif
    block_alloc_end<10>(sh, mult, prefix, idx);
    // a follower takes its leader's ray entry (read while every lane is still here: the returns are below)
    const uint32_t rj = (uint32_t)__shfl((int)idx[2], (int)(lane_id() - lead));
#ifdef MCPT_TRAVERSAL_STATS
    if (S.dbg && lane_id() == 0) {  // cycles of this wave: in block_alloc_begin (ballots + first barrier), in block_alloc_end (second barrier), since its start
        const long long tb3 = clock64();
        atomicAdd(&S.dbg[20], (unsigned long long)(tb1 - tb0));
        atomicAdd(&S.dbg[21], (unsigned long long)(tb3 - tb2));
        atomicAdd(&S.dbg[22], (unsigned long long)(tb3 - t_wave0));
        atomicAdd(&S.dbg[23], 1ull);
    }
    if (S.dbg) {  // material divergence: how many of the four material types the shading lanes of this wave hold
        int nd = 0;
        for (int t = 0; t < 4; ++t) nd += __ballot(do_shade && m.type == t) != 0ull ? 1 : 0;
        const unsigned long long ms = __ballot(do_shade);
        if (lane_id() == 0) {
            atomicAdd(&S.dbg[24 + nd], 1ull);
            atomicAdd(&S.dbg[29], (unsigned long long)__popcll(ms));
        }
    }
#endif
    if (done) C.free_slots[idx[0] & C.free_mask] = slot;
    if (!do_shade) return;
    if (ends_here) {
        const float l_dir = inside ? (float)((1. - (double)kr) * (double)0.f) : kr * 0.f;  // Scene.cpp:116-119 with l_dir == 0
        (pq ? C.result[1] : C.result[0])[pid] = unwind(C, slot, depth, l_dir);
        return;
    }
    const uint32_t j = idx[1], dj = idx[3];

    if (need_direct) {  // work-list entry for k_direct (Scene::directLighting runs there, one lane per light sample)
        Xs.vtx0[dj] = make_float4(q.x, q.y, q.z, uv.x);
        Xs.vtx1[dj] = make_float4(n.x, n.y, n.z, uv.y);
        Xs.vtx2[dj] = make_float4(wo.x, wo.y, wo.z, __uint_as_float((uint32_t)mat_id | ((uint32_t)ch << 16) | (inside ? (1u << 18) : 0u) |
                                                                    (zero_direct ? (1u << 19) : 0u) | (behind ? (1u << 20) : 0u) | (by_tir ? (1u << 21) : 0u) |
                                                                    (past_gate ? (1u << 22) : 0u)));
        Xs.vtx_j[dj] = j;
    }
    uint32_t flags = depth | (inside ? kInside : 0u) | (need_direct ? 0u : kNoDirect) | (pq ? kPassBit : 0u);
    if (has_cont) {
        if (lead == 0u) {  // (a follower's p2 and wi are its leader's, bit for bit: see `lead`)
            next.ray_o[rj] = make_float4(p2.x, p2.y, p2.z, 0.f);
            next.ray_d[rj] = make_float4(wi.x, wi.y, wi.z, 0.f);
        }
    } else {
        flags |= kTerminate;
    }
    next.rec0[j] = make_uint4(pid, has_cont ? rj : slot, flags, __float_as_uint(kr));
    if (has_cont) next.rec1[j] = make_float4(ev, aw, pd, __uint_as_float(slot));
}

// ------------------------------------------------------------------------------------------------
// k_direct: Scene::directLighting (Scene.cpp:56-82), one lane per (shaded vertex, light sample).
//   c = emit * eval(ws, wo, n) * (ws.n) * (-ws.n_light) / dist^2 / pdf / n_dir_sample          (Scene.cpp:76-79)
// is stored in contrib[]; samples with c != 0 go to the shadow queue.  A sample whose contribution is exactly
// +-0 (Dirac BSDFs away from the mirror direction, back-facing configurations: Material.hpp:338,356,382,397)
// adds nothing to l_dir whether it is visible or not, so it casts no shadow ray; a NaN contribution is not zero
// and is traced.
// ------------------------------------------------------------------------------------------------
// (7 waves per SIMD: 70 VGPRs, nothing spilled.  With the former workgroup-wide queue allocation 8 had been better -- more waves to
// hide its barriers; with the per-wave allocation below, 8 spills 27 registers: frame 4880 against 5000.)
#ifndef MCPT_DIRECT_WAVES
#define MCPT_DIRECT_WAVES 7
#endif
// SMALL: light tables, materials and the triangles / spheres in LDS (small scenes, see SmallGeomLds).
// (Round 3, measured and not kept: for these scenes, where 75-86 % of the light samples do cast a ray, the shadow query run right here in
// the lane that made the sample -- no queue entry, no prefix sums, no second launch.  Correct, and slower: cornell_rc 784^2 spp 256
// 427 against 475 Msamples/s, DEMO 1080p 755 against 857: the fused kernel took 288 ms where k_direct + k_trace_shadow take 112 + 137
// side by side with the other chains.)
template <bool SMALL>
__global__ __launch_bounds__(kBlock, MCPT_DIRECT_WAVES) void k_direct(DevScene S, RenderConst C, Wave next, Scratch Xs, int next_idx) {
    if constexpr (SMALL) {
        __shared__ SmallGeomLds small_geom;
        __shared__ SmallLightLds small_lights;
        stage_small_geom(S, small_geom);
        stage_small_lights(S, small_lights);
        __syncthreads();
    }
    const uint32_t n_dir = (uint32_t)C.n_dir;
    const uint32_t total = C.counters->n_direct[next_idx].v * n_dir;  // the grid is sized from an estimate: stride over the list
    for (uint32_t base = blockIdx.x * kBlock; base < total; base += gridDim.x * kBlock) {  // uniform trip count per block
    const uint32_t g = base + threadIdx.x;
    const bool valid = g < total;
    bool cast = false, window = false;
    f3 q = mk3(0, 0, 0), ws = mk3(0, 0, 1);
    float dist = 0.f;
    uint32_t target = 0;
#ifdef MCPT_TRAVERSAL_STATS
    bool st_nonzero = false, st_first = false, st_behind = false, st_dirac = false, st_inside = false, st_gate = false, st_tir = false;
#endif
    if (valid) {
        uint32_t dj, k;
        if (n_dir == 4u) {  // the reference's fixed count (Scene.hpp:28): no division
            dj = g >> 2;
            k = g & 3u;
        } else if ((n_dir & (n_dir - 1u)) == 0u) {  // another power of two (32, the README's count): still no division
            dj = g >> (uint32_t)(__ffs((int)n_dir) - 1);
            k = g & (n_dir - 1u);
        } else {
            dj = g / n_dir;
            k = g - dj * n_dir;
        }
        const float4 v0 = Xs.vtx0[dj], v1 = Xs.vtx1[dj], v2 = Xs.vtx2[dj];
        const uint32_t j = Xs.vtx_j[dj];
        target = j * n_dir + k;
        const uint4 r0 = next.rec0[j];
        const uint32_t bits = __float_as_uint(v2.w);
        const MaterialRec m = S.mats[bits & 0xffffu];
        const bool inside = (bits >> 18) & 1u;
        q = ld3(v0);
        const f3 n = ld3(v1), wo = ld3(v2);
        const f2 uv{v0.w, v1.w};
        RngKey key;
        int ch;
        path_key(C, r0.x, (int)((r0.z >> 20) & 1u), key, ch);
        float u[4];
        rng_block(key, r0.z & 0xffffu, 1u + k, u);
        f3 x_l = mk3(0, 0, 0), n_l = mk3(0, 0, 0), emit3 = mk3(0, 0, 0);
        float pdf = 0.f, c = 0.f;
        int32_t light_prim = -1;
        if (sample_light(S, u, x_l, n_l, emit3, pdf, light_prim)) {
            const float emit = comp(emit3, ch);
            ws = normalized(x_l - q);
            dist = norm(x_l - q);
            c = emit * mat_eval(m, ws, wo, n, ch, uv, !inside) * (dot(ws, n)) * dot(-ws, n_l) / (dist * dist) / pdf / C.n_dir;
        }
        cast = C.enable_shadow && !(c == 0.f);
        if (cast) {
            // Scene.cpp:72-75: the sample counts iff the closest hit of the shadow ray lies within EPSILON of `dist`.  The
            // ray is aimed at a point of primitive light_prim, so that primitive is tested here: a hit closer than
            // dist - EPSILON settles the sample as invisible (no ray at all); a hit inside the window settles the window
            // search, leaving only the occluder search to k_trace_shadow; otherwise the full query runs.
            double t = 0;
            uint32_t mb;
            window = true;
            if (leaf_hit(S, light_prim, make_ray(q, ws), t, mb)) {
                const double dd = t - (double)dist;
                if (dd <= -(double)kEps) {
                    c = 0.f;
                    cast = false;
                } else if (fabs(dd) < (double)kEps) {
                    window = false;
                }
            }
        }
#ifdef MCPT_CHECK_DIRECT_SKIP
        if (((bits >> 19) & 1u) && S.dbg) {
            atomicAdd(&S.dbg[14], 1ull);
            if (!(c == 0.f)) atomicAdd(&S.dbg[15], 1ull);
#ifndef MCPT_TRAVERSAL_STATS  // (that build keeps its shadow-ray statistics in 8..13)
            if ((bits >> 20) & 1u) {  // the same two counts for the vertices the half-space rule claims, with or without another rule
                atomicAdd(&S.dbg[12], 1ull);
                if (!(c == 0.f)) atomicAdd(&S.dbg[13], 1ull);
            }
            if ((bits >> 21) & 1u) {  // and for the vertices the total-internal-reflection rule claims
                atomicAdd(&S.dbg[10], 1ull);
                if (!(c == 0.f)) atomicAdd(&S.dbg[11], 1ull);
            }
#endif
        }
#endif
#ifdef MCPT_TRAVERSAL_STATS
        st_nonzero = !(c == 0.f);
        st_first = k == 0u;
        st_behind = (bits >> 20) & 1u;
        st_dirac = m.isDirac;
        st_inside = inside;
        st_tir = (bits >> 21) & 1u;
        st_gate = (bits >> 22) & 1u;
#endif
        next.contrib[target] = c;
    }
#ifdef MCPT_TRAVERSAL_STATS
    // Where the zero light samples come from (tools/direct_stats.py): samples, samples with c == 0, and -- the samples of a vertex are
    // n_dir neighbouring lanes of one wave when n_dir is a power of two -- vertices ALL of whose samples are zero, by cause: (a) every
    // emitter behind the tangent plane (emitters_behind; k_shade's statistics flavour lists those instead of skipping them),
    // (b) Dirac BSDF and not (a), (c) rough BSDF and not (a).
    if (S.dbg) {
        const unsigned long long mv = __ballot(valid), mz = __ballot(valid && !st_nonzero), mn = __ballot(st_nonzero), mf = __ballot(st_first);
        bool all_zero = false;
        if (st_first && n_dir <= 64u && (n_dir & (n_dir - 1u)) == 0u)
            all_zero = ((mn >> lane_id()) & (n_dir == 64u ? ~0ull : (1ull << n_dir) - 1ull)) == 0ull;
        const unsigned long long ma = __ballot(all_zero && st_behind), mb = __ballot(all_zero && !st_behind && st_dirac),
                                 mc = __ballot(all_zero && !st_behind && !st_dirac);
        const unsigned long long mi = __ballot(st_inside), mg = __ballot(st_gate), mt = __ballot(st_tir);
        if (lane_id() == 0) {
            atomicAdd(&S.dbg[16], (unsigned long long)__popcll(mv));
            atomicAdd(&S.dbg[17], (unsigned long long)__popcll(mz));
            atomicAdd(&S.dbg[18], (unsigned long long)__popcll(ma));
            atomicAdd(&S.dbg[19], (unsigned long long)__popcll(mb));
            atomicAdd(&S.dbg[30], (unsigned long long)__popcll(mc));
            atomicAdd(&S.dbg[31], (unsigned long long)__popcll(mf));
            // (b) split: reflection; refraction within the sin2 < 0.81 gate; beyond the gate and not / and claimed by the
            // total-internal-reflection rule (slots of their own: 6 and 7 hold the deepest traversal stacks)
            atomicAdd(&S.dbg[32], (unsigned long long)__popcll(mb & ~mi));
            atomicAdd(&S.dbg[33], (unsigned long long)__popcll(mb & mi & ~mg));
            atomicAdd(&S.dbg[34], (unsigned long long)__popcll(mb & mi & mg & ~mt));
            atomicAdd(&S.dbg[35], (unsigned long long)__popcll(mb & mi & mg & mt));
        }
    }
#endif
    // queue entries: one atomic per wave and kind on the counters of the wave's shard (see Counters): no barrier, no LDS
    const unsigned long long mf = __ballot(cast && !window), mw = __ballot(cast && window);
    if (mf | mw) {
        const uint32_t shard = (g >> 6) & (kShadowShards - 1u);
        uint32_t bf = 0, bw = 0;
        if (lane_id() == 0) {
            if (mf) bf = atomicAdd(&C.counters->n_shadow[next_idx][shard].v, (uint32_t)__popcll(mf));
            if (mw) bw = atomicAdd(&C.counters->n_shadow_w[next_idx][shard].v, (uint32_t)__popcll(mw));
        }
        bf = (uint32_t)__shfl((int)bf, 0);
        bw = (uint32_t)__shfl((int)bw, 0);
        if (cast) {
            const uint32_t region = shadow_region((uint32_t)C.pool * n_dir);
            const unsigned long long m = window ? mw : mf;
            const uint32_t off = (window ? bw : bf) + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const uint32_t e = window ? (shard + 1u) * region - 1u - off : shard * region + off;
            Xs.shq_o[e] = make_float4(q.x, q.y, q.z, __uint_as_float(target));
            Xs.shq_d[e] = make_float4(ws.x, ws.y, ws.z, dist);
        }
    }
    }
}

// ------------------------------------------------------------------------------------------------
// k_accumulate: framebuffer[m] += Vector3f(R,G,B)/spp, samples in order (Renderer.cpp:80).
// One lane per (owned pixel, channel).  kMoments (adaptive sampling, mcpt_render_adaptive): the same fold, and besides it the
// lane adds v and v*v, in double and in sample order, into moments[6m + c] and moments[6m + 3 + c].
// ------------------------------------------------------------------------------------------------
template <bool kMoments>
__global__ __launch_bounds__(kBlock) void k_accumulate(const float *__restrict__ result, const uint32_t *__restrict__ pixel_list,
                                                       uint32_t n_pix, int32_t s_pass, float spp_total, float *__restrict__ fb,
                                                       double *__restrict__ moments) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_pix * 3u) return;
    const uint32_t pl = g / 3u, c = g % 3u;
    const uint32_t m = pixel_list ? pixel_list[pl] : pl;
    float acc = fb[(size_t)m * 3 + c];
    double s1 = 0.0, s2 = 0.0;
    if (kMoments) {
        s1 = moments[(size_t)m * 6 + c];
        s2 = moments[(size_t)m * 6 + 3 + c];
    }
    const float *src = result + (size_t)pl * s_pass * 3 + c;
    int k = 0;
    for (; k + 8 <= s_pass; k += 8) {  // eight loads in flight; the additions stay in sample order (Renderer.cpp:80)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(k + u) * 3];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc += v[u] / spp_total;
            if (kMoments) {
                const double d = (double)v[u];
                s1 += d;
                s2 += d * d;
            }
        }
    }
    for (; k < s_pass; ++k) {
        const float v = src[(size_t)k * 3];
        acc += v / spp_total;
        if (kMoments) {
            const double d = (double)v;
            s1 += d;
            s2 += d * d;
        }
    }
    fb[(size_t)m * 3 + c] = acc;
    if (kMoments) {
        moments[(size_t)m * 6 + c] = s1;
        moments[(size_t)m * 6 + 3 + c] = s2;
    }
}

// ------------------------------------------------------------------------------------------------
// k_accumulate_sh: the projection fold of the light probes (mcpt_query_probes), beside k_accumulate on the same pass of `result`.
//   sh[27i + 3j + c] += (v(i, k, c) * (kFourPi * Y_j(d(i, k)))) / spp_total   for the pass's samples k in sample order
// One lane per (probe, coefficient) with the three channel sums: the direction d(i, k) is sensor_ray's, recomputed from (seed, i, k)
// rather than stored, once per sample; the three values of a sample are one 12-byte run that the nine lanes of a probe share.  Eight
// samples' loads are in flight, as in k_accumulate.  The coefficient is picked with selects: an indexed Y[j] would live in scratch.
// ------------------------------------------------------------------------------------------------
MCPT_DI float sh_weight(const SensorConst &sn, uint32_t seed, uint32_t i, uint32_t k, uint32_t j) {
    f3 pos, dir;
    sensor_ray(sn, seed, i, k, pos, dir);
    const float d[3] = {dir.x, dir.y, dir.z};
    float Y[9];
    sh::sh9_basis(d, Y);
    float y = Y[0];
#pragma unroll
    for (uint32_t q = 1; q < 9; ++q) y = j == q ? Y[q] : y;
    return sh::kFourPi * y;
}

__global__ __launch_bounds__(kBlock) void k_accumulate_sh(const float *__restrict__ result, SensorConst sn, uint32_t seed, uint32_t n_probes,
                                                          int32_t s_pass, uint32_t first_sample, float spp_total, float *__restrict__ sh_out) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_probes * 9u) return;
    const uint32_t i = g / 9u, j = g - 9u * i;
    float *dst = sh_out + (size_t)i * 27 + 3 * j;
    float a0 = dst[0], a1 = dst[1], a2 = dst[2];
    const float *src = result + (size_t)i * s_pass * 3;
    int k = 0;
    for (; k + 8 <= s_pass; k += 8) {
        float v[8][3];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            v[u][0] = src[(size_t)(k + u) * 3];
            v[u][1] = src[(size_t)(k + u) * 3 + 1];
            v[u][2] = src[(size_t)(k + u) * 3 + 2];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float w = sh_weight(sn, seed, i, first_sample + (uint32_t)(k + u), j);
            a0 += (v[u][0] * w) / spp_total;
            a1 += (v[u][1] * w) / spp_total;
            a2 += (v[u][2] * w) / spp_total;
        }
    }
    for (; k < s_pass; ++k) {
        const float v0 = src[(size_t)k * 3], v1 = src[(size_t)k * 3 + 1], v2 = src[(size_t)k * 3 + 2];
        const float w = sh_weight(sn, seed, i, first_sample + (uint32_t)k, j);
        a0 += (v0 * w) / spp_total;
        a1 += (v1 * w) / spp_total;
        a2 += (v2 * w) / spp_total;
    }
    dst[0] = a0;
    dst[1] = a1;
    dst[2] = a2;
}

__global__ __launch_bounds__(kBlock) void k_mask_unowned(float *fb, int W, int H, int tile, int rank, int nranks) {
    const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= (uint32_t)W * (uint32_t)H) return;
    const int i = (int)(m % (uint32_t)W), j = (int)(m / (uint32_t)W);
    const int tx = (W + tile - 1) / tile;
    if (((j / tile) * tx + i / tile) % nranks == rank) return;  // owned (mcpt_params: tile_size / rank / nranks)
    fb[(size_t)m * 3] = 0.f;
    fb[(size_t)m * 3 + 1] = 0.f;
    fb[(size_t)m * 3 + 2] = 0.f;
}

__global__ __launch_bounds__(kBlock) void k_add_frame(float *__restrict__ a, const float *__restrict__ b, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) a[i] += b[i];
}

__global__ __launch_bounds__(kBlock) void k_debug_fmath(int kind, uint32_t n, const float *x, const float *y, float *out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float s, c;
    switch (kind) {
    case 0: mcpt_sincosf(x[i], &s, &c); out[i] = s; break;
    case 1: mcpt_sincosf(x[i], &s, &c); out[i] = c; break;
    case 2: out[i] = mcpt_atan2f(x[i], y[i]); break;
    case 3: out[i] = mcpt_acosf(x[i]); break;
    case 4: out[i] = mcpt_powf(x[i], y[i]); break;
    default: out[i] = (float)mcpt_tonemap_byte(x[i]); break;
    }
}

// Material functions on arrays (mcpt_debug_material): rows of `in` are {a.xyz, b.xyz, c.xyz, uv.xy, u1, u2}, `sel` = {material, channel,
// is_reflect}; out = 4 floats per row.  kind 0 eval(wi=a, wo=b, n=c), 1 pdf, 2 fresnel(I=a, N=b), 3 sample(n=a, u1, u2), 4 refract(I=a, N=b),
// 5 the fused eval+pdf of k_shade (out = {eval, pdf}), 6 reflect(I=a, N=b).
__global__ __launch_bounds__(kBlock) void k_debug_material(DevScene S, int kind, uint32_t n, const float *__restrict__ in, const int32_t *__restrict__ sel,
                                                           float *__restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *r = in + (size_t)i * 13;
    const f3 a = mk3(r[0], r[1], r[2]), b = mk3(r[3], r[4], r[5]), c = mk3(r[6], r[7], r[8]);
    const f2 uv{r[9], r[10]};
    const MaterialRec m = S.mats[sel[3 * i]];
    const int ch = sel[3 * i + 1];
    const bool refl = sel[3 * i + 2] != 0;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    switch (kind) {
    case 0: o[0] = mat_eval(m, a, b, c, ch, uv, refl); break;
    case 1: o[0] = mat_pdf(m, a, b, c, ch, refl); break;
    case 2: o[0] = mat_fresnel(m, a, b, ch); break;
    case 3: {
        const f3 v = mat_sample(m, a, r[11], r[12]);
        o[0] = v.x, o[1] = v.y, o[2] = v.z;
        break;
    }
    case 4: {
        const f3 v = mat_refract(m, a, b, ch);
        o[0] = v.x, o[1] = v.y, o[2] = v.z;
        break;
    }
    case 5: mat_eval_pdf_rough(m, a, b, c, ch, uv, refl, o[0], o[1]); break;
    default: {
        const f3 v = mat_reflect(a, b);
        o[0] = v.x, o[1] = v.y, o[2] = v.z;
        break;
    }
    }
    for (int k = 0; k < 4; ++k) out[(size_t)i * 4 + k] = o[k];
}

// Scene functions on arrays (mcpt_debug_scene): kind 0 Scene::sampleLight for 4 uniforms per row -> {x_l, n_l, emit, pdf} (10 floats; zeros
// when no light was selected), kind 1 Scene::sampleEnv for a direction per row -> rgb.
__global__ __launch_bounds__(kBlock) void k_debug_scene(DevScene S, int kind, uint32_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (kind == 0) {
        const float u[4] = {in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]};
        f3 x = mk3(0, 0, 0), nl = mk3(0, 0, 0), e = mk3(0, 0, 0);
        float pdf = 0.f;
        int32_t prim = -1;
        (void)sample_light(S, u, x, nl, e, pdf, prim);
        float *o = out + (size_t)i * 10;
        o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = nl.x, o[4] = nl.y, o[5] = nl.z, o[6] = e.x, o[7] = e.y, o[8] = e.z, o[9] = pdf;
    } else {
        const f3 c = sample_env(S, mk3(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
        out[3 * i] = c.x, out[3 * i + 1] = c.y, out[3 * i + 2] = c.z;
    }
}

// The light samples and shadow rays of the sampled direct term (launch_direct_rays, csrc/mcpt_kernels.h).  It sits here for sample_light,
// which it runs as k_debug_scene does; the geometry is dl::sample_geometry.  LIT: the points are the lit pass's records.  No early
// return: every lane takes part in the ballot.
template <bool LIT>
__global__ __launch_bounds__(kBlock) void k_direct_rays(DevScene S, DirectRays a) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    const bool in = g < a.m * a.jc;
    bool live = false, sampled = false;
    float q[3], ws[3], dist = 0.f, contrib[3] = {0.f, 0.f, 0.f};
    if (in) {
        const uint32_t pi = g / a.jc, s = g - pi * a.jc, i = a.i0 + pi;
        float p[3], nf[3];
        RngKey rk{a.seed, i, a.key_sample, kDirectStream};
        bool point = true;
        if (LIT) {
            point = __float_as_uint(a.r0[i].w) == a.surface_kind;
            const float4 p4 = a.r2[i], n4 = a.r1[i];
            p[0] = p4.x, p[1] = p4.y, p[2] = p4.z;
            nf[0] = n4.x, nf[1] = n4.y, nf[2] = n4.z;
            rk.pixel = a.p0 + i / (uint32_t)a.aov_spp;
            rk.sample = a.sample0 + i % (uint32_t)a.aov_spp;
        } else {
            const size_t b = 3 * (size_t)i;
            p[0] = a.points[b], p[1] = a.points[b + 1], p[2] = a.points[b + 2];
            nf[0] = a.normals[b], nf[1] = a.normals[b + 1], nf[2] = a.normals[b + 2];
        }
        if (point) {
            float u[4];
            rng_block(rk, 0u, a.j0 + s, u);
            f3 x = mk3(0, 0, 0), nl = mk3(0, 0, 0), e = mk3(0, 0, 0);
            float pdf = 0.f;
            int32_t prim = -1;
            (void)sample_light(S, u, x, nl, e, pdf, prim);
            const float row[dl::kLightRow] = {x.x, x.y, x.z, nl.x, nl.y, nl.z, e.x, e.y, e.z, pdf};
            live = dl::sample_geometry(p, nf, row, a.N, q, ws, dist, contrib);
            sampled = true;
        }
    }
    (void)sampled;
    bool ray = live;  // the lanes whose shadow ray is traced
#ifdef MCPT_DIRECT_TRACE_DEAD
    // A/B only (tools/ab.sh, DESIGN.md "Direct light in probe-lit frames"): a dead sample with a usable direction is traced as well, and
    // its hit ignored, to measure what the compaction saves.
    ray = live || (sampled && dist > 0.f && dist <= dl::kFltMax);
#endif
    const unsigned long long mask = __ballot(ray), lmask = __ballot(live);
    uint32_t k = kDirectDead;
    if (mask != 0ull) {
        uint32_t base = 0;
        if (lane_id() == 0) {
            base = atomicAdd(a.n_rays, (uint32_t)__popcll(mask));
            if (a.total && lmask != 0ull) atomicAdd(a.total, (unsigned long long)__popcll(lmask));
        }
        base = __shfl(base, 0);
        if (ray) {
            const uint32_t kr = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            a.ray_o[kr] = make_float4(q[0], q[1], q[2], __uint_as_float(g));
            a.ray_d[kr] = make_float4(ws[0], ws[1], ws[2], dist);
            if (live) k = kr;
        }
    }
    if (in) a.slot[g] = make_float4(contrib[0], contrib[1], contrib[2], __uint_as_float(k));
}

// Renderer.cpp:95-103 on the device: one lane per pixel, RGBA8 out (alpha 255).
__global__ __launch_bounds__(kBlock) void k_tonemap(const float *__restrict__ fb, uint32_t n_pix, uchar4 *__restrict__ rgba) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pix) return;
    rgba[i] = make_uchar4(mcpt_tonemap_byte(fb[(size_t)i * 3]), mcpt_tonemap_byte(fb[(size_t)i * 3 + 1]), mcpt_tonemap_byte(fb[(size_t)i * 3 + 2]), 255);
}

inline uint32_t blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

// Runs after k_shade(cur -> next).  List `cur` and everything indexed like it (its closest-hit queue, k_direct work
// list and shadow queue, all produced one iteration earlier) are consumed: their lengths go to the totals and are
// cleared, because `cur` is the next iteration's output list.
// In the regular schedule k_primary may already be appending fresh records to list `next` on another stream, so the host
// passes the lengths it read right after k_shade (from_host); in the drain phase they are read here.
__global__ void k_bookkeep(Counters *c, int cur_idx, int from_host, uint32_t n_next, uint32_t n_cont, uint32_t n_direct) {
    const int nxt = cur_idx ^ 1;
    // The 2 x 32 shard counters of the consumed shadow queue: one lane each, summed over the wave.  (Until round 3 lane 0 walked them in a
    // loop: 64 dependent global round trips, 115 us per launch of a kernel that sits between k_shade and k_direct on the main stream --
    // 29 ms of a 650 ms frame.)
    static_assert(2 * kShadowShards == 64, "one lane per shard counter");
    HotCounter *const shard = threadIdx.x < kShadowShards ? &c->n_shadow[cur_idx][threadIdx.x] : &c->n_shadow_w[cur_idx][threadIdx.x - kShadowShards];
    uint32_t n_shadow = shard->v;
    shard->v = 0;
    for (int o = 32; o > 0; o >>= 1) n_shadow += (uint32_t)__shfl_xor((int)n_shadow, o);
    switch (threadIdx.x) {  // one lane per field: the global accesses are independent and overlap
    case 0: {
        c->tot_shadow += n_shadow;
        c->last_shadow = n_shadow;
        break;
    }
    // (Records only, not the fresh entries of new samples.  The records k_primary's short path writes into list `nxt` are first vertices
    // shaded there and are counted here like k_shade's; the first list of a call is never counted here, so for
    // that one (RenderConst::first_fill) the short path adds them to `ended` itself.)
    case 1: c->tot_shaded += from_host ? n_next : c->n_paths[nxt].v; break;
    case 2: c->tot_cont += from_host ? n_cont : c->n_rays[nxt].v; break;
    case 3: c->tot_direct += from_host ? n_direct : c->n_direct[nxt].v; break;
    case 4: c->tot_iterations += 1; break;
    case 8: {  // only k_shade (same stream, already finished) and this iteration's k_primary (joined before the read-back that precedes this launch) write these
        const uint32_t v = c->ended.v;
        c->ended.v = 0;
        c->tot_ended += v;
        break;
    }
    case 9: {
        const uint32_t v = c->pushes.v;
        c->pushes.v = 0;
        c->tot_pushes += v;
        break;
    }
    case 11: {
        const uint32_t v = c->shared.v;
        c->shared.v = 0;
        c->tot_shared += v;
        break;
    }
    case 5: c->n_paths[cur_idx].v = 0; break;
    case 6: c->n_rays[cur_idx].v = 0; break;
    case 10: c->n_prays[cur_idx].v = 0; break;
    case 12: c->n_brays[cur_idx].v = 0; break;
    case 13: {
        const uint32_t v = c->pc_samples.v;
        c->pc_samples.v = 0;
        c->tot_pc_samples += v;
        break;
    }
    case 14: {
        const uint32_t v = c->pc_rays.v;
        c->pc_rays.v = 0;
        c->tot_pc_rays += v;
        break;
    }
    case 7: c->n_direct[cur_idx].v = 0; break;
    default: break;
    }
}

void launch_bookkeep(Counters *c, int cur_idx, bool from_host, uint32_t n_next, uint32_t n_cont, uint32_t n_direct, hipStream_t s) {
    hipLaunchKernelGGL(k_bookkeep, dim3(1), dim3(64), 0, s, c, cur_idx, from_host ? 1 : 0, n_next, n_cont, n_direct);
}

void launch_init_free(uint32_t *free_slots, Counters *c, uint32_t pool, uint32_t start, uint32_t mask, hipStream_t s) {
    hipLaunchKernelGGL(k_init_free, dim3(blocks(pool)), dim3(kBlock), 0, s, free_slots, c, pool, start, mask);
}

// (MCPT_STACK_DISPATCH, the choice of the stack flavour by tree height, and kRetraceGrid: csrc/mcpt_stack_dispatch.h)
void launch_primary(const DevScene &S, const CameraConst &cam, const RenderConst &C, Wave next, int next_idx, int parity,
                    uint32_t first_sample, uint32_t n_samples, const RetryList &rl, hipStream_t s) {
    if (n_samples == 0) return;
    const dim3 g(blocks(n_samples)), b(kBlock);
    MCPT_STACK_DISPATCH(S.height, k_primary, hipLaunchKernelGGL(k_primary_retrace, dim3(kRetraceGrid), b, 0, s, S, cam, C, next, next_idx, parity, rl), g, b, 0, s, S,
                        cam, C, next, next_idx, parity, first_sample, n_samples, rl);
}

void launch_sensor_primary(const DevScene &S, const SensorConst &sn, const RenderConst &C, Wave next, int next_idx, int parity,
                           uint32_t first_sample, uint32_t n_samples, const RetryList &rl, hipStream_t s) {
    if (n_samples == 0) return;
    const dim3 g(blocks(n_samples)), b(kBlock);
    if (sn.indirect_only) {
        MCPT_STACK_DISPATCH(S.height, k_sensor_primary_indirect,
                            hipLaunchKernelGGL(k_sensor_primary_retrace_indirect, dim3(kRetraceGrid), b, 0, s, S, sn, C, next, next_idx, parity, rl), g, b, 0, s, S, sn,
                            C, next, next_idx, parity, first_sample, n_samples, rl);
        return;
    }
    MCPT_STACK_DISPATCH(S.height, k_sensor_primary, hipLaunchKernelGGL(k_sensor_primary_retrace, dim3(kRetraceGrid), b, 0, s, S, sn, C, next, next_idx, parity, rl), g,
                        b, 0, s, S, sn, C, next, next_idx, parity, first_sample, n_samples, rl);
}

void launch_sensor_rays(const SensorConst &sn, uint32_t seed, uint32_t n, const uint32_t *sensor, const uint32_t *sample, float4 *o, float4 *d,
                        hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_sensor_rays, dim3(blocks(n)), dim3(kBlock), 0, s, sn, seed, n, sensor, sample, o, d);
}

void launch_sensor_variance(uint32_t n_sensors, int32_t spp, const double *moments, float *variance, hipStream_t s) {
    if (n_sensors == 0) return;
    hipLaunchKernelGGL(k_sensor_variance, dim3(blocks(n_sensors * 3u)), dim3(kBlock), 0, s, n_sensors * 3u, spp, moments, variance);
}

void launch_generate_explicit(const RenderConst &C, Wave next, int next_idx, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_generate_explicit, dim3(blocks(n)), dim3(kBlock), 0, s, next, C.counters, next_idx, n);
}

void launch_camera_rays(const CameraConst &cam, uint32_t seed, uint32_t n, const uint32_t *pixel, const uint32_t *sample,
                        float4 *o, float4 *d, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_camera_rays, dim3(blocks(n)), dim3(kBlock), 0, s, cam, seed, n, pixel, sample, o, d);
}

void launch_centre_rays(const CameraConst &cam, uint32_t p0, uint32_t n, float4 *o, float4 *d, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_centre_rays, dim3(blocks(n)), dim3(kBlock), 0, s, cam, p0, n, o, d);
}

void launch_trace_closest(const DevScene &S, uint32_t n, const uint32_t *n_dev, const float4 *ray_o, const float4 *ray_d, uint4 *hit,
                          const RetryList &rl, hipStream_t s) {
    if (n == 0) return;
#ifndef MCPT_NO_REFILL
    if (S.qnodes && !S.inst) {  // the common configuration: lanes refill from the wave's chunk of rays
        const dim3 g((n + kBlock * kRaysPerLane - 1) / (kBlock * kRaysPerLane)), b(kBlock);
        MCPT_STACK_DISPATCH(S.height, k_trace_closest_refill, hipLaunchKernelGGL(k_retrace_closest, dim3(kRetraceGrid), b, 0, s, S, ray_o, ray_d, hit, rl), g, b, 0, s, S,
                            n, n_dev, ray_o, ray_d, hit, rl);
        return;
    }
#endif
    const dim3 g(blocks(n)), b(kBlock);
    MCPT_STACK_DISPATCH(S.height, k_trace_closest, hipLaunchKernelGGL(k_retrace_closest, dim3(kRetraceGrid), b, 0, s, S, ray_o, ray_d, hit, rl), g, b, 0, s, S, n, n_dev,
                        ray_o, ray_d, hit, rl);
}

void launch_direct(const DevScene &S, const RenderConst &C, Wave next, Scratch X, int next_idx, uint32_t n_vertices_grid, uint32_t small_per_cu, hipStream_t s) {
    if (n_vertices_grid == 0) return;
    dim3 g(blocks(n_vertices_grid * (uint32_t)C.n_dir)), b(kBlock);
    // (SMALL: every workgroup first copies the scene into LDS; a capped grid lets it stride over several chunks of the list for one copy)
    if (S.small && small_per_cu) g.x = std::min<uint32_t>(g.x, 256u * small_per_cu);
    if (S.small) hipLaunchKernelGGL((k_direct<true>), g, b, 0, s, S, C, next, X, next_idx);
    else hipLaunchKernelGGL((k_direct<false>), g, b, 0, s, S, C, next, X, next_idx);
}

void launch_trace_shadow(const DevScene &S, const Counters *counters, int next_idx, uint32_t n_max, uint32_t cap, Scratch X,
                         float *contrib, uint32_t per_cu, const RetryList &rl, hipStream_t s) {
    if (n_max == 0) return;
    // The queue length is only known on the device.  The grid covers the upper bound, capped at `per_cu` workgroups per CU (Knobs:
    // 128, far more than are resident, so the hardware balances uneven rays dynamically: a persistent 8-per-CU grid
    // was 30 % slower on the Cornell box); workgroups past the end of the queue exit at once, longer queues stride.
    const dim3 g(std::min<uint32_t>(blocks(n_max), 256u * per_cu)), b(kBlock);
    MCPT_STACK_DISPATCH(S.height, k_trace_shadow,
                        hipLaunchKernelGGL(k_retrace_shadow, dim3(kRetraceGrid), b, 0, s, S, counters, next_idx, cap, X.shq_o, X.shq_d, contrib, rl), g, b, 0, s, S,
                        counters, next_idx, cap, X.shq_o, X.shq_d, contrib, rl);
}

void launch_shade(const DevScene &S, const RenderConst &C, Wave cur, Wave next, Scratch X, int cur_idx, uint32_t n_cur_max,
                  hipStream_t s) {
    if (n_cur_max == 0) return;
    hipLaunchKernelGGL(k_shade, dim3((n_cur_max + kShadeBlock - 1) / kShadeBlock), dim3(kShadeBlock), 0, s, S, C, cur, next, X, cur_idx);
}

void launch_direct_rays(const DevScene &S, const DirectRays &a, hipStream_t s) {
    if (a.m == 0 || a.jc == 0) return;
    if (a.r0) hipLaunchKernelGGL(k_direct_rays<true>, dim3(blocks(a.m * a.jc)), dim3(kBlock), 0, s, S, a);
    else hipLaunchKernelGGL(k_direct_rays<false>, dim3(blocks(a.m * a.jc)), dim3(kBlock), 0, s, S, a);
}

void launch_tonemap(const float *fb, uint32_t n_pix, unsigned char *rgba, hipStream_t s) {
    if (n_pix == 0) return;
    hipLaunchKernelGGL(k_tonemap, dim3(blocks(n_pix)), dim3(kBlock), 0, s, fb, n_pix, reinterpret_cast<uchar4 *>(rgba));
}

void launch_mask_unowned(float *fb, int width, int height, int tile, int rank, int nranks, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_unowned, dim3(blocks((uint32_t)width * (uint32_t)height)), dim3(kBlock), 0, s, fb, width, height, tile, rank, nranks);
}

void launch_add_frame(float *a, const float *b, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_add_frame, dim3(blocks(n)), dim3(kBlock), 0, s, a, b, n);
}

void launch_debug_fmath(int kind, uint32_t n, const float *x, const float *y, float *out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_fmath, dim3(blocks(n)), dim3(kBlock), 0, s, kind, n, x, y, out);
}

void launch_debug_scene(const DevScene &S, int kind, uint32_t n, const float *in, float *out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_scene, dim3(blocks(n)), dim3(kBlock), 0, s, S, kind, n, in, out);
}

void launch_debug_material(const DevScene &S, int kind, uint32_t n, const float *in, const int32_t *sel, float *out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_material, dim3(blocks(n)), dim3(kBlock), 0, s, S, kind, n, in, sel, out);
}

void launch_accumulate(const float *result, const uint32_t *pixel_list, uint32_t n_pix, int32_t s_pass, float spp_total,
                       float *fb, double *moments, hipStream_t s) {
    if (n_pix == 0) return;
    if (moments)
        hipLaunchKernelGGL(k_accumulate<true>, dim3(blocks(n_pix * 3u)), dim3(kBlock), 0, s, result, pixel_list, n_pix, s_pass, spp_total, fb, moments);
    else
        hipLaunchKernelGGL(k_accumulate<false>, dim3(blocks(n_pix * 3u)), dim3(kBlock), 0, s, result, pixel_list, n_pix, s_pass, spp_total, fb, moments);
}

void launch_accumulate_sh(const float *result, const ShSink &sink, uint32_t n_probes, int32_t s_pass, int32_t first_sample, float spp_total, hipStream_t s) {
    if (n_probes == 0) return;
    hipLaunchKernelGGL(k_accumulate_sh, dim3(blocks(n_probes * 9u)), dim3(kBlock), 0, s, result, sink.sn, sink.seed, n_probes, s_pass, (uint32_t)first_sample,
                       spp_total, sink.sh);
}

}  // namespace mcpt
