// The host layer behind the C ABI (include/mcpt.h): error plumbing, the owners of device resources, the wavefront workspace, the
// environment knobs, the event timer, struct mcpt_scene, and what its translation units call in each other:
//   mcpt_wavefront.hip  the wavefront loop, workspace / pass sizing (render_list), the pixel list and sky cull set-up
//   mcpt_upload.hip     scene create / upload / snapshot / destroy / info, the BVH dumps
//   mcpt_edit.hip       the live edits: update / deform / material and environment edits / visibility / added objects
//   mcpt_update.hip     the kernels that move, deform and add objects in HBM (the device path of mcpt_scene_update / mcpt_scene_deform /
//                       mcpt_scene_add_objects), mcpt_transform_triangles, mcpt_deform_triangles
//   mcpt_render.hip     the frame-level entry points (render, adaptive, AOVs, denoise, motion, temporal blend); mcpt_frame.h has what
//                       it shares with
//   mcpt_sequence.hip   mcpt_temporal_accumulate and mcpt_sequence_*: a frame loop whose history and buffers stay on the device
//   mcpt_query.hip      ray queries on host memory, tone map and the debug entry points
//   mcpt_rayquery.hip   mcpt_query_closest / mcpt_query_occluded: ray queries on device memory, with their kernels; mcpt_query_radiance /
//                       mcpt_sensor_rays: radiance at sensors in device memory (csrc/mcpt_sensor.h)
//   mcpt_lightmap.hip   mcpt_lightmap_texels / mcpt_lightmap_scatter / mcpt_bake_lightmap and their host forms, with their kernels
//                       (csrc/mcpt_lightmap.h)
//   mcpt_multi.hip      mcpt_group_*
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mcpt_kernels.h"
#include "mcpt_lbvh.h"
#include "mcpt_material.h"

namespace mcpt {

extern thread_local std::string g_err;  // what mcpt_last_error returns (defined in mcpt_upload.hip)

inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? MCPT_ERR_OOM : MCPT_ERR_HIP,                        \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                             \
    } while (0)

#define MCPT_LOCAL __attribute__((visibility("hidden")))  // shared between translation units, not in the library's dynamic symbol table

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

// ---- owners.  Each frees what it holds when it goes out of scope (the device it was made on must be current), so an early error
// return cannot leak it and nothing is listed a second time for release.  None can be copied or moved.

// Device allocation; release() frees early.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    size_t bytes() const { return n * sizeof(T); }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
};

template <typename T>
hipError_t upload(DevBuf<T> &b, const T *src, size_t count) {
    hipError_t e = b.alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpy(b.p, src, count * sizeof(T), hipMemcpyHostToDevice);
}
template <typename T>
hipError_t upload(DevBuf<T> &b, const std::vector<T> &v) {
    return upload(b, v.data(), v.size());
}
template <typename T>
hipError_t download(T *dst, const DevBuf<T> &b, size_t count) {
    return hipMemcpy(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost);
}

// Non-blocking stream.  Destroyed only after the work queued on it is known to be done (drained(), or a synchronise that returned).
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create(bool timing = false) { return timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    operator hipEvent_t() const { return e; }
};

// The pinned host copy of the device counters.
struct PinnedCounters {
    Counters *p = nullptr;
    PinnedCounters() = default;
    PinnedCounters(const PinnedCounters &) = delete;
    PinnedCounters &operator=(const PinnedCounters &) = delete;
    ~PinnedCounters() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t alloc() { return p ? hipSuccess : hipHostMalloc((void **)&p, sizeof(Counters)); }
    Counters *operator->() const { return p; }
};

struct WaveBufs {
    DevBuf<uint4> rec0, hit;
    DevBuf<float4> rec1, ray_o, ray_d;
    DevBuf<float> contrib;
    DevBuf<uint2> fresh;
    Wave view() const { return Wave{rec0.p, rec1.p, ray_o.p, ray_d.p, hit.p, contrib.p, fresh.p}; }
};

// The retrace lists of the traversal kernels (RetryList, csrc/mcpt_kernels.h): allocated only for scenes whose tree runs the retry
// flavour of the traversal stack (stack_uses_retry); each list holds as many entries as one launch can have rays.
struct RetryBufs {
    DevBuf<uint32_t> ctl;  // {count, done} x 3, zero between launches
    DevBuf<uint32_t> items[3];
    uint32_t cap[3] = {0, 0, 0};
    hipError_t alloc(const uint32_t want[3]) {
        hipError_t e = ctl.alloc(8);
        if (e != hipSuccess) return e;
        if ((e = hipMemset(ctl.p, 0, 8 * sizeof(uint32_t))) != hipSuccess) return e;
        for (int k = 0; k < 3; ++k) {
            if ((e = items[k].alloc(want[k])) != hipSuccess) return e;
            cap[k] = want[k];
        }
        return hipSuccess;
    }
    // the closest-hit list alone, for launches of up to n rays outside the wavefront loop; nothing when the tree needs no retrace
    hipError_t for_rays(uint32_t n, int height) {
        const uint32_t want[3] = {n, 1u, 1u};
        return stack_uses_retry(height) ? alloc(want) : hipSuccess;
    }
    RetryList list(int k) const { return ctl.p ? RetryList{ctl.p + 2 * k, ctl.p + 2 * k + 1, items[k].p, cap[k]} : RetryList{nullptr, nullptr, nullptr, 0u}; }
};

struct Workspace {
    uint32_t pool = 0, free_ring = 0, ray_cap = 0;
    RetryBufs retry;  // 0 closest-hit rays, 1 shadow rays, 2 primary samples
    int32_t n_dir = 0, max_depth = 0;
    WaveBufs wave[2];
    DevBuf<float4> vtx0, vtx1, vtx2, shq_o, shq_d;
    DevBuf<uint32_t> vtx_j;
    Scratch scratch() const { return Scratch{vtx0.p, vtx1.p, vtx2.p, vtx_j.p, shq_o.p, shq_d.p}; }
    DevBuf<float4> stack;
    DevBuf<uint32_t> free_slots;
    DevBuf<Counters> counters;
    PinnedCounters h_counters;
};

// Buffers shared by the wavefront pools of one scene.
struct SharedBufs {
    DevBuf<float> result;
    DevBuf<uint32_t> pixel_list, key_pixel, key_sample;
    DevBuf<uint32_t> culled_list, cull_count;  // pixel_list partitioned: [may hit | background only] (csrc/mcpt_cull.hip)
    DevBuf<uint8_t> cull_flags, cull_temp;
    DevBuf<int4> cand_tmp, cand_list;  // per pixel: the few primitives its rays can hit (aligned with culled_list)
    DevBuf<int32_t> key_channel;
    DevBuf<double> sensor_moments;  // mcpt_query_radiance with a variance: 6 doubles per sensor (sums of v and v*v per channel); grows to the largest call
    int pix_key[5] = {0, 0, 0, 0, 0};  // (W, H, tile, rank, nranks) of the pixel list currently in HBM
    uint32_t n_pix = 0;
};

// What mcpt_query_closest / mcpt_query_occluded (csrc/mcpt_rayquery.hip) keep between calls.  The buffers only ever grow, so a call
// allocates only when it stages more rays than any call before it.  `done` is recorded on the caller's stream behind every query: a call
// that frees or swaps what a query reads (the geometry arrays, these buffers) waits for it on the host first (query_settle, below), and
// a query on another stream waits for it on the device before it reuses the staging buffers.
struct QueryBufs {
    DevBuf<float4> ray_o, ray_d;     // one chunk of staged rays; ray_d.w = tmax
    DevBuf<uint4> hit;               // their closest hits
    RetryBufs retry;                 // list 0 alone: the rays of a chunk, for trees that run the retry flavour
    DevBuf<int32_t> ranges;          // the mesh triangle ranges for the object lookup: m starts in ascending order, then their m objects
    std::vector<int32_t> h_ranges;   // its host copy
    bool table_valid = false;        // `ranges` describes the scene's objects (false again after mcpt_scene_add_objects)
    // mcpt_query_direct alone: one record per (point, light sample) of a chunk, and the length of the chunk's compacted shadow-ray list
    DevBuf<float4> direct_slot;
    DevBuf<uint32_t> direct_n;
    Event done;
    bool pending = false;            // `done` has been recorded and nobody has waited for it on the host since
    hipStream_t last_stream = nullptr;
};

// What the lightmap calls (csrc/mcpt_lightmap.hip) keep between calls.  Like QueryBufs the buffers only ever grow, and everything these
// calls enqueue is followed by a record of QueryBufs::done, so whatever settles a ray query settles a lightmap call too.
struct LightmapBufs {
    DevBuf<unsigned long long> counts, scan;  // per triangle of the object (+ 1): tiles its chart touches, and their exclusive sum
    DevBuf<int32_t> owner;                    // W*H: the lowest primitive id covering the texel, lm::kNoOwner for none
    DevBuf<uint8_t> temp;                     // hipcub's scratch (scan and select)
    DevBuf<int32_t> n_sel;                    // the select's count
    DevBuf<float> plane;                      // W*H*3: the second plane of the dilation's ping-pong
    DevBuf<uint8_t> cov[2];                   // W*H each: the second coverage plane, and the first when the caller passes none
    // mcpt_bake_lightmap: the sensors and their results
    DevBuf<int32_t> texel;                    // W*H
    DevBuf<float> origins, normals, radiance, variance;  // n*3 each
    int64_t last_items = 0;                   // of the last mcpt_lightmap_texels
    bool grew = false;                        // a buffer above was (re)allocated since the flag was last cleared
};

// What the light-probe calls (csrc/mcpt_probes.hip) keep between calls; the buffers only ever grow.
struct ProbeBufs {
    DevBuf<float> points;    // mcpt_bake_probe_grid: the grid's points, n*3
    DevBuf<float> radiance;  // mcpt_query_probes without a caller's radiance: the plain fold still needs a place, n*3
    int64_t allocations = 0; // how often one of them was (re)allocated (mcpt_scene_probe_buffers)
    // mcpt_render_probe_lit[_direct]: the eight-byte counters of its lookups and live light samples, made by the scene's first such call.  Working storage, no
    // probe buffer: it is in neither figure of mcpt_scene_probe_buffers.
    DevBuf<unsigned long long> lit_count;
    // mcpt_probe_volume_relight: per probe ray of a piece the lit sample's records {v or a, kind} {nf} {p} and its direct term D, and the
    // staging of the direct term's light samples (shadow rays, their hits, the per-sample records and the compacted list's length).  Probe
    // buffers: counted in both figures of mcpt_scene_probe_buffers (four floats per entry; the two scalars are not).
    DevBuf<float4> relit_r0, relit_r1, relit_r2, relit_d, relit_ray_o, relit_ray_d, relit_slot;
    DevBuf<uint4> relit_hit;
    DevBuf<uint32_t> relit_n;
    DevBuf<unsigned long long> relit_count;  // k_lit_shade's count of lookups; never read back
};

// Environment knobs, read ONCE per scene in mcpt_scene_create: a render call never calls getenv.
struct Knobs {
    bool overlap = true;        // MCPT_OVERLAP=0: one stream instead of three
    bool queue_ahead = true;    // MCPT_QUEUE_AHEAD=0: wait for the counters before launching the chains
    bool timing = true;         // MCPT_TIMING=0: no per-kernel HIP events
    bool verbose = false;       // MCPT_RENDER_VERBOSE=1: a line per render call on stderr (pass size, pool, time of the allocations)
    int pools = 1;              // MCPT_POOLS=2: two pools on two host threads
    int drain_batch = 4;        // MCPT_DRAIN_BATCH: iterations per host sync in the drain tail
    uint64_t pool_min_work = 1ull << 20;  // MCPT_POOL_MIN_WORK: smallest pass (samples) that uses two pools
    // Grid caps, in workgroups per CU.  Every workgroup of k_trace_shadow computes the prefix sums of the queue's shards first, and the
    // LDS-resident flavours copy the scene into LDS first: with 128 / 64 per CU a workgroup strides over several chunks for one such
    // prologue and the hardware still balances uneven rays (round 3, A/B: cornell_rc 784^2 471 -> 490 Msamples/s, DEMO 1080p 873 -> 924,
    // k_trace_shadow -11 %, k_direct -14 %; chess within noise for 64..1024.  8 per CU, a persistent grid, was 30 % slower in round 1).
    uint32_t shadow_grid_per_cu = 128;    // MCPT_SHADOW_GRID_PER_CU: grid cap of k_trace_shadow
    uint32_t direct_grid_per_cu = 64;     // MCPT_DIRECT_GRID_PER_CU: grid cap of k_direct for LDS-resident scenes (0: none)
    uint32_t query_chunk = 1u << 20;      // MCPT_QUERY_CHUNK: most rays mcpt_query_closest / mcpt_query_occluded stage at once (at least 64)
    // pure test hooks, compiled only into the checking build (-DMCPT_TEST_HOOKS, libmcpt_hip_check.so)
    uint32_t ring_start = 0;    // MCPT_RING_START: the free ring's counters start here (exercises the 2^32 wrap)
    int host_delay_us = 0;      // MCPT_HOST_DELAY_US: a slow host
    float halfspace_slack_scale = 1.f;  // MCPT_HALFSPACE_SLACK_SCALE: multiplies the margin of direct_is_zero's half-space rule (a negative
                                        // scale makes the rule wrong on purpose: the negative control of tests/test_gpu_direct_halfspace.py)
    float tir_bound_scale = 1.f;        // MCPT_TIR_BOUND_SCALE: multiplies the bound of direct_is_zero's total-internal-reflection rule (below
                                        // 1: wrong on purpose, the negative control of tests/test_gpu_direct_tir.py)
    float cone_tol_scale = 1.f;         // MCPT_CONE_TOL_SCALE: multiplies the two tolerances of direct_is_zero's cone rule (below 1: wrong
                                        // on purpose, the negative control of tests/test_gpu_direct_cone.py)
    float cull_rho_scale = 1.f;         // MCPT_CULL_RHO_SCALE: multiplies the sky cull's final rho (below 1: wrong on purpose, the negative
                                        // control of tests/test_gpu_cull_classify.py)
    bool sky_cull = true;       // MCPT_SKY_CULL=0: trace the pixels that can only see the background too
    bool small_scene = true;    // MCPT_SMALL_SCENE=0: no LDS-resident flavour for scenes of a few KB
    bool share_rays = true;     // MCPT_SHARE_RAYS=0: every channel path stores and traces its own continuation ray (RenderConst::share_rays)
    bool primary_conductor = true;  // MCPT_PRIMARY_CONDUCTOR=0: first hits on smooth conductors go through k_shade like every other (RenderConst::primary_conductor)
    uint64_t fake_free_mb = 0;  // MCPT_FAKE_FREE_MB: pretend that only this much device memory is free (exercises the pool shrink)
    void read();
};

enum KClass { K_CLOSEST = 0, K_SHADOW, K_SHADE, K_GENERATE, K_RESOLVE, K_DIRECT, K_NCLASS };

struct Timer {
    // Two banks of events: the host runs one iteration ahead of the GPU, so the events of iteration i are only known to be
    // complete once the read-back of iteration i+1 has arrived; iteration i+1 meanwhile records into the other bank.
    bool enabled = true;
    int bank = 0;
    std::vector<hipEvent_t> pool[2];  // owned
    struct Rec { int a, b, cls; };
    std::vector<Rec> recs[2];
    size_t used[2] = {0, 0};
    double ms[K_NCLASS] = {0, 0, 0, 0, 0, 0};
    uint64_t count[K_NCLASS] = {0, 0, 0, 0, 0, 0};
    Timer() = default;
    Timer(const Timer &) = delete;
    Timer &operator=(const Timer &) = delete;
    ~Timer() {
        for (int k = 0; k < 2; ++k)
            for (hipEvent_t e : pool[k]) (void)hipEventDestroy(e);
    }
    int get() {
        if (used[bank] == pool[bank].size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return -1;
            pool[bank].push_back(e);
        }
        return (int)used[bank]++;
    }
    // One launch of class `cls` on stream s: counted, and (timing on) bracketed by two events on s.
    template <typename Launch>
    void timed(int cls, hipStream_t s, Launch &&launch) {
        const int a = enabled ? get() : -1;
        if (a >= 0) (void)hipEventRecord(pool[bank][a], s);
        launch();
        count[cls]++;
        const int b = a >= 0 ? get() : -1;
        if (b < 0) return;
        (void)hipEventRecord(pool[bank][b], s);
        recs[bank].push_back({a, b, cls});
    }
    void collect_bank(int k) {  // every event of bank k must have completed
        for (const Rec &r : recs[k]) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, pool[k][r.a], pool[k][r.b]) == hipSuccess) ms[r.cls] += t;
        }
        recs[k].clear();
        used[k] = 0;
    }
    void collect() {  // call after a full stream sync
        collect_bank(0);
        collect_bank(1);
    }
    void reset() {
        for (int i = 0; i < K_NCLASS; ++i) { ms[i] = 0; count[i] = 0; }
        for (int k = 0; k < 2; ++k) { recs[k].clear(); used[k] = 0; }
        bank = 0;
    }
};

// What the wavefront loop did, summed over pools, passes and calls.
struct Totals {
    uint64_t iterations = 0, shaded = 0, closest = 0, shadow = 0, direct = 0, pushes = 0, overflow = 0;
    // `closest` counts resolved rays: every record's ray, whether k_trace_closest walked the tree for it or a sibling's ray served
    // (Counters::shared).  The continuation rays among them: cont_traced walked, cont_shared did not.
    uint64_t cont_traced = 0, cont_shared = 0;
    // Of those, k_primary's short path (first hits on smooth conductors): its samples, and the reflected rays it walked itself (part of cont_traced).
    uint64_t pc_samples = 0, pc_rays = 0;
    double ms[K_NCLASS] = {0, 0, 0, 0, 0, 0};
    uint64_t cnt[K_NCLASS] = {0, 0, 0, 0, 0, 0};
    Totals &operator+=(const Totals &o) {
        iterations += o.iterations;
        shaded += o.shaded;
        closest += o.closest;
        shadow += o.shadow;
        direct += o.direct;
        pushes += o.pushes;
        overflow += o.overflow;
        cont_traced += o.cont_traced;
        cont_shared += o.cont_shared;
        pc_samples += o.pc_samples;
        pc_rays += o.pc_rays;
        for (int c = 0; c < K_NCLASS; ++c) {
            ms[c] += o.ms[c];
            cnt[c] += o.cnt[c];
        }
        return *this;
    }
};

// The device arrays that depend on where the objects are.  Every live edit (csrc/mcpt_edit.hip) fills a second set beside the live one,
// in its EditAside, and the commit swaps the two once the new tree is known to be usable, so that a failed edit leaves the scene as it was.
struct GeomBufs {
    DevBuf<Node> nodes;
    DevBuf<QNode> qnodes;
    DevBuf<TriGeom> tri_geom;
    DevBuf<TriShade> tri_shade;
    DevBuf<SphereRec> spheres;
    DevBuf<mcpt_triangle> tris;  // device builders, after the first update: the moved triangles the tree was built from
    DevBuf<LightRec> lights;
    DevBuf<LightNode> light_nodes;
    DevBuf<LightTri> light_tris;
    void swap_nodes(GeomBufs &o) {  // the tree alone (mcpt_scene_set_visibility, path 1: no record is written)
        nodes.swap(o.nodes);
        qnodes.swap(o.qnodes);
    }
    void swap_prims(GeomBufs &o) {  // the tree and the primitive records
        nodes.swap(o.nodes);
        qnodes.swap(o.qnodes);
        tri_geom.swap(o.tri_geom);
        tri_shade.swap(o.tri_shade);
        spheres.swap(o.spheres);
        tris.swap(o.tris);
    }
    void swap_lights(GeomBufs &o) {
        lights.swap(o.lights);
        light_nodes.swap(o.light_nodes);
        light_tris.swap(o.light_tris);
    }
};

// What DevScene and mcpt_scene_info take from a flattened scene besides the arrays (fill_view, csrc/mcpt_upload.hip).
struct SceneMeta {
    int32_t root = 0, height = 0, n_inner = 0, n_leaf_prims = 0;
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0}, q_origin[3] = {0, 0, 0}, q_cell[3] = {1, 1, 1};
    int32_t n_triangles = 0, n_objects = 0, builder = 0, n_instances = 0;
    int32_t n_sphere_slots = 0, n_mats = 0, n_lights = 0, n_light_nodes = 0, n_light_tris = 0;
    int32_t env_w = 0, env_h = 0;
    float background[3] = {0, 0, 0};
    float light_area_sum = 0.f, light_center[3] = {0, 0, 0}, light_radius = 0.f;
};

// The base description of a scene and the transforms its objects currently have (mcpt_scene_update: transforms are absolute, so every
// update starts from these arrays).  The triangles are the creation-time ones until mcpt_scene_deform replaces a mesh's positions; the
// host copy is kept current by every successful deformation (positions given by device pointer are downloaded eagerly).
struct SceneSource {
    std::vector<mcpt_triangle> triangles;
    std::vector<mcpt_object> objects;
    std::vector<mcpt_material> materials;
    std::vector<uint8_t> moved;  // per object: 1 once it has been given a transform
    std::vector<float> xf;       // per object: its row-major 3x4 matrix (unused while moved == 0)
    BuildChoice choice;          // the builder and its options as resolved at creation
    std::vector<uint8_t> visible;  // per object: 0 while hidden (mcpt_scene_set_visibility); every rebuild keeps hidden objects out of the tree
    std::vector<float> env;      // the environment map (meta.env_w x env_h x 3; empty: the constant background), the way back of
                                 // mcpt_group_set_environment
};

// One run of lanes of the update kernel (csrc/mcpt_update.hip): the triangles of a moved mesh, or one moved sphere.
struct alignas(16) MoveSeg {
    int32_t first_lane;  // lanes [first_lane, first_lane + count) work on this segment
    int32_t count;       // mesh: its triangles; sphere: 1
    int32_t first_tri;   // mesh: its first triangle; sphere: -1
    int32_t object;      // sphere: its slot in the SphereRec array
    float m[12];
    float c0[3];         // sphere: the creation-time centre
    int32_t raw;         // 1: the object has no transform: the creation-time values are copied, not multiplied by an identity
};
static_assert(sizeof(MoveSeg) == 80, "MoveSeg must be 80 bytes");
// Writes, for every listed segment, the moved triangle into tris_cur and the geometry words of its TriGeom / TriShade records (mat_bits,
// mat and the texture coordinates stay), or the moved centre into its SphereRec.  tris0: the creation-time triangles.
void launch_move_objects(const MoveSeg *d_segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *tris0, mcpt_triangle *tris_cur,
                         TriGeom *tri_geom, TriShade *tri_shade, SphereRec *spheres, hipStream_t s);

// One run of lanes of the deformation kernel (csrc/mcpt_update.hip): the triangles of one deformed mesh.
struct alignas(16) DeformSeg {
    int32_t first_lane;      // lanes [first_lane, first_lane + the mesh's triangle count) work on this segment
    int32_t first_tri;       // the mesh's first triangle
    int32_t object;
    int32_t raw;             // 1: the object has no transform: the given floats are stored, not multiplied by an identity
    float m[12];             // the object's current transform (unused when raw)
    const float *positions;  // device pointer: 9 floats per triangle, the scene's staging buffer or the caller's array read in place
};
static_assert(sizeof(DeformSeg) == 80, "DeformSeg must be 80 bytes");
// For every lane: the new base triangle (positions + the texture coordinates of tris0) into `base`, and what launch_move_objects writes
// for it.  *flag (zeroed by the caller) becomes 1 when a position is not finite; such a lane writes nothing else.
void launch_deform_objects(const DeformSeg *d_segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *tris0, mcpt_triangle *base, mcpt_triangle *tris_cur,
                           TriGeom *tri_geom, TriShade *tri_shade, uint32_t *flag, hipStream_t s);
// Writes, for every lane of the listed segments (mat::MatSeg, csrc/mcpt_material.h), the segment's mat_bits and mat into the TriGeom /
// TriShade records of its triangle, or into its SphereRec; nothing else in the records is read or written.
void launch_set_materials(const mat::MatSeg *d_segs, int32_t n_segs, int32_t n_lanes, TriGeom *tri_geom, TriShade *tri_shade, SphereRec *spheres,
                          hipStream_t s);

// One run of lanes of k_add_objects (csrc/mcpt_update.hip): the triangles of one added mesh, or one added sphere.  Three 16-byte quarters.
struct alignas(16) AddSeg {
    int32_t first_lane;  // lanes [first_lane, first_lane + count) work on this segment
    int32_t count;       // mesh: its triangles; sphere: 1
    int32_t first_tri;   // mesh: its first triangle in the extended arrays; sphere: -1
    int32_t object;      // sphere: its slot in the SphereRec array
    uint32_t mat_bits;   // TriGeom::mat_bits / SphereRec::mat_bits (mat::tri_mat_bits / sphere_mat_bits)
    int32_t mat;         // TriShade::mat / SphereRec::mat
    float radius;        // sphere
    int32_t pad0;
    float c[3];          // sphere: its centre
    int32_t pad1;
};
static_assert(sizeof(AddSeg) == 48, "AddSeg must be 48 bytes");
// Writes, for every lane of the listed segments, the WHOLE records of an added primitive: a triangle lane reads its triangle from tris0
// (the appended tail of the base array), stores it into tris_cur and writes its TriGeom and TriShade records; a sphere lane writes its
// SphereRec.  Nothing is loaded from the record arrays.
void launch_add_objects(const AddSeg *d_segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *tris0, mcpt_triangle *tris_cur, TriGeom *tri_geom,
                        TriShade *tri_shade, SphereRec *spheres, hipStream_t s);

}  // namespace mcpt

// Members are destroyed in reverse order, with the scene's device current (mcpt_scene_destroy): the pools' workspaces and timers, their
// events, their streams, the shared buffers, then the scene arrays.
struct mcpt_scene {
    int device = 0;
    int device_sharers = 1;  // scenes of one group that live on this device (mcpt_group_create with a device listed several times)
    mcpt::Knobs knobs;
    mcpt_scene_info info{};
    uint64_t last_pc_samples = 0, last_pc_rays = 0;  // the short path of k_primary in that call (mcpt_scene_primary_conductor_counts)
    uint64_t last_cont_traced = 0, last_cont_shared = 0;  // continuation rays of the last render or mcpt_cast_rays call (mcpt_scene_ray_counts)
    mcpt::SceneMeta meta;
    mcpt::SceneSource src;
    mcpt::GeomBufs geom;
    // mcpt_scene_snapshot: where the primitives were when it was last called (TriGeom and SphereRec arrays indexed like the live ones;
    // primitive ids are stable across updates).  Empty until the first snapshot: the motion pass then reads the live arrays.
    mcpt::DevBuf<mcpt::TriGeom> snap_tri;
    mcpt::DevBuf<mcpt::SphereRec> snap_sph;
    bool has_snapshot = false;
    mcpt::DevBuf<mcpt_triangle> tris0;   // device builders: the base triangles (creation time, then every mcpt_scene_deform)
    mcpt::DevBuf<int32_t> sphere_obj;    // device builders: object index of every sphere (the builder's primitive list)
    mcpt::DevBuf<mcpt::MoveSeg> segs;    // the update kernel's segment table
    mcpt::DevBuf<mcpt::DeformSeg> dsegs; // the deformation kernel's segment table,
    mcpt::DevBuf<float> stage;           // its staging buffer for host positions (36 B per triangle, grows to the largest call)
    mcpt::DevBuf<uint32_t> dflag;        // and its flag word (a position that is not finite)
    mcpt::DevBuf<mcpt::mat::MatSeg> msegs;  // the segment table of k_set_materials
    mcpt::DevBuf<mcpt::AddSeg> asegs;    // the segment table of k_add_objects
    mcpt::DevBuf<mcpt::MaterialRec> mats;
    mcpt::DevBuf<mcpt::InstRec> inst;
    mcpt::DevBuf<float> env;
    mcpt::DevBuf<unsigned long long> dbg;
    mcpt::DevScene view{};
    mcpt::Event fork;
    mcpt::QueryBufs query;
    mcpt::LightmapBufs lightmap;
    mcpt::ProbeBufs probes;
    mcpt::SharedBufs shared;
    // A wavefront pool: its own path lists, queues, clamp stack, counters and streams.  With MCPT_POOLS=2 two pools
    // are driven by two host threads on disjoint halves of each pass, so that one pool's k_shade (and its host
    // round trip) overlaps the other pool's traversal kernels.
    struct PoolCtx {
        mcpt::Stream main;  // owned stream (pool 0 uses the caller's stream instead)
        // The three chains of one iteration (direct -> shadow, continuation rays, new primary rays) are
        // independent: they run on separate streams and are joined before the next k_shade.
        mcpt::Stream side[2];
        mcpt::Event join[2];
        mcpt::Event book;  // main -> primary stream: the previous iteration's k_bookkeep has cleared the list counters
        mcpt::Event shaded, readback;  // k_shade done (-> closest stream); counters are in host memory
        int rc = 0;
        std::string err;
        mcpt::Timer timer;
        mcpt::Workspace ws;
    };
    static constexpr int kMaxPools = 2;
    PoolCtx pools[kMaxPools];
    int n_pools = 2;
};

namespace mcpt {

using PoolCtx = mcpt_scene::PoolCtx;

// Waits on the host for the last ray query enqueued on the scene (QueryBufs::done).  Called, with the scene's device current, by everything
// that frees or swaps arrays a query reads; without a query in flight it does nothing.  objects_changed: the object table is no longer
// the one the query's range table was made from.
inline hipError_t query_settle(mcpt_scene *sc, bool objects_changed = false) {
    if (objects_changed) sc->query.table_valid = false;
    if (!sc->query.pending) return hipSuccess;
    const hipError_t e = hipEventSynchronize(sc->query.done);
    if (e == hipSuccess) sc->query.pending = false;
    return e;
}

// hipPointerGetAttributes places p in the memory of `device` (the pointer checks of the ray queries and the lightmap calls)
inline bool on_device(const void *p, int device) {
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (an address the runtime does not know: not a sticky error)
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == device;
}

// ---- mcpt_rayquery.hip
// The two ends of everything that uses the ray queries' staging buffers: query_stage makes them hold `chunk` rays on stream st (growth
// behind query_settle, the wait for a query on another stream, the range table; qi.grew says whether it allocated) and gives the retry
// list of the chunk's launches; query_finish records QueryBufs::done behind what was enqueued since.  With the scene's device current.
int query_stage(mcpt_scene *sc, uint32_t chunk, hipStream_t st, mcpt_query_info &qi, RetryList &rl);
int query_finish(mcpt_scene *sc, hipStream_t st, mcpt_query_info &qi);

// ---- mcpt_upload.hip
// The two halves of mcpt_scene_create, exposed for mcpt_group_create (csrc/mcpt_multi.hip), which flattens the scene and builds its
// tree once and then uploads it to every device from one thread per device.
struct HostBuild {
    HostScene hs;
    BuildChoice choice;
    double build_ms = 0.0;  // flattening + host tree build
    double init_ms = 0.0;   // first use of the device by this process (context, code objects), overlapped with the host build
};
int build_scene_host(const mcpt_scene_desc *desc, const mcpt_build_options *options, HostBuild &hb);
int upload_scene(const mcpt_scene_desc *desc, HostBuild &hb, int device, mcpt_scene **out);
double warm_up_device(int device);
// What the edit layer (csrc/mcpt_edit.hip) shares with creation.
MCPT_LOCAL SceneMeta meta_of(const HostScene &hs);
// What the device builders need to leave hidden objects out (VisTable, csrc/mcpt_lbvh.h): one entry per visible mesh in triangle-array
// order, and the visible sphere objects.
struct DevVis {
    DevBuf<VisSeg> segs;
    DevBuf<int32_t> sph;
    int32_t n_segs = 0, n_tri = 0, n_sph = 0;
    bool active = false;  // false: every object is visible, the builders run as they do without a table
};
MCPT_LOCAL int upload_vis(const std::vector<mcpt_object> &objects, const std::vector<uint8_t> &visible, DevVis &dv);
MCPT_LOCAL int32_t count_visible_prims(const SceneSource &S, const std::vector<uint8_t> &visible);
// The device builders' tree into g.nodes / g.qnodes, depth check included (see the definition).
MCPT_LOCAL int build_device_tree_checked(const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, int n_sph, const BuildChoice &choice, GeomBufs &g, SceneMeta &meta,
                                         const DevVis *dv, const SphereRec *d_spheres = nullptr);
// Copies the arrays of a flattened scene that depend on where its objects are into `g`; for the device builders the tree is then built
// there from d_tris (the triangles `hs` was flattened from).  Shared by mcpt_scene_create and the host path of every edit.
MCPT_LOCAL int upload_geometry(const HostScene &hs, const BuildChoice &choice, const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, GeomBufs &g, SceneMeta &meta,
                               double &gpu_build_ms, const DevVis *dv = nullptr);
// DevScene and the geometry fields of mcpt_scene_info from the scene's arrays and sc->meta: after creation and after every edit.
MCPT_LOCAL void fill_view(mcpt_scene *sc);

// ---- mcpt_edit.hip
// Every edit in two halves: check_* are the argument checks, before any device call (they fill what the scene would hold afterwards);
// apply_* is the edit without them, which mcpt_group_* (csrc/mcpt_multi.hip) runs on every replica and, with the previous values, as the
// way back when another replica fails.  update: the table (moved, xf) the scene gets, of which the objects in `touched`
// differ; deform: the n listed meshes get the given positions as their base; visibility: the mask, and the objects whose state changes.
int check_moves(const mcpt_scene *sc, int32_t n, const mcpt_object_transform *moves, std::vector<uint8_t> &moved, std::vector<float> &xf,
                std::vector<int32_t> &touched);
int apply_transforms(mcpt_scene *sc, const std::vector<uint8_t> &moved, const std::vector<float> &xf, const std::vector<int32_t> &touched,
                     mcpt_update_info *info);
int check_deform(const mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items);
int apply_deform(mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items, mcpt_update_info *info);
int check_material_edit(const mcpt_scene *sc, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign, const mcpt_object_material *assign,
                        mat::EditPlan &plan);
int apply_material_edit(mcpt_scene *sc, const mat::EditPlan &plan, mcpt_update_info *info);
int check_visibility(const mcpt_scene *sc, int32_t n, const mcpt_object_visibility *items, std::vector<uint8_t> &visible, std::vector<int32_t> &changed);
int apply_visibility(mcpt_scene *sc, const std::vector<uint8_t> &visible, const std::vector<int32_t> &changed, mcpt_update_info *info);
// What an edit builds aside: `parts` says which of the members below replace the scene's, and the commit exchanges exactly those, so
// afterwards the aside holds what the scene had.  Freed with the scene's device current.
struct EditAside {
    enum Part : uint32_t {  // geom's tree, its primitive records (and the tree with them), its light tables; the device builders' base triangles and sphere
                            // list; the material table; the snapshot; a deformation's new base on the host, or PATCH: the meshes in `patch` are overwritten in place
        TREE = 1u << 0, PRIMS = 1u << 1, LIGHTS = 1u << 2, TRIS0 = 1u << 3, SPHERE_OBJ = 1u << 4, MATS = 1u << 5, SNAPSHOT = 1u << 6,
        TRIANGLES = 1u << 7, PATCH = 1u << 8,
    };
    uint32_t parts = 0;
    GeomBufs geom;
    DevBuf<mcpt_triangle> tris0;
    DevBuf<int32_t> sphere_obj;
    DevBuf<MaterialRec> mats;
    DevBuf<TriGeom> snap_tri;
    DevBuf<SphereRec> snap_sph;
    SceneMeta meta;  // (always part of the exchange)
    std::vector<mcpt_triangle> triangles;
    std::vector<std::pair<int32_t, const float *>> patch;  // a deformation: (object, its 9 floats per triangle on the host)
    std::vector<std::vector<float>> fetched;                // of which those downloaded from device pointers live here
};
// mcpt_scene_add_objects.  After a successful apply_add with `keep`, *keep holds the arrays the scene had: undo_add commits them back
// (mcpt_group_add_objects, when another replica fails).  A type of its own only so that apply_add and undo_add keep their exported names.
struct AddAside : EditAside {};
int check_add(const mcpt_scene *sc, const mcpt_scene_addition *add);
int apply_add(mcpt_scene *sc, const mcpt_scene_addition *add, int32_t *first_object, mcpt_update_info *info, AddAside *keep = nullptr);
int undo_add(mcpt_scene *sc, AddAside &aside);
int check_environment(const mcpt_scene *sc, const float *background, int32_t env_w, int32_t env_h, const float *env_pixels);
int apply_environment(mcpt_scene *sc, const float *background, int32_t env_w, int32_t env_h, const float *env_pixels, mcpt_update_info *info);

// ---- mcpt_wavefront.hip
hipError_t ensure_workspace(PoolCtx &ctx, uint32_t pool, int32_t n_dir, int32_t max_depth, bool retry_lists);
int derive_max_depth(const mcpt_params &p);
CameraConst make_camera(const mcpt_camera &c);
// RenderConst with what the params decide (rr_rate, n_dir_sample, shadows, seed) and max_depth; the rest zero
RenderConst base_consts(const mcpt_params &p, int max_depth);

// One pass of a render call: `n_work` camera samples whose results live in one half of the result buffer.
struct PassPlan {
    uint32_t first_work;  // first sample slot of the pass handled by this pool
    uint32_t n_work;      // sample slots handled by this pool
    int32_t s_pass, sample_offset;
};

// Where finished passes go.  acc == nullptr: the caller accumulates (single pass only).
struct AccumPlan {
    float *fb;
    float spp_total;
    uint32_t n_pix;
    const uint32_t *pixel_list;
    float *result[2];
    double *moments;  // adaptive sampling: per-pixel sums of v and v*v (nullptr: the plain fold)
    const ShSink *sh = nullptr;  // mcpt_query_probes: every pass is also projected by k_accumulate_sh (nullptr: nothing changes)
};

// Where the first rays of new samples come from (mode 0): the camera of a frame, or the sensors of mcpt_query_radiance.  Holds pointers:
// what it is made from outlives the call it is passed to.  Neither (mode 1, mcpt_cast_rays): the caller has uploaded the rays.
struct RaySource {
    const CameraConst *cam = nullptr;
    const SensorConst *sensors = nullptr;
    RaySource() = default;
    RaySource(const CameraConst &c) : cam(&c) {}
    RaySource(const SensorConst &s) : sensors(&s) {}
};

int run_wavefront(mcpt_scene *sc, PoolCtx &ctx, const RenderConst &C0, const RaySource &src, const std::vector<PassPlan> &plan,
                  const AccumPlan *acc, hipStream_t st, Totals &tot);
// After a failed run_wavefront the side streams may still hold kernels that use the workspace: wait for them before the
// caller sees the error (and possibly frees buffers).  The error text of the failure is kept.
int drained(int rc);

// The owned pixels of a render call once the sky cull has run: the traced ones (with their candidate lists, or none) and the culled ones.
struct PixelSet {
    uint32_t n_owned = 0, n_pix = 0;  // owned pixels, traced pixels
    const uint32_t *list = nullptr;   // the traced pixels
    const int4 *cand = nullptr;       // their sky-cull candidate entries (nullptr: primary rays walk the tree)
    const uint32_t *sky = nullptr;    // the n_owned - n_pix culled pixels
};
int prepare_pixels(mcpt_scene *sc, const CameraConst &cc, const mcpt_params &p, int32_t spp, float spp_total, float *fb_dev, hipStream_t st,
                   PixelSet &ps);
int render_list(mcpt_scene *sc, const RaySource &src, const mcpt_params &p, const uint32_t *pixel_list, const int4 *pixel_cand, uint32_t n_pix,
                int32_t sample_offset, int32_t spp, float spp_total, float *fb_dev, double *moments, hipStream_t st, Clock::time_point t0,
                Totals &rt, const ShSink *sh = nullptr);

// ---- mcpt_rayquery.hip
// mcpt_query_radiance after its checks, shared with mcpt_query_probes (csrc/mcpt_probes.hip): n > 0 sensors `sn` into radiance (cleared
// unless p.accumulate), the variance when asked, and with sh != nullptr the projection fold into sh (cleared likewise).  Blocks.
int sensor_radiance(mcpt_scene *sc, const mcpt_params &p, uint32_t n, const SensorConst &sn, float *radiance, float *variance, float *sh,
                    hipStream_t st, mcpt_stats *stats);

// ---- mcpt_render.hip
void add(mcpt_stats &a, const mcpt_stats &b);  // every count and kernel time of b into a (ms_total is the caller's)

}  // namespace mcpt
