// The host-side wavefront loop, and what sizes and feeds it.
//
// The loop replaces the pixel/spp loops of Renderer::Render (reference src/Renderer.cpp:36-90).  Samples are
// streamed through a fixed pool of path records: every iteration shades all live records, refills the
// pool with new camera samples ("path regeneration") and traces all rays of the iteration in two launches
// (closest-hit queue, shadow queue), so the GPU always works on full, compacted queues.
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <thread>

#include "mcpt_host.h"
#include "mcpt_cull.h"

namespace mcpt {

hipError_t ensure_workspace(PoolCtx &ctx, uint32_t pool, int32_t n_dir, int32_t max_depth, bool retry_lists) {
    Workspace &w = ctx.ws;
    hipError_t e;
    const size_t n_rays = (size_t)pool + pool / 3 + 64;
    for (int k = 0; k < 2; ++k) {
        WaveBufs &b = w.wave[k];
        if ((e = b.rec0.alloc(pool)) != hipSuccess) return e;
        if ((e = b.rec1.alloc(pool)) != hipSuccess) return e;
        if ((e = b.ray_o.alloc(n_rays)) != hipSuccess) return e;
        if ((e = b.ray_d.alloc(n_rays)) != hipSuccess) return e;
        if ((e = b.hit.alloc(n_rays)) != hipSuccess) return e;
        if ((e = b.contrib.alloc((size_t)pool * n_dir)) != hipSuccess) return e;
        if ((e = b.fresh.alloc(pool / 3 + 64)) != hipSuccess) return e;
    }
    if ((e = w.vtx0.alloc(pool)) != hipSuccess) return e;
    if ((e = w.vtx1.alloc(pool)) != hipSuccess) return e;
    if ((e = w.vtx2.alloc(pool)) != hipSuccess) return e;
    if ((e = w.vtx_j.alloc(pool)) != hipSuccess) return e;
    const size_t shq = (size_t)kShadowShards * shadow_region((uint32_t)std::min<uint64_t>((uint64_t)pool * n_dir, 0xffffffffull));  // (sharded: Counters)
    if ((e = w.shq_o.alloc(shq)) != hipSuccess) return e;
    if ((e = w.shq_d.alloc(shq)) != hipSuccess) return e;
    if ((e = w.stack.alloc((size_t)pool * max_depth)) != hipSuccess) return e;
    uint64_t ring = 1;
    // free-slot ring: a power of two, so that the 32-bit head/tail counters may wrap, and at least twice the pool: the entries
    // k_primary has popped are read one iteration later (by k_shade) and must not be reached by the pushes made meanwhile
    // (free + pushed + popped <= 2 * pool)
    while (ring < 2 * (uint64_t)pool) ring <<= 1;
    if ((e = w.free_slots.alloc(ring)) != hipSuccess) return e;
    w.free_ring = (uint32_t)ring;
    w.ray_cap = (uint32_t)n_rays;
    if (retry_lists) {
        const uint32_t want[3] = {(uint32_t)n_rays, (uint32_t)std::min<uint64_t>((uint64_t)pool * n_dir, 0xffffffffull), pool / 3 + 64};
        if ((e = w.retry.alloc(want)) != hipSuccess) return e;
    }
    if ((e = w.counters.alloc(1)) != hipSuccess) return e;
    if ((e = w.h_counters.alloc()) != hipSuccess) return e;
    w.pool = pool;
    w.n_dir = n_dir;
    w.max_depth = max_depth;
    return hipSuccess;
}

int derive_max_depth(const mcpt_params &p) {
    if (p.max_depth > 0) return p.max_depth;
    const double rr = std::min(std::max((double)p.rr_rate, 1e-6), 0.999999);
    const int d = (int)std::ceil(std::log(1e-12) / std::log(rr));
    return std::min(std::max(d, 8), 8192);
}

CameraConst make_camera(const mcpt_camera &c) {
    CameraConst k;
    std::memset(&k, 0, sizeof k);
    k.width = c.width;
    k.height = c.height;
    k.use_dof = c.use_dof;
    // Renderer.cpp:13,25-26: deg2rad(deg) = deg * M_PI(float) / 180.0 returned as float; scale = tan(...)
    const float half = c.fov * 0.5f;
    const float rad = (float)((double)(half * 3.141592653589793f) / 180.0);
    k.scale = (float)std::tan((double)rad);
    k.aspect = c.width / (float)c.height;
    k.focal_distance = c.focal_distance;
    k.aperture_radius = c.aperture_radius;
    for (int i = 0; i < 3; ++i) k.eye[i] = c.position[i];
    for (int i = 0; i < 9; ++i) k.orient[i] = c.orientation[i];
    return k;
}

RenderConst base_consts(const mcpt_params &p, int max_depth) {
    RenderConst C;
    std::memset(&C, 0, sizeof C);
    C.rr_rate = p.rr_rate;
    C.inv_rr = 1 / p.rr_rate;  // Scene.hpp:112
    C.n_dir = p.n_dir_sample;
    C.enable_shadow = p.enable_shadow;
    C.seed = p.seed;
    C.max_depth = max_depth;
    return C;
}

// Owned pixels in an order that keeps neighbouring list entries neighbouring on screen: tiles in
// row-major order, 8x8 blocks inside a tile.
static void build_pixel_list(int W, int H, int tile, int rank, int nranks, std::vector<uint32_t> &out) {
    out.clear();
    if (tile <= 0) tile = 32;
    if (nranks < 1) nranks = 1;
    const int tx = (W + tile - 1) / tile, ty = (H + tile - 1) / tile;
    for (int tj = 0; tj < ty; ++tj)
        for (int ti = 0; ti < tx; ++ti) {
            if (((tj * tx + ti) % nranks) != rank) continue;
            const int x0 = ti * tile, y0 = tj * tile, x1 = std::min(W, x0 + tile), y1 = std::min(H, y0 + tile);
            for (int by = y0; by < y1; by += 8)
                for (int bx = x0; bx < x1; bx += 8)
                    for (int y = by; y < std::min(y1, by + 8); ++y)
                        for (int x = bx; x < std::min(x1, bx + 8); ++x) out.push_back((uint32_t)(y * W + x));
        }
}

// Runs the wavefront loop over a schedule of passes (mode 0) or over `plan[0].n_work` explicit paths (mode 1).
// Up to two passes are in flight: as soon as a pass has no samples left to issue, the next one starts filling the pool,
// so the drain tail of a pass overlaps useful work.  A pass is complete when its live-path counter is 0 (and all its
// samples were issued at least one iteration ago); passes are accumulated into the framebuffer strictly in order.
int run_wavefront(mcpt_scene *sc, PoolCtx &ctx, const RenderConst &C0, const RaySource &src, const std::vector<PassPlan> &plan,
                  const AccumPlan *acc, hipStream_t st, Totals &tot) {
    Workspace &w = ctx.ws;
    Timer &T = ctx.timer;
    RenderConst C = C0;
    C.pool = w.pool;
    C.stack = w.stack.p;
    C.free_slots = w.free_slots.p;
    C.free_mask = w.free_ring - 1u;
    C.ray_cap = w.ray_cap;
    C.counters = w.counters.p;
    const uint32_t pool = w.pool;
    const int n_dir = C.n_dir;
    const int P = (int)plan.size();
    C.track_live = (acc && P > 1) ? 1 : 0;
    const Knobs &K = sc->knobs;
    C.share_rays = K.share_rays ? 1 : 0;
    C.primary_conductor = (K.primary_conductor && C.mode == 0) ? 1 : 0;
    launch_init_free(w.free_slots.p, w.counters.p, pool, K.ring_start, w.free_ring - 1u, st);
    if (ctx.side[1].s) {  // fork: the side streams start after everything queued on `st` so far (counters, pixel list, framebuffer)
        HIP_TRY(hipEventRecord(ctx.book, st));
        for (int k = 0; k < 2; ++k) HIP_TRY(hipStreamWaitEvent(ctx.side[k], ctx.book, 0));
    }
    int cur = 0;
    uint32_t n_cur_max = 0;  // upper bound of the record count of wave[cur] (the exact count lives on the device)
    int issue_pass = 0, accum_next = 0;
    uint32_t issued = 0;
    uint32_t free_known = 0;  // free slots according to the last read-back (a lower bound of what k_primary may pop)
    bool have_counters = false;  // w.h_counters holds a read-back of THIS call
    // continuation rays / direct-lighting vertices per record, as observed in the last iteration: they size the grids of the
    // kernels that are queued before the host knows the true lengths (grid-stride kernels: any grid is correct)
    double cont_ratio = 1.0, direct_ratio = 1.0;
    double shadow_ratio = 1.0;      // shadow rays per light sample, as observed (sizes the grid of k_trace_shadow; any grid is correct)
    uint32_t n_direct_prev = 0, n_direct_prev2 = 0;  // lengths of the k_direct work lists of the two previous iterations
    bool n_cur_exact = false;  // n_cur_max is the true list length (false right after the prologue: an upper bound)
    long it = 0;
    std::vector<long> issue_done_iter(P, -1);
    hipStream_t s_close = ctx.side[0].s ? ctx.side[0].s : st, s_prim = ctx.side[1].s ? ctx.side[1].s : st;

    auto set_pass_consts = [&](int pi) {  // kernel constants of the pass occupying parity pi & 1
        const int32_t sp = plan[pi].s_pass;
        C.s_pass[pi & 1] = sp;
        C.sample_offset[pi & 1] = plan[pi].sample_offset;
        int sh = -1;
        if (sp > 0 && (sp & (sp - 1)) == 0)
            for (sh = 0; (1 << sh) < sp; ++sh) {}
        C.s_pass_shift[pi & 1] = sh;
    };
    // issues up to `room` new samples from the passes that may be in flight; returns how many
    // Room in list `nxt` for the short path of k_primary (first hits on smooth conductors).  A sample still yields at most three records and
    // three slots, so the callers' checks ((pool - n_cur_max) / 3, free_known / 3) hold as they are.  Ray entries: a sample takes ONE back
    // entry, either among the first `room` (its camera ray, indexed by n_prays) or among the `room` below them (the reflected ray it traced
    // itself, indexed by n_brays from back2_base down); k_shade's continuation rays fill the front, at most one per lane, n_cur_max in all.
    // n_cur_max + 2 room <= n_cur_max + 2 (pool - n_cur_max) / 3 <= pool < ray_cap = pool + pool / 3 + 64 (the prologue: 2 pool / 3).
    auto issue = [&](Wave nx, int nxt, uint32_t room) -> uint32_t {
        uint32_t total = 0;
        C.back2_base = C.ray_cap - 1u - room;
        C.first_fill = it == 0 ? 1 : 0;
        while (room > 0 && issue_pass < P && (!acc || issue_pass < accum_next + 2)) {
            if (issued == 0) set_pass_consts(issue_pass);
            const uint32_t g = std::min<uint32_t>(room, plan[issue_pass].n_work - issued);
            if (g > 0) {
                T.timed(K_GENERATE, s_prim, [&] {
                    if (src.sensors) launch_sensor_primary(sc->view, *src.sensors, C, nx, nxt, issue_pass & 1, plan[issue_pass].first_work + issued, g, w.retry.list(2), s_prim);
                    else launch_primary(sc->view, *src.cam, C, nx, nxt, issue_pass & 1, plan[issue_pass].first_work + issued, g, w.retry.list(2), s_prim);
                });
                tot.closest += g;
            }
            issued += g;
            room -= g;
            total += g;
            if (issued == plan[issue_pass].n_work) {
                issue_done_iter[issue_pass] = it;
                issue_pass++;
                issued = 0;
            } else {
                break;
            }
        }
        return total;
    };
    // accumulates, in order, every pass that is complete according to the counters just read back
    auto accumulate_done = [&](hipStream_t s) {
        while (acc && have_counters && accum_next < issue_pass && issue_done_iter[accum_next] < it &&
               (C.track_live ? w.h_counters->live[accum_next & 1].v == 0 : (n_cur_max == 0 && issue_pass >= P))) {
            T.timed(K_RESOLVE, s, [&] { launch_accumulate(acc->result[accum_next & 1], acc->pixel_list, acc->n_pix, plan[accum_next].s_pass, acc->spp_total, acc->fb, acc->moments, s); });
            if (acc->sh)  // (light probes: the same pass of `result`, before the half is handed to the pass after next)
                T.timed(K_RESOLVE, s, [&] { launch_accumulate_sh(acc->result[accum_next & 1], *acc->sh, acc->n_pix, plan[accum_next].s_pass, plan[accum_next].sample_offset, acc->spp_total, s); });
            accum_next++;
        }
    };

    // prologue: fill the pool
    {
        Wave nx = w.wave[cur].view();
        if (C.mode == 0) {
            n_cur_max = 3 * issue(nx, cur, pool / 3);
        } else {
            // explicit rays were uploaded into wave[cur].ray_o/ray_d by the caller
            const uint32_t n_work = plan[0].n_work;
            launch_generate_explicit(C, nx, cur, n_work, st);
            issue_pass = P;
            n_cur_max = n_work;
            T.timed(K_CLOSEST, st, [&] { launch_trace_closest(sc->view, n_work, nullptr, nx.ray_o, nx.ray_d, nx.hit, w.retry.list(0), st); });
            tot.closest += n_work;
        }
        for (int k = 0; k < 2; ++k) {  // join the side streams before the first k_shade
            if (!ctx.side[k].s) continue;
            HIP_TRY(hipEventRecord(ctx.join[k], ctx.side[k]));
            HIP_TRY(hipStreamWaitEvent(st, ctx.join[k], 0));
        }
    }

    const bool queue_ahead = K.queue_ahead;
    const int host_delay_us = K.host_delay_us;
    const int drain_batch = K.drain_batch;  // iterations queued per host sync once no samples are left to issue
    while (n_cur_max > 0 || issue_pass < P || (acc && accum_next < P)) {
        ++it;
        // (big lists keep the three-stream schedule with exact launch sizes: over-sized grids only pay off when small)
        const bool draining = issue_pass >= P && n_cur_max > 0 && n_cur_max <= (2u << 20);
        if (draining && drain_batch > 1) {
            // Drain phase: no regeneration, so list lengths only shrink.  Several iterations are queued back to back
            // on one stream with the last known length as the grid bound (every kernel reads the true lengths on the
            // device); the host looks at the counters once per batch.
            for (int k = 0; k < drain_batch; ++k) {
                const int nxt = cur ^ 1;
                Wave cw = w.wave[cur].view(), nx = w.wave[nxt].view();
                T.timed(K_SHADE, st, [&] { launch_shade(sc->view, C, cw, nx, w.scratch(), cur, n_cur_max, st); });
                launch_bookkeep(w.counters.p, cur, false, 0, 0, 0, st);
                T.timed(K_DIRECT, st, [&] { launch_direct(sc->view, C, nx, w.scratch(), nxt, n_cur_max, K.direct_grid_per_cu, st); });
                if (C.enable_shadow) {
                    T.timed(K_SHADOW, st, [&] { launch_trace_shadow(sc->view, w.counters.p, nxt, n_cur_max * (uint32_t)n_dir, (uint32_t)C.pool * (uint32_t)n_dir, w.scratch(), nx.contrib, K.shadow_grid_per_cu, w.retry.list(1), st); });
                }
                T.timed(K_CLOSEST, st, [&] { launch_trace_closest(sc->view, n_cur_max, &w.counters.p->n_rays[nxt].v, nx.ray_o, nx.ray_d, nx.hit, w.retry.list(0), st); });
                cur = nxt;
            }
            HIP_TRY(hipMemcpyAsync(w.h_counters.p, w.counters.p, kCountersHeadBytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            T.collect();
            have_counters = true;
            n_cur_max = w.h_counters->n_paths[cur].v + 3u * w.h_counters->n_prays[cur].v;
            n_cur_exact = true;
            accumulate_done(st);
            continue;
        }
        const int nxt = cur ^ 1;
        Wave cw = w.wave[cur].view(), nx = w.wave[nxt].view();
        // (the counters indexed `nxt` were cleared by the previous iteration's k_bookkeep, or by k_init_free)
        // New samples are generated CONCURRENTLY with k_shade (memory-latency-bound; the primary kernel is issue-bound):
        // both append to list `nxt`.  How many fit is decided from the previous read-back: k_shade only ever adds free
        // slots and never lengthens the list, so the slots and the list room known then are still there.
        accumulate_done(s_prim);  // frees the result half that the pass after next needs; ordered before its k_primary
        if (C.mode == 0 && n_cur_max < pool && free_known >= 3u) {
            if (ctx.side[1].s) HIP_TRY(hipStreamWaitEvent(s_prim, ctx.book, 0));
            issue(nx, nxt, std::min<uint32_t>((pool - n_cur_max) / 3, free_known / 3));
        }
        if (n_cur_max > 0) T.timed(K_SHADE, st, [&] { launch_shade(sc->view, C, cw, nx, w.scratch(), cur, n_cur_max, st); });
        if (ctx.side[0].s) HIP_TRY(hipEventRecord(ctx.shaded, st));
        if (ctx.side[1].s) {  // the read-back waits for the new samples (and for a k_accumulate issued above) as well
            HIP_TRY(hipEventRecord(ctx.join[1], s_prim));
            HIP_TRY(hipStreamWaitEvent(st, ctx.join[1], 0));
        }
        HIP_TRY(hipMemcpyAsync(w.h_counters.p, w.counters.p, kCountersHeadBytes, hipMemcpyDeviceToHost, st));  // (not the sharded counters)
        HIP_TRY(hipEventRecord(ctx.readback, st));

        // queue_ahead: the rest of the iteration is queued BEFORE the host looks at the counters.  Every kernel reads the
        // true queue lengths on the device and strides over its queue, so the grids only need estimates (the ratios seen in
        // the previous iteration).  The GPU then never waits for the host round trip: while the host sizes the next
        // iteration, the three chains below are running.  Otherwise the host waits first and launches exact grids.
        uint32_t n_cont = 0, n_direct = 0;
        auto wait_counters = [&]() -> int {
            HIP_TRY(hipEventSynchronize(ctx.readback));
            if (host_delay_us > 0) usleep((useconds_t)host_delay_us);  // test hook: a slow host
            T.collect_bank(T.bank ^ 1);  // the previous iteration's kernels all finished before this iteration's k_shade
            have_counters = true;
            n_cont = w.h_counters->n_rays[nxt].v;
            n_direct = w.h_counters->n_direct[nxt].v;
            return MCPT_OK;
        };
        if (!queue_ahead) {
            const int rc = wait_counters();
            if (rc != MCPT_OK) return rc;
        }
        // (+25 %, and never fewer than 2048 workgroups' worth of lanes: a grid that is too small still works, but loses balance)
        const uint32_t grid_floor = std::min<uint32_t>(n_cur_max, 2048u * 256u);
        const uint32_t grid_cont = !queue_ahead ? n_cont : std::max<uint32_t>(grid_floor, std::min<uint32_t>(n_cur_max, (uint32_t)(1.25 * cont_ratio * n_cur_max) + 4096u));
        const uint32_t grid_direct = !queue_ahead ? n_direct : std::max<uint32_t>(grid_floor, std::min<uint32_t>(n_cur_max, (uint32_t)(1.25 * direct_ratio * n_cur_max) + 4096u));
        if (grid_cont > 0) {
            if (ctx.side[0].s) HIP_TRY(hipStreamWaitEvent(s_close, ctx.shaded, 0));
            T.timed(K_CLOSEST, s_close, [&] { launch_trace_closest(sc->view, grid_cont, queue_ahead ? &w.counters.p->n_rays[nxt].v : nullptr, nx.ray_o, nx.ray_d, nx.hit, w.retry.list(0), s_close); });
        }
        launch_bookkeep(w.counters.p, cur, false, 0, 0, 0, st);  // totals += lengths; list `cur` is consumed
        if (ctx.side[1].s) HIP_TRY(hipEventRecord(ctx.book, st));
        if (grid_direct > 0) {
            T.timed(K_DIRECT, st, [&] { launch_direct(sc->view, C, nx, w.scratch(), nxt, grid_direct, K.direct_grid_per_cu, st); });
            if (C.enable_shadow) {
                // (every workgroup of k_trace_shadow pays for the prefix sums of the queue's shards before it knows whether it has work:
                // the grid follows the observed number of shadow rays per light sample instead of covering every light sample)
                const uint32_t n_samples_max = grid_direct * (uint32_t)n_dir;
                const uint32_t grid_shadow = std::max<uint32_t>(std::min<uint32_t>(n_samples_max, 1024u * 256u),
                                                                std::min<uint32_t>(n_samples_max, (uint32_t)(1.5 * shadow_ratio * n_samples_max) + 4096u));
                T.timed(K_SHADOW, st, [&] { launch_trace_shadow(sc->view, w.counters.p, nxt, grid_shadow, (uint32_t)C.pool * (uint32_t)n_dir, w.scratch(), nx.contrib, K.shadow_grid_per_cu, w.retry.list(1), st); });
            }
        }
        // join
        if (ctx.side[0].s) {
            HIP_TRY(hipEventRecord(ctx.join[0], ctx.side[0]));
            HIP_TRY(hipStreamWaitEvent(st, ctx.join[0], 0));
        }
        if (queue_ahead) {
            const int rc = wait_counters();
            if (rc != MCPT_OK) return rc;
        }
        T.bank ^= 1;
        const uint32_t n_next = w.h_counters->n_paths[nxt].v + 3u * w.h_counters->n_prays[nxt].v;  // records + three lanes per new sample
        free_known = w.h_counters->free_tail.v - w.h_counters->free_head.v;
        if (n_cur_max > 0) {
            if (n_cur_exact) {  // (an upper bound in the denominator would under-size the next grids)
                cont_ratio = (double)n_cont / n_cur_max;
                direct_ratio = (double)n_direct / n_cur_max;
            }
            // (last_shadow: the queue k_bookkeep cleared before this read-back, i.e. the one k_direct filled two iterations ago)
            if (n_direct_prev2 > 0) shadow_ratio = std::min(1.0, (double)w.h_counters->last_shadow / ((double)n_direct_prev2 * n_dir));
        }
        n_direct_prev2 = n_direct_prev;
        n_direct_prev = n_direct;
        n_cur_max = n_next;
        n_cur_exact = true;
        cur = nxt;
    }
    // the last shadow queue was consumed after the last k_bookkeep: fold it into the totals
    HIP_TRY(hipMemcpyAsync(w.h_counters.p, w.counters.p, sizeof(Counters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    T.collect();
    const Counters &hc = *w.h_counters.p;
    tot.pushes += hc.tot_pushes + hc.pushes.v;
    tot.overflow += hc.overflow.v;
    tot.iterations += hc.tot_iterations;
    tot.shaded += hc.tot_shaded + hc.tot_ended + hc.ended.v;
    tot.direct += hc.tot_direct;
    const uint64_t shared = hc.tot_shared + hc.shared.v;
    const uint64_t pc_rays = hc.tot_pc_rays + hc.pc_rays.v;  // reflected rays k_primary walked itself (they never enter k_trace_closest's queue)
    tot.closest += hc.tot_cont + shared + pc_rays;  // resolved rays: the counts do not depend on how many of them shared a ray, nor on which kernel walked them
    tot.cont_traced += hc.tot_cont + pc_rays;
    tot.pc_samples += hc.tot_pc_samples + hc.pc_samples.v;
    tot.pc_rays += pc_rays;
    tot.cont_shared += shared;
    tot.shadow += hc.tot_shadow;
    for (uint32_t k = 0; k < kShadowShards; ++k) tot.shadow += hc.n_shadow[0][k].v + hc.n_shadow[1][k].v + hc.n_shadow_w[0][k].v + hc.n_shadow_w[1][k].v;
    return MCPT_OK;
}

int drained(int rc) {
    if (rc != MCPT_OK) {
        const std::string keep = g_err;
        (void)hipDeviceSynchronize();
        (void)hipGetLastError();
        g_err = keep;
    }
    return rc;
}

// Device bytes one pool path costs in ensure_workspace (two waves + scratch + clamp stack + free ring).
static uint64_t bytes_per_pool_path(int n_dir, int max_depth) {
    const double rays = 1.0 + 1.0 / 3.0;
    const double wave = 16 + 16 + rays * 48 + 4.0 * n_dir + 8.0 / 3.0;
    const double scratch = 3 * 16 + 4 + 32.0 * n_dir;
    const double retrace = 4.0 * (rays + n_dir + 1.0 / 3.0);  // (lists of the retry flavour; counted whether or not the tree needs them)
    return (uint64_t)(2 * wave + scratch + retrace + 16.0 * max_depth + 16.0);
}

// Uploads the owned pixels (when the partition changed), clears the framebuffer unless p.accumulate, and runs the sky cull: the culled
// pixels get spp additions of background / spp_total here.
int prepare_pixels(mcpt_scene *sc, const CameraConst &cc, const mcpt_params &p, int32_t spp, float spp_total, float *fb_dev, hipStream_t st,
                   PixelSet &ps) {
    const int W = cc.width, H = cc.height;
    // owned pixels: rebuilt and uploaded only when the partition changes (progressive calls reuse it)
    SharedBufs &sh = sc->shared;
    const int pk[5] = {W, H, p.tile_size, p.nranks > 1 ? p.rank : 0, p.nranks > 1 ? p.nranks : 1};
    if (std::memcmp(pk, sh.pix_key, sizeof pk) != 0 || !sh.pixel_list.p) {
        std::vector<uint32_t> pix;
        build_pixel_list(W, H, pk[2], pk[3], pk[4], pix);
        sh.n_pix = (uint32_t)pix.size();
        HIP_TRY(sh.pixel_list.alloc(std::max<size_t>(pix.size(), 1)));
        if (!pix.empty()) HIP_TRY(hipMemcpy(sh.pixel_list.p, pix.data(), pix.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        std::memcpy(sh.pix_key, pk, sizeof pk);
    }
    const uint32_t n_pix_owned = sh.n_pix;
    if (!p.accumulate) HIP_TRY(hipMemsetAsync(fb_dev, 0, (size_t)W * H * 3 * sizeof(float), st));

    // Pixels that can only see the background (no environment map: every sample returns the same constant) are finished here,
    // without a ray; the wavefront loop runs over the others.  csrc/mcpt_cull.hip has the conservative bound.
    uint32_t n_pix = n_pix_owned;
    const uint32_t *pixel_list = sh.pixel_list.p;
    const int4 *pixel_cand = nullptr;
    const uint32_t *sky = nullptr;
    if (sc->knobs.sky_cull && sc->view.env_w <= 0 && n_pix_owned > 0) {
        const size_t tb = cull_temp_bytes(n_pix_owned);
        HIP_TRY(sh.culled_list.alloc(n_pix_owned));
        HIP_TRY(sh.cull_flags.alloc(n_pix_owned));
        HIP_TRY(sh.cull_temp.alloc(tb));
        HIP_TRY(sh.cull_count.alloc(1));
        HIP_TRY(sh.cand_tmp.alloc(n_pix_owned));
        HIP_TRY(sh.cand_list.alloc(n_pix_owned));
        uint32_t n_trace = n_pix_owned + 1;  // (left untouched when the camera is outside what the bound covers)
        HIP_TRY(cull_sky_pixels(sc->view, cc, sh.pixel_list.p, n_pix_owned, sh.culled_list.p, sh.cull_flags.p, sh.cand_tmp.p, sh.cand_list.p, sh.cull_temp.p,
                                tb, sh.cull_count.p, &n_trace, sc->knobs.cull_rho_scale, nullptr, st));
        if (n_trace <= n_pix_owned) {  // classified: the traced pixels come first, in their original order, with their candidate lists
            sky = sh.culled_list.p + n_trace;
            launch_sky_fill(sky, n_pix_owned - n_trace, sc->view.background, spp, spp_total, fb_dev, st);
            n_pix = n_trace;
            pixel_list = sh.culled_list.p;
            // (candidate lists skip the float box tests of a primitive's ancestors: a ray that grazes a box face within rounding is a hit
            // through the list and a miss through the tree.  With the reference's own topology the kernels promise the reference's box
            // semantics exactly, so primary rays walk the tree there; the sky cull itself stays.)
            pixel_cand = sc->info.builder == 1 ? nullptr : sh.cand_list.p;
        }
    }
    ps.n_owned = n_pix_owned;
    ps.n_pix = n_pix;
    ps.list = pixel_list;
    ps.cand = pixel_cand;
    ps.sky = sky;
    return MCPT_OK;
}

// Renders the n_pix listed pixels (with their candidate entries, or none) for samples [sample_offset, sample_offset + spp), each added as
// value / spp_total into fb_dev in sample order.  With sensors as the ray source: the n_pix sensors, pixel_list and pixel_cand null, fb_dev
// the caller's n_pix * 3 floats (moments != nullptr: the per-pixel sums of v and v*v as well).  Blocks until done.
// p supplies everything else (rr_rate, n_dir_sample, shadows, seed, spp_per_pass, pool_paths, max_depth).
// sh_sink (light probes, sensors only): every pass is also folded by k_accumulate_sh, right behind k_accumulate; null: nothing changes.
int render_list(mcpt_scene *sc, const RaySource &src, const mcpt_params &p, const uint32_t *pixel_list, const int4 *pixel_cand, uint32_t n_pix,
                int32_t sample_offset, int32_t spp, float spp_total, float *fb_dev, double *moments, hipStream_t st, Clock::time_point t0,
                Totals &rt, const ShSink *sh_sink) {
    SharedBufs &sh = sc->shared;
    const int max_depth = derive_max_depth(p);
    // default: the smallest pool within 1 % of the best rate.  Measured on the chess frame (round 3, A/B on one box): 40 Mi paths 5031-5045,
    // 48 Mi 5061, 60 Mi 5052-5066 Msamples/s (round 2: 28 Mi 4467, 40 Mi 4557, 60 Mi 4617, 80 Mi 4605); 40 Mi paths are 38 GB of workspace
    uint64_t pool64 = p.pool_paths > 0 ? (uint64_t)p.pool_paths : (40ull << 20);
    pool64 = std::max<uint64_t>(pool64, 3 * 256);
    // The pass size: what the caller asks for, or (spp_per_pass 0) one chosen here.  Only two passes are in flight (one result half each), and
    // the tail of a pass -- a few long paths -- holds its half for some twenty iterations: a pass has to carry many pools' worth of samples
    // or the pool runs half empty between passes.  Measured (tools/pass_size.py, chess 1080p spp 2048; the pool holds 13.4 M samples): 1.2 M
    // traced pixels x 32 spp (3x the pool) 4263 Msamples/s, x 64 4684, x 128 4907, x 256 4997, x 512 5010, x 1024 / 2048 4880 (the result buffer
    // grows with the pass); one rank of eight (0.15 M pixels): 32 spp 2317, 256 4282, 512 4610, 1024 4732, 2048 4769.  Chosen: the power
    // of two that makes a pass at least 16 pools' worth of samples (256 spp for the 1080p chess frame: 5.5 GB of result buffers; 2048 for an eighth
    // of it), between 32 spp and the call's own spp, within a quarter of the free memory.
    // (device memory this call may use: what is free now plus what this scene's workspace and result buffer already hold; other tenants
    // of the GPU, a second scene, replicas of one group that share the device -- a rehearsal on a one-GPU box -- each take their share)
    uint64_t have = 0;
    bool have_mem = false;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (sc->knobs.fake_free_mb) free_b = std::min<size_t>(free_b, (size_t)sc->knobs.fake_free_mb << 20);  // (test hook)
            uint64_t held = 0;
            for (int k = 0; k < mcpt_scene::kMaxPools; ++k) held += (uint64_t)sc->pools[k].ws.pool * bytes_per_pool_path(sc->pools[k].ws.n_dir, sc->pools[k].ws.max_depth);
            have = ((uint64_t)free_b + held + sc->shared.result.bytes()) / (uint64_t)std::max(1, sc->device_sharers);
            have_mem = true;
        }
    }
    int s_pass_req = p.spp_per_pass;  // what the result buffer is sized for
    if (s_pass_req <= 0) {
        const uint64_t want = 16ull * (pool64 / 3) / std::max<uint32_t>(n_pix, 1u) + 1ull;
        int cap = 32;
        while (cap < spp && cap < (1 << 20)) cap *= 2;  // (no larger than the call needs: the buffer of a short call stays small)
        s_pass_req = 32;
        while ((uint64_t)s_pass_req < want && s_pass_req < cap) s_pass_req *= 2;
        if (have_mem) while (s_pass_req > 32 && (uint64_t)n_pix * s_pass_req * 3ull * 4ull * 2ull > have / 4) s_pass_req /= 2;
    }
    while ((uint64_t)n_pix * s_pass_req * 3ull > 0xfffffff0ull && s_pass_req > 1) s_pass_req /= 2;
    const int s_pass = std::min(s_pass_req, spp);
    // keep the clamp stack within 48 GiB
    while (pool64 * (uint64_t)max_depth * 16ull > (48ull << 30) && pool64 > 3 * 4096) pool64 /= 2;
    // light-sample indices (record * n_dir + k) are 32-bit
    while (pool64 * (uint64_t)p.n_dir_sample > (1ull << 31) && pool64 > 3 * 4096) pool64 /= 2;
    pool64 = std::min<uint64_t>(pool64, std::max<uint64_t>(3ull * n_pix * (uint64_t)s_pass, 3 * 256));
    // ... and the workspace within 80 % of that memory: a smaller pool is slower, never wrong
    if (have_mem) {
        const uint64_t result_b = (uint64_t)n_pix * s_pass_req * 3ull * 4ull * 2ull;
        const uint64_t budget = have * 8 / 10 > result_b ? have * 8 / 10 - result_b : 0;
        const uint64_t per = bytes_per_pool_path(p.n_dir_sample, max_depth);
        while (pool64 * per > budget && pool64 > 3 * 4096) pool64 /= 2;
    }
    // two pools (each half the paths) once a pass is big enough to keep both busy
    int n_pools = sc->n_pools;
    const uint64_t min_work = sc->knobs.pool_min_work;  // samples per pass below which one pool is used
    if ((uint64_t)n_pix * s_pass < min_work || pool64 / 2 < 3 * 256) n_pools = 1;
    const uint32_t pool = (uint32_t)(pool64 / n_pools / 3 * 3);

    // (n_pix == 0 with owned pixels: every one of them was culled; the loop below then has no samples to issue and falls through)
    const auto t_alloc0 = Clock::now();
    for (int k = 0; k < n_pools; ++k) HIP_TRY(ensure_workspace(sc->pools[k], pool, p.n_dir_sample, max_depth, stack_uses_retry(sc->view.height)));
    // two halves: a pass accumulates from one while the next pass fills the other (one half with a single pass)
    const size_t half_floats = (size_t)n_pix * s_pass * 3;
    const bool two_halves = n_pools == 1 && spp > s_pass;
    // both halves are allocated, for the REQUESTED pass size, even when this call needs less: a later call with more or longer passes
    // (a warm-up followed by the real frame) must not pay a multi-GB hipFree + hipMalloc
    HIP_TRY(sh.result.alloc((size_t)n_pix * s_pass_req * 3 * (n_pools == 1 ? 2 : 1)));
    if (sc->knobs.verbose)
        std::fprintf(stderr, "[mcpt render] %u traced pixels, pass %d spp, pool %u paths; set-up before the allocations %.1f ms, workspace + result buffers %.1f ms\n", n_pix, s_pass,
                     pool, std::chrono::duration<double, std::milli>(t_alloc0 - t0).count(), ms_since(t_alloc0));

    RenderConst C = base_consts(p, max_depth);
    C.mode = 0;
    C.pixel_list = pixel_list;
    C.pixel_cand = pixel_cand;
    C.result[0] = sh.result.p;
    C.result[1] = two_halves ? sh.result.p + half_floats : sh.result.p;
    for (int k = 0; k < n_pools; ++k) {
        sc->pools[k].timer.reset();
        sc->pools[k].timer.enabled = sc->knobs.timing;
    }
    Totals tot[mcpt_scene::kMaxPools];
    if (n_pools == 1) {
        // one pool: all passes of the call go through one pipelined schedule
        std::vector<PassPlan> plan;
        for (int k0 = 0; k0 < spp; k0 += s_pass) {
            const int s_now = std::min(s_pass, spp - k0);
            plan.push_back(PassPlan{0u, n_pix * (uint32_t)s_now, s_now, sample_offset + k0});
        }
        AccumPlan acc{fb_dev, spp_total, n_pix, pixel_list, {C.result[0], C.result[1]}, moments, sh_sink};
        const int rc = drained(run_wavefront(sc, sc->pools[0], C, src, plan, &acc, st, tot[0]));
        if (rc != MCPT_OK) return rc;
    } else {
        for (int k0 = 0; k0 < spp; k0 += s_pass) {
            const int s_now = std::min(s_pass, spp - k0);
            const uint32_t n_work = n_pix * (uint32_t)s_now;
            // pool 1 (own stream, own host thread) takes the second half of the pass; it starts after the
            // framebuffer clear / pixel-list upload / previous accumulate queued on the caller's stream
            const uint32_t half = n_work / 2;
            HIP_TRY(hipEventRecord(sc->fork, st));
            PoolCtx &c1 = sc->pools[1];
            HIP_TRY(hipStreamWaitEvent(c1.main, sc->fork, 0));
            c1.rc = MCPT_OK;
            const std::vector<PassPlan> plan0{PassPlan{0u, half, s_now, sample_offset + k0}};
            const std::vector<PassPlan> plan1{PassPlan{half, n_work - half, s_now, sample_offset + k0}};
            std::thread worker([&]() {
                if (hipSetDevice(sc->device) != hipSuccess) {
                    c1.rc = MCPT_ERR_HIP;
                    c1.err = "hipSetDevice failed in the pool thread";
                    return;
                }
                c1.rc = run_wavefront(sc, c1, C, src, plan1, nullptr, c1.main, tot[1]);
                if (c1.rc != MCPT_OK) c1.err = g_err;
            });
            const int rc0 = run_wavefront(sc, sc->pools[0], C, src, plan0, nullptr, st, tot[0]);
            worker.join();  // run_wavefront ends with a stream synchronise: both halves are complete here
            if (rc0 != MCPT_OK) return drained(rc0);
            if (c1.rc != MCPT_OK) return drained(fail(c1.rc, c1.err));
            Timer &T0 = sc->pools[0].timer;
            T0.timed(K_RESOLVE, st, [&] { launch_accumulate(C.result[0], pixel_list, n_pix, s_now, spp_total, fb_dev, moments, st); });
            if (sh_sink) T0.timed(K_RESOLVE, st, [&] { launch_accumulate_sh(C.result[0], *sh_sink, n_pix, s_now, sample_offset + k0, spp_total, st); });
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    sc->pools[0].timer.collect();
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < n_pools; ++k) {
        for (int c = 0; c < K_NCLASS; ++c) {
            tot[k].ms[c] = sc->pools[k].timer.ms[c];
            tot[k].cnt[c] = sc->pools[k].timer.count[c];
        }
        rt += tot[k];
    }
    if (sc->knobs.verbose) {
        uint64_t traced = 0, shared = 0;
        for (int k = 0; k < n_pools; ++k) {
            traced += tot[k].cont_traced;
            shared += tot[k].cont_shared;
        }
        std::fprintf(stderr, "[mcpt render] continuation rays: %llu traced, %llu shared with a sibling's\n", (unsigned long long)traced, (unsigned long long)shared);
        uint64_t pcs = 0, pcr = 0;
        for (int k = 0; k < n_pools; ++k) {
            pcs += tot[k].pc_samples;
            pcr += tot[k].pc_rays;
        }
        std::fprintf(stderr, "[mcpt render] first hits on smooth conductors finished or handed on by k_primary: %llu samples, %llu reflected rays traced there\n",
                     (unsigned long long)pcs, (unsigned long long)pcr);
    }
    return MCPT_OK;
}

}  // namespace mcpt
