// The BVH walk of the wavefront path tracer: one definition of the node visit, the descend step, the stack, the leaf test and the
// closest-hit update, used by the generic loop (traverse_loop: every query kind, node format and stack flavour) and by the lane-refill
// kernel (k_trace_closest_refill in mcpt_kernels.hip, which traces nearly every closest-hit ray of a frame).  A change to what is tested
// per ray is made here once.  Included by the translation units that define traversal kernels: mcpt_kernels.hip and mcpt_rayquery.hip.
#pragma once

#include <cfloat>

#include "mcpt_kernels.h"

namespace mcpt {

namespace {

constexpr int kBlock = 256;  // threads per workgroup of the kernels in mcpt_kernels.hip; a traversal stack is stk[level][kBlock] in LDS

MCPT_DI uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// ------------------------------------------------------------------------------------------------
// Traversal.  One lane per ray; the per-lane stack of child references lives in LDS as
// stk[level][thread] so that the 64 lanes of a wave hit 64 consecutive banks.
//
// Result equivalence with BVHAccel::getIntersection (BVH.cpp:103-116), which visits both children and
// never prunes: a primitive is tested here only if every ancestor box test of the reference passes
// (same box test, same tree), children are visited near-first, and a subtree is skipped only when its
// entry distance exceeds the best hit by a margin far above float rounding (closest hit) or lies beyond
// the light sample (shadow rays).  Equal distances go to the larger primitive id.
// ------------------------------------------------------------------------------------------------
struct TraceResult {
    double t;
    int32_t prim;
    uint32_t mat_bits;  // closest hit: material index | kMatTextured | kMatEmissive (TriGeom::mat_bits)
    bool visible;       // shadow queries only
    bool dropped;       // retry flavour: a stack entry was lost, the result is void (the ray goes to the retrace list)
};

// One traversal loop, three query kinds:
//   kClosest   closest hit (BVH.cpp:95-116); subtrees entered beyond the best hit (+margin) are skipped.
//   kWindow    shadow phase A: only subtrees whose [tmin,tmax] overlaps [dist-m, dist+m] are entered.  Finds
//              every hit the visibility test |t - dist| < EPSILON (Scene.cpp:75) could accept; a hit with
//              t <= dist - EPSILON met on the way proves occlusion at once.
//   kOccluder  shadow phase B: any hit with t <= dist - EPSILON ends the search (subtrees entered beyond dist skipped).
// The margin m = 1e-4*dist + 1e-2 is far above the float rounding of the slab test.
enum { kClosest = 0, kWindow = 1, kOccluder = 2 };

// What a query has found so far (it outlives the walk: a shadow query is a window walk followed by an occluder walk).
struct TraceState {
    double best_t;
    int32_t best_prim;
    uint32_t best_mat;
    bool occluded, found;
    bool dropped;  // a stack entry was lost (retry flavour): the result is void
#ifdef MCPT_TRAVERSAL_STATS
    unsigned nv, nt, iters, maxsp;
#endif
};
// `found`, shadow queries: the window search is already settled (k_direct found the sampled primitive in the window).
MCPT_DI void trace_reset(TraceState &st, bool found) {
    st.best_t = DBL_MAX;
    st.best_prim = -1;
    st.best_mat = 0;
    st.occluded = false;
    st.found = found;
    st.dropped = false;
#ifdef MCPT_TRAVERSAL_STATS
    st.nv = st.nt = st.iters = st.maxsp = 0;
#endif
}

constexpr int32_t kNoWork = (int32_t)0x80000000;   // neither an inner node (>= 0) nor a leaf (~index, index < 2^31 - 2)
constexpr int32_t kInstExit = (int32_t)0x80000001; // stack marker: the subtree of the current instance is exhausted
constexpr uint32_t kAllLeaves = 0x7ffffffeu;       // n_leaf_prims of a tree without instances: every ~index is a primitive

// The per-lane traversal stack: STK entries in LDS (column `tid` of stk[][kBlock]).  A ray holds at most one entry per inner ancestor
// (tree height - 1), but the deepest stack any ray of the chess frames reaches is 11-12 entries (SAH trees of height 20-24) or 14-15
// (LBVH, height 27-36; tools/traversal_stats_env.py), while every LDS entry costs 1 KB per workgroup and, beyond 19, resident
// workgroups (up to 19 entries: 8 per CU, 20-22: 7, 23-26: 6, 32: 5, 48: 3).  Three flavours:
//   plain   trees of up to 24 levels: STK >= height - 1 LDS entries, a push can never fail.
//   retry   deeper trees (MARK): 16 LDS entries; a push onto a full stack drops the entry and marks the ray (`dropped`).  The walk goes on
//           (it only visits less) and its result is thrown away: the ray goes to the kernel's RETRACE LIST (RetryList), and a small
//           kernel launched right behind (k_retrace_closest / k_retrace_shadow / k_primary_retrace) traces the listed rays again with the
//   scratch flavour (STK = 0, SCR): the whole stack is a per-lane array of kMaxBvhHeight entries in scratch memory -- slow and exact.
// The hot kernels carry no second copy of the loop: a retrace inlined behind the first walk was measured first and cost them 6-8 %
// (registers, scratch set-up, instruction cache); so did an overflow array behind the LDS entries inside the loop (a compare per pop).
// Results never depend on the stack size: the checking build (-DMCPT_FORCE_RETRY -DMCPT_STK_RETRY=4) sends most rays of every scene
// through the lists and renders the same frames (tests/test_gpu_checks.py).  Measured, chess frame with the GPU-built tree (27
// levels): 32 LDS entries 3700 Msamples/s, retry flavour 4160 (8 workgroups per CU instead of 5).
#ifndef MCPT_STK_RETRY
#define MCPT_STK_RETRY 16
#endif
constexpr int kStkRetry = MCPT_STK_RETRY;  // LDS entries of the retry flavour (the checking build: 4, and every tree uses it)

struct StackMem {
    int32_t (*lds)[kBlock];  // the workgroup's stk[STK][kBlock]
    int32_t *scr;            // scratch flavour: the lane's kMaxBvhHeight entries
    int tid;
};

// Where one ray is in the tree, with its stack.  Push and pop were macros once, after inline functions had cost the plain kernels two
// VGPRs; as forced-inline members of this local aggregate, with the flavour as template constants, they give every kernel the registers,
// spills and LDS it had with the macros (tools/kernel_resources.py before and after: profiles/traversal_refactor.txt).  What the register
// allocation does depend on is the SHAPE of the conditions around them: see walk_start and descend.
template <int STK, bool SCR, bool MARK>
struct Walk {
    StackMem m;
    int sp = 0;
    int32_t cur = kNoWork;   // the node to visit next: >= 0 inner, ~index leaf (or instance), kNoWork, kInstExit
    int32_t leaf = kNoWork;  // the parked leaf, as ~(global primitive id)
    float lim = INFINITY;    // subtrees entered beyond it are skipped
    int32_t prim_base = 0;   // first triangle of the current instance (0 at the top level: leaf indices are primitive ids)
    uint32_t n_leaf_prims = kAllLeaves;  // instanced trees: a leaf index >= n_leaf_prims is an instance

    MCPT_DI void push(int32_t v, bool &dropped) {
        if (SCR) {
            if (sp < kMaxBvhHeight) m.scr[sp++] = v;  // never full: mcpt_scene_create refuses deeper trees
        } else {
            if (sp < STK) m.lds[sp++][m.tid] = v;  // plain: never full (STK >= height - 1, asserted at creation)
            else if (MARK) dropped = true;         // retry: the entry is lost, the ray is traced again
        }
    }
    MCPT_DI int32_t pop() { return sp == 0 ? kNoWork : (SCR ? m.scr[--sp] : m.lds[--sp][m.tid]); }
    MCPT_DI bool idle() const { return cur == kNoWork && leaf == kNoWork; }
    MCPT_DI bool is_leaf(int32_t c) const { return c < 0 && (uint32_t)(~c) < n_leaf_prims; }
    MCPT_DI void park() {  // the leaf waiting in `cur` (a global primitive id from here on); the walk goes on with the stack
        leaf = ~(prim_base + ~cur);
        cur = pop();
    }
};

// A ray enters the tree: the root's box, then the root as the node to visit (or, a scene of one primitive, as the parked leaf).
// (`cur = root`, then moved to `leaf` if it is one: written as `if (leaf) .. else ..` k_trace_closest took 61 VGPRs instead of 59 and the refill kernel spilled 6 registers instead of 4.)
template <bool FAST, bool INST, class W>
MCPT_DI bool walk_start(W &w, const DevScene &S, const Ray &r, float lim) {
    w.sp = 0;
    w.cur = w.leaf = kNoWork;
    w.lim = lim;
    w.prim_base = 0;
    w.n_leaf_prims = INST ? (uint32_t)S.n_leaf_prims : kAllLeaves;
    float tm, tx;
    if (!box_hit<FAST>(S.root_min, S.root_max, r, tm, tx)) return false;
    w.cur = S.root;
    if (w.is_leaf(w.cur)) {
        w.leaf = w.cur;
        w.cur = kNoWork;
    }
    return true;
}

// NF, the node format: 0 float boxes (the exact ones: the reference's own box semantics), 1 quantised (QNode), 2 "prepared" -- the
// SMALL kernels' LDS copy of the quantised nodes, converted once per workgroup to floats RELATIVE to the grid origin (x' = q * cell), so that
// a slab bound is ONE fma, x' * inv + (origin - o) * inv, with no integer-to-float conversion per visit (12 of the ~55 vector instructions
// of a visit).  Same grid, same conservative boxes as format 1 (the error of the form is 0.4 % of the one-cell margin).
struct NodeHits {
    int32_t left, right;
    bool hl, hr;                                     // the child's box is hit
    float tl = 0.f, tr = 0.f, txl = 0.f, txr = 0.f;  // entry and exit distances
};
// The two children of inner node `cur` (every inner node has two: the builders only emit one for >= 2 primitives).  rb: the ray of the
// box tests (origin shifted inside an instance).
template <int NF, bool FAST>
MCPT_DI NodeHits node_visit(const DevScene &S, const Ray &rb, const QRay &qr, int32_t cur) {
    NodeHits h;
    if (NF == 2) {  // prepared node (LDS): float boxes relative to the grid origin
        const float4 *np = S.pnodes + 4 * cur;
        const float4 a = np[0], b = np[1], c = np[2], e = np[3];
        h.left = __float_as_int(e.x);
        h.right = __float_as_int(e.y);
        h.hl = pbox_hit<FAST>(S, rb, qr, a.x, a.y, a.z, a.w, b.x, b.y, h.tl, h.txl);
        h.hr = pbox_hit<FAST>(S, rb, qr, b.z, b.w, c.x, c.y, c.z, c.w, h.tr, h.txr);
    } else if (NF == 1) {  // 32-byte node: two 16-byte requests per lane instead of four
        const uint4 *np = reinterpret_cast<const uint4 *>(S.qnodes + cur);
        const uint4 a = np[0], b = np[1];
        h.left = (int32_t)b.z;
        h.right = (int32_t)b.w;
        h.hl = qbox_hit<FAST>(S, rb, qr, a.x & 0xffffu, a.x >> 16, a.y & 0xffffu, a.y >> 16, a.z & 0xffffu, a.z >> 16, h.tl, h.txl);
        h.hr = qbox_hit<FAST>(S, rb, qr, a.w & 0xffffu, a.w >> 16, b.x & 0xffffu, b.x >> 16, b.y & 0xffffu, b.y >> 16, h.tr, h.txr);
    } else {
        const float4 *np = reinterpret_cast<const float4 *>(S.nodes + cur);
        const float4 a = np[0], b = np[1], c = np[2], e = np[3];
        const float lmin[3] = {a.x, a.y, a.z}, lmax[3] = {a.w, b.x, b.y};
        const float rmin[3] = {b.z, b.w, c.x}, rmax[3] = {c.y, c.z, c.w};
        h.left = __float_as_int(e.x);
        h.right = __float_as_int(e.y);
        h.hl = box_hit<FAST>(lmin, lmax, rb, h.tl, h.txl);
        h.hr = box_hit<FAST>(rmin, rmax, rb, h.tr, h.txr);
    }
    return h;
}

// One step down from a visited inner node: children beyond `lim` (kWindow: or ending before `lo`) are pruned; the nearer of two goes
// first and the farther onto the stack; with none left the stack is popped.  A lane that reaches its first leaf of the round parks it
// and keeps traversing.
template <int MODE, class W>
MCPT_DI void descend(W &w, NodeHits h, float lo, TraceState &st) {
#ifdef MCPT_TRAVERSAL_STATS
    st.nv++;
#endif
    h.hl = h.hl && !(h.tl > w.lim);
    h.hr = h.hr && !(h.tr > w.lim);
    if (MODE == kWindow) {
        h.hl = h.hl && !(h.txl < lo);
        h.hr = h.hr && !(h.txr < lo);
    }
    if (h.hl && h.hr) {
        const bool swap = h.tr < h.tl;
#ifdef MCPT_TRAVERSAL_STATS
        const int sp_before = w.sp;
#endif
        w.push(swap ? h.left : h.right, st.dropped);
#ifdef MCPT_TRAVERSAL_STATS
        st.maxsp = max(st.maxsp, w.sp == sp_before ? 1000u : (unsigned)w.sp);  // (1000: a dropped entry)
#endif
        w.cur = swap ? h.right : h.left;
    } else if (h.hl) {
        w.cur = h.left;
    } else if (h.hr) {
        w.cur = h.right;
    } else {
        w.cur = w.pop();
    }
    // (operand order matters to the compiler: with `leaf == kNoWork` tested first the traversal kernels grew by 90 to 180 instructions)
    if (w.is_leaf(w.cur) && w.leaf == kNoWork) w.park();
}

// The primitive test of a leaf: triangle or sphere by index.  (k_direct tests the sampled light primitive with it, k_primary the
// candidates of a pixel.)
MCPT_DI bool leaf_hit(const DevScene &S, int32_t prim, const Ray &r, double &t, uint32_t &mat_bits) {
    if (prim < S.n_tri) {
        const TriGeom g = S.tri_geom[prim];
        double u, v;
        mat_bits = g.mat_bits;
        return tri_hit(g, r, t, u, v);
    }
    float ts = 0.f;
    const SphereRec sph = S.spheres[prim - S.n_tri];
    mat_bits = sph.mat_bits;
    const bool h = sphere_hit(sph, r, ts);
    t = (double)ts;
    return h;
}

// A hit replaces the best one if it is nearer; equal distances go to the larger primitive id.  The walk then skips what lies
// beyond it by more than the margin.
MCPT_DI void closest_update(TraceState &st, float &lim, double t, int32_t prim, uint32_t mat_bits) {
    if (t < st.best_t || (t == st.best_t && prim > st.best_prim)) {
        st.best_t = t;
        st.best_prim = prim;
        st.best_mat = mat_bits;
        lim = (float)(t + (fabs(t) * 1e-4 + 1e-2));
    }
}

// Phase 2 of a round: the parked leaf is tested (with the world ray r), and a second leaf waiting in `cur` is parked for the next round.
// Returns true when the query is decided (shadow queries: an occluder).
template <int MODE, class W>
MCPT_DI bool leaf_step(W &w, const DevScene &S, const Ray &r, float dist, TraceState &st) {
    if (w.leaf == kNoWork) return false;
#ifdef MCPT_TRAVERSAL_STATS
    st.nt++;
#endif
    const int32_t prim = ~w.leaf;
    double t = 0;
    uint32_t mb;
    if (leaf_hit(S, prim, r, t, mb)) {
        if (MODE != kClosest) {
            const double dd = t - (double)dist;
            if (dd <= -(double)kEps) {
                st.occluded = true;
                return true;
            }
            if (fabs(dd) < (double)kEps) st.found = true;
        } else {
            closest_update(st, w.lim, t, prim, mb);
        }
    }
    w.leaf = kNoWork;
    if (w.is_leaf(w.cur)) w.park();
    return false;
}

// Speculative while-while loop (Aila & Laine 2009, "Understanding the efficiency of ray traversal on GPUs").  A plain
// `if (inner) node-step else leaf-test` loop makes a wave pay for BOTH bodies in nearly every iteration (with 64 lanes, some lane
// always holds a leaf).  Here a round has two phases:
//   phase 1  inner nodes only.  A lane that reaches a leaf PARKS it and keeps descending from its stack (speculatively: the
//            parked leaf might have shortened the ray); a lane that reaches a second leaf, or runs out of work, waits.  The phase ends
//            when at most kLeafVote lanes of the wave are still looking for their first leaf.
//   phase 2  every lane tests its parked leaf; a second leaf waiting in `cur` is parked for the next round.
// Measured on the chess frame (A/B on one box, same build otherwise): plain loop 4190 Msamples/s; this loop with vote 0: 4375,
// 4: 4515, 8: 4540, 12: 4540, 16: 4525; testing the second leaf in the same round instead of parking it: 4430.  The serialised
// k_trace_closest went from 82.5 to 72 ms per 2 x 256 spp.  Same tests, same results: the order of primitive tests does not
// matter (ties go to the larger primitive id), and the pruning margins are unchanged.
//
// INST (scenes with instanced objects, csrc/mcpt_scene.cpp): a leaf index >= n_leaf_prims is an instance.  Entering it moves the
// origin used by the BOX tests by -shift, pushes an exit marker and continues in the prototype's shared subtree, whose leaves hold
// local triangle indices; primitive tests always use the world ray and the object's own world-space triangle
// (first_tri + local index), so hits are exactly those of the un-instanced tree.  Popping the marker restores the origin.
#ifndef MCPT_LEAF_VOTE
#define MCPT_LEAF_VOTE 12
#endif
constexpr int kLeafVote = MCPT_LEAF_VOTE;

template <int MODE, int STK, bool SCR, bool MARK, bool FAST, int NF, bool INST>
MCPT_DI void traverse_loop(const DevScene &S, const Ray &r, float dist, const StackMem &m, TraceState &st) {
    constexpr bool QUANT = NF != 0;
    static_assert(NF != 2 || !INST, "prepared nodes: small scenes, never instanced");
    QRay qr;
    if (QUANT) qr = make_qray(S, r);
    Ray rb = r;  // the ray of the box tests (origin shifted inside an instance)
    const float margin = dist * 1e-4f + 1e-2f;
    const float lo = dist - margin;
    Walk<STK, SCR, MARK> w{m};
    if (!walk_start<FAST, INST>(w, S, r, (MODE == kClosest) ? INFINITY : (dist + margin))) return;
    while (true) {
        // ---- phase 1: inner nodes
        while (true) {
#ifdef MCPT_TRAVERSAL_STATS
            st.iters++;
#endif
            if (INST) {
                if (w.cur == kInstExit) {  // back to the top level
                    rb.o = r.o;
                    w.prim_base = 0;
                    if (QUANT) qr.b = make_qray(S, r).b;
                    w.cur = w.pop();
                }
                if (w.cur > kInstExit && w.cur < 0 && !w.is_leaf(w.cur)) {  // an instance: enter its prototype's subtree
                    const InstRec I = S.inst[(uint32_t)(~w.cur) - w.n_leaf_prims];
                    rb.o = mk3(r.o.x - I.shift[0], r.o.y - I.shift[1], r.o.z - I.shift[2]);
                    w.prim_base = I.first_tri;
                    if (QUANT) qr.b = make_qray(S, rb).b;
                    w.push(kInstExit, st.dropped);
                    w.cur = I.root;
                }
            }
            if (w.cur >= 0) descend<MODE>(w, node_visit<NF, FAST>(S, rb, qr, w.cur), lo, st);
            // a lane can still make progress on nodes if it holds an inner node (or, INST, an instance / exit marker)
            const bool workable = INST ? (w.cur >= 0 || (w.cur > kNoWork && !w.is_leaf(w.cur))) : (w.cur >= 0);
            if (__popcll(__ballot(w.leaf == kNoWork && workable)) <= kLeafVote) break;
        }
        // ---- phase 2: the parked leaf
        if (leaf_step<MODE>(w, S, r, dist, st) || w.idle()) return;
    }
}

// The dispatch of one query over the loop's instantiations.  Node format and instancing:
template <int MODE, bool FAST, int STK, bool SCR, bool MARK, bool PREP>
MCPT_DI void traverse_nodes(const DevScene &S, const Ray &r, float dist, const StackMem &m, TraceState &st) {
    if (PREP && S.pnodes) {  // SMALL kernels of a scene with quantised nodes
        traverse_loop<MODE, STK, SCR, MARK, FAST, (PREP ? 2 : 1), false>(S, r, dist, m, st);
    } else if (S.inst) {
        if (S.qnodes) traverse_loop<MODE, STK, SCR, MARK, FAST, 1, true>(S, r, dist, m, st);
        else traverse_loop<MODE, STK, SCR, MARK, FAST, 0, true>(S, r, dist, m, st);
    } else {
        if (S.qnodes) traverse_loop<MODE, STK, SCR, MARK, FAST, 1, false>(S, r, dist, m, st);
        else traverse_loop<MODE, STK, SCR, MARK, FAST, 0, false>(S, r, dist, m, st);
    }
}
// Query kind.  Shadow queries, Scene.cpp:74-75: a light sample counts iff the CLOSEST hit lies within EPSILON of the light distance, i.e.
// iff some hit lies in the window AND no hit lies at or below dist - EPSILON.
template <bool SHADOW, bool FAST, int STK, bool SCR, bool MARK, bool PREP>
MCPT_DI void traverse_kind(const DevScene &S, const Ray &r, float dist, const StackMem &m, bool found, TraceState &st) {
    if (SHADOW) {
        if (!found) traverse_nodes<kWindow, FAST, STK, SCR, MARK, PREP>(S, r, dist, m, st);
        if (st.found && !st.occluded) traverse_nodes<kOccluder, FAST, STK, SCR, MARK, PREP>(S, r, dist, m, st);
    } else {
        traverse_nodes<kClosest, FAST, STK, SCR, MARK, PREP>(S, r, dist, m, st);
    }
}
// Slab-test flavour (wave-uniform): the exact NaN-faithful chain only when some lane of the wave has a non-finite reciprocal, i.e. a
// zero direction component; otherwise the bit-identical max3/min3 form.
template <bool SHADOW, int STK, bool SCR, bool MARK, bool PREP>
MCPT_DI void traverse_query(const DevScene &S, const Ray &r, float dist, const StackMem &m, bool found, TraceState &st) {
    if (__all(ray_is_plain(r)) != 0) traverse_kind<SHADOW, true, STK, SCR, MARK, PREP>(S, r, dist, m, found, st);
    else traverse_kind<SHADOW, false, STK, SCR, MARK, PREP>(S, r, dist, m, found, st);
}

MCPT_DI TraceResult trace_result(const TraceState &st) { return TraceResult{st.best_t, st.best_prim, st.best_mat, !st.occluded && st.found, st.dropped}; }

template <bool SHADOW, int STK, bool RETRY, bool PREP = false>
MCPT_DI TraceResult traverse(const DevScene &S, const Ray &r, float dist, int32_t (*stk)[kBlock], int tid, bool found = false) {
    TraceState st;
    trace_reset(st, found);
    traverse_query<SHADOW, STK, false, RETRY, PREP>(S, r, dist, StackMem{stk, nullptr, tid}, found, st);
#ifdef MCPT_TRAVERSAL_STATS
    if (S.dbg) {  // [kind*8 + {rays, node visits, prim tests, occluded/hit, wave-iterations*64, found}]
        const int base = SHADOW ? 8 : 0;
        atomicAdd(&S.dbg[base + 0], 1ull);
        atomicAdd(&S.dbg[base + 1], (unsigned long long)st.nv);
        atomicAdd(&S.dbg[base + 2], (unsigned long long)st.nt);
        atomicAdd(&S.dbg[base + 3], (unsigned long long)(SHADOW ? (st.occluded ? 1 : 0) : (st.best_prim >= 0 ? 1 : 0)));
        unsigned mx = st.iters;
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        if (lane_id() == 0) atomicAdd(&S.dbg[base + 4], (unsigned long long)mx * 64ull);
        atomicAdd(&S.dbg[base + 5], (unsigned long long)(SHADOW ? (st.found ? 1 : 0) : 0));
        atomicMax(&S.dbg[SHADOW ? 7 : 6], (unsigned long long)st.maxsp);  // deepest stack of any ray (1000: an entry was dropped)
    }
#endif
    return trace_result(st);
}

// The retrace of one listed ray: again, from the start, with the whole stack in a per-lane array (the scratch flavour of Walk).
template <bool SHADOW>
MCPT_DI TraceResult traverse_scratch(const DevScene &S, const Ray &r, float dist, int32_t (*stk)[kBlock], int tid, bool found = false) {
    int32_t scr[kMaxBvhHeight];
    TraceState st;
    trace_reset(st, found);
    traverse_query<SHADOW, 0, true, false, false>(S, r, dist, StackMem{stk, scr, tid}, found, st);
    return trace_result(st);
}

MCPT_DI void retry_append(const RetryList &rl, uint32_t v) {  // (one atomic per lost ray: there are next to none)
    const uint32_t k = atomicAdd(rl.count, 1u);
    if (k < rl.cap) rl.items[k] = v;
}
// end of a retrace kernel: the last workgroup to finish clears the list for the next launch
MCPT_DI void retry_finish(const RetryList &rl) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(rl.done, 1u) == gridDim.x - 1u) {
            *rl.count = 0u;
            *rl.done = 0u;
        }
    }
}

MCPT_DI uint4 pack_hit(double t, int32_t prim, uint32_t mat_bits) {  // {t lo, t hi, prim, TriGeom::mat_bits}
    const unsigned long long tb = (unsigned long long)__double_as_longlong(t);
    return make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)prim, mat_bits);
}

}  // namespace

}  // namespace mcpt
