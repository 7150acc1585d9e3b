// GPU BVH builder: a linear BVH built entirely on the device, as an alternative data producer to the
// host builders of mcpt_scene.cpp (which mirror BVHAccel::recursiveBuild, BVH.cpp:27-93).  Same product: one array of 64-byte
// nodes holding both child boxes and two child references, one primitive per leaf, every inner node with two children, plus the
// quantised 32-byte copy -- so the traversal kernels and their result-equivalence argument (closest hit does not depend on the
// tree; ties go to the larger primitive id) are unchanged.
//
// Pipeline (Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees and k-d trees"):
//   k_prim_boxes   one lane per primitive: exact box of the stored vertices (Triangle::getBounds, Triangle.hpp:220) or of the
//                  sphere (Sphere.hpp:58-63); scene bounds of the centroids by ordered-integer atomics
//                  (k_prim_boxes_visible: the same over the visible primitives only, mcpt_scene_set_visibility)
//   k_morton       63-bit Morton code of the centroid (21 bits per axis)
//   hipcub         radix sort of (code, primitive) pairs
//   k_hierarchy    one lane per inner node: range and split from common-prefix lengths (equal codes are told apart by position)
//   k_refit        one lane per leaf walks up; the second arrival at a node (atomic flag) writes the node's child boxes
//   k_depth        tree height (the traversal kernels size their LDS stack from it)
//   k_quantise     the 16-bit conservative boxes (minima floored, maxima ceiled, one extra cell each; done in double)
// Build time for the 296 k-triangle chess scene: a few milliseconds, against ~1.5 s for the host SAH builder; the tree is of lower
// quality (more node visits per ray), which is what the bench reports next to it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mcpt_lbvh.h"

namespace mcpt {

namespace {

constexpr int kB = 256;
inline uint32_t nblocks(uint32_t n) { return (n + kB - 1) / kB; }

// order-preserving float <-> uint mapping for atomicMin/atomicMax on floats
__device__ __forceinline__ uint32_t f2o(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float o2f(uint32_t o) {
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

struct BuildScratch {
    float *pmin, *pmax;        // [n][3] primitive boxes (indexed by primitive slot 0..n-1)
    int32_t *prim_id;          // global primitive id of slot i
    uint32_t *bounds;          // 6 ordered-uint words: centroid min xyz, max xyz
    unsigned long long *keys, *keys_sorted;
    uint32_t *vals, *vals_sorted;
    int32_t *parent_inner, *parent_leaf;
    int2 *child;               // per inner node: child references in SORTED-LEAF numbering (>= 0 inner, < 0: ~sorted position)
    float *nmin, *nmax;        // [n-1][3] bounds of inner nodes
    uint32_t *flag;
    int32_t *height;
    double *diag_sum;
};

__global__ __launch_bounds__(kB) void k_prim_boxes(const mcpt_triangle *__restrict__ tris, int n_tri, const int32_t *__restrict__ sphere_obj,
                                                    const SphereRec *__restrict__ spheres, int n_sph, BuildScratch S) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_tri + n_sph) return;
    float mn[3], mx[3];
    if (i < n_tri) {
        const mcpt_triangle t = tris[i];
        for (int a = 0; a < 3; ++a) {  // Bounds3(v0, v1) U v2: fmin/fmax of the stored vertices
            mn[a] = fminf(fminf(t.v0[a], t.v1[a]), t.v2[a]);
            mx[a] = fmaxf(fmaxf(t.v0[a], t.v1[a]), t.v2[a]);
        }
        S.prim_id[i] = i;
    } else {
        const int oi = sphere_obj[i - n_tri];
        const SphereRec s = spheres[oi];
        for (int a = 0; a < 3; ++a) {
            mn[a] = s.c[a] - s.radius;
            mx[a] = s.c[a] + s.radius;
        }
        S.prim_id[i] = n_tri + oi;
    }
    for (int a = 0; a < 3; ++a) {
        S.pmin[3 * i + a] = mn[a];
        S.pmax[3 * i + a] = mx[a];
        const float c = 0.5f * mn[a] + 0.5f * mx[a];
        atomicMin(&S.bounds[a], f2o(c));
        atomicMax(&S.bounds[3 + a], f2o(c));
    }
}

// The flavour for a scene with hidden objects (VisTable, csrc/mcpt_lbvh.h): slot i is the i-th VISIBLE primitive in id order.  The mesh
// segment of a triangle slot is found by bisection (the last segment whose first_slot <= i), as k_move_objects finds its segment.
__global__ __launch_bounds__(kB) void k_prim_boxes_visible(const mcpt_triangle *__restrict__ tris, int n_tri, const int32_t *__restrict__ sphere_obj,
                                                            const SphereRec *__restrict__ spheres, int n_sph, const VisSeg *__restrict__ segs, int n_segs,
                                                            int n_tri_ids, BuildScratch S) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_tri + n_sph) return;
    float mn[3], mx[3];
    if (i < n_tri) {
        int lo = 0, hi = n_segs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[mid].first_slot <= i) lo = mid;
            else hi = mid - 1;
        }
        const VisSeg sg = segs[lo];
        const int ti = sg.first_tri + (i - sg.first_slot);
        const mcpt_triangle t = tris[ti];
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(fminf(t.v0[a], t.v1[a]), t.v2[a]);
            mx[a] = fmaxf(fmaxf(t.v0[a], t.v1[a]), t.v2[a]);
        }
        S.prim_id[i] = ti;
    } else {
        const int oi = sphere_obj[i - n_tri];
        const SphereRec s = spheres[oi];
        for (int a = 0; a < 3; ++a) {
            mn[a] = s.c[a] - s.radius;
            mx[a] = s.c[a] + s.radius;
        }
        S.prim_id[i] = n_tri_ids + oi;
    }
    for (int a = 0; a < 3; ++a) {
        S.pmin[3 * i + a] = mn[a];
        S.pmax[3 * i + a] = mx[a];
        const float c = 0.5f * mn[a] + 0.5f * mx[a];
        atomicMin(&S.bounds[a], f2o(c));
        atomicMax(&S.bounds[3 + a], f2o(c));
    }
}

__device__ __forceinline__ unsigned long long spread21(unsigned long long x) {  // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(kB) void k_morton(int n, float3 cmin, float3 cinv, BuildScratch S) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    unsigned long long code = 0;
    const float lo[3] = {cmin.x, cmin.y, cmin.z}, inv[3] = {cinv.x, cinv.y, cinv.z};
    for (int a = 0; a < 3; ++a) {
        const float c = 0.5f * S.pmin[3 * i + a] + 0.5f * S.pmax[3 * i + a];
        float u = (c - lo[a]) * inv[a];  // [0, 1]
        u = fminf(fmaxf(u, 0.f), 1.f);
        const unsigned long long q = (unsigned long long)fminf(u * 2097152.f, 2097151.f);
        code |= spread21(q) << (2 - a);
    }
    S.keys[i] = code;
    S.vals[i] = (uint32_t)i;
}

__device__ __forceinline__ int delta(const unsigned long long *keys, int n, int i, long long j) {
    if (j < 0 || j >= n) return -1;
    const unsigned long long a = keys[i], b = keys[j];
    if (a == b) return 64 + __clz((unsigned)i ^ (unsigned)j);
    return __clzll((long long)(a ^ b));
}

__global__ __launch_bounds__(kB) void k_hierarchy(int n, BuildScratch S) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n - 1) return;
    const unsigned long long *keys = S.keys_sorted;
    const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta(keys, n, i, (long long)i - d);
    long long lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = delta(keys, n, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const long long gamma = i + s * d + (d < 0 ? -1 : 0);
    const long long lo = i < j ? i : j, hi = i < j ? j : i;
    int2 c;
    if (lo == gamma) {
        c.x = ~(int)gamma;
        S.parent_leaf[gamma] = i;
    } else {
        c.x = (int)gamma;
        S.parent_inner[gamma] = i;
    }
    if (hi == gamma + 1) {
        c.y = ~(int)(gamma + 1);
        S.parent_leaf[gamma + 1] = i;
    } else {
        c.y = (int)(gamma + 1);
        S.parent_inner[gamma + 1] = i;
    }
    S.child[i] = c;
    if (i == 0) S.parent_inner[0] = -1;
}

__device__ __forceinline__ float ld_agent(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bounds of a child reference (sorted-leaf numbering)
__device__ __forceinline__ void child_box(const BuildScratch &S, int ref, float mn[3], float mx[3]) {
    if (ref < 0) {
        const uint32_t p = S.vals_sorted[~ref];
        for (int a = 0; a < 3; ++a) {
            mn[a] = S.pmin[3 * p + a];
            mx[a] = S.pmax[3 * p + a];
        }
    } else {
        for (int a = 0; a < 3; ++a) {
            mn[a] = ld_agent(&S.nmin[3 * ref + a]);
            mx[a] = ld_agent(&S.nmax[3 * ref + a]);
        }
    }
}

__global__ __launch_bounds__(kB) void k_refit(int n, BuildScratch S, Node *__restrict__ nodes) {
    const int k = blockIdx.x * kB + threadIdx.x;
    if (k >= n) return;
    int cur = S.parent_leaf[k];
    while (cur >= 0) {
        __threadfence();
        if (atomicAdd(&S.flag[cur], 1u) == 0u) return;  // the other child's subtree is not finished: its walker will do this node
        __threadfence();
        const int2 c = S.child[cur];
        float lmn[3], lmx[3], rmn[3], rmx[3];
        child_box(S, c.x, lmn, lmx);
        child_box(S, c.y, rmn, rmx);
        Node N;
        for (int a = 0; a < 3; ++a) {
            N.lmin[a] = lmn[a];
            N.lmax[a] = lmx[a];
            N.rmin[a] = rmn[a];
            N.rmax[a] = rmx[a];
            st_agent(&S.nmin[3 * cur + a], fminf(lmn[a], rmn[a]));
            st_agent(&S.nmax[3 * cur + a], fmaxf(lmx[a], rmx[a]));
        }
        N.left = c.x < 0 ? ~S.prim_id[S.vals_sorted[~c.x]] : c.x;
        N.right = c.y < 0 ? ~S.prim_id[S.vals_sorted[~c.y]] : c.y;
        N.pad[0] = N.pad[1] = 0;
        nodes[cur] = N;
        cur = S.parent_inner[cur];
    }
}

__global__ __launch_bounds__(kB) void k_depth(int n, BuildScratch S) {
    const int k = blockIdx.x * kB + threadIdx.x;
    if (k >= n) return;
    int depth = 1, cur = S.parent_leaf[k];  // (convention of the host flattener: a leaf below d inner ancestors has depth d + 1)
    while (cur >= 0) {
        ++depth;
        cur = S.parent_inner[cur];
    }
    atomicMax(S.height, depth);
    const uint32_t p = S.vals_sorted[k];
    const float dx = S.pmax[3 * p] - S.pmin[3 * p], dy = S.pmax[3 * p + 1] - S.pmin[3 * p + 1], dz = S.pmax[3 * p + 2] - S.pmin[3 * p + 2];
    atomicAdd(S.diag_sum, (double)sqrtf(dx * dx + dy * dy + dz * dz));
}

struct QGrid {
    float origin[3], cell[3];
};

__global__ __launch_bounds__(kB) void k_quantise(int n_nodes, const Node *__restrict__ nodes, QNode *__restrict__ qn, QGrid G) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_nodes) return;
    const Node N = nodes[i];
    auto qlo = [&](float v, int a) {
        const double q = floor(((double)v - (double)G.origin[a]) / (double)G.cell[a]) - 1.0;
        return (uint32_t)fmin(65535.0, fmax(0.0, q));
    };
    auto qhi = [&](float v, int a) {
        const double q = ceil(((double)v - (double)G.origin[a]) / (double)G.cell[a]) + 1.0;
        return (uint32_t)fmin(65535.0, fmax(0.0, q));
    };
    QNode Q;
    Q.w[0] = qlo(N.lmin[0], 0) | (qlo(N.lmin[1], 1) << 16);
    Q.w[1] = qlo(N.lmin[2], 2) | (qhi(N.lmax[0], 0) << 16);
    Q.w[2] = qhi(N.lmax[1], 1) | (qhi(N.lmax[2], 2) << 16);
    Q.w[3] = qlo(N.rmin[0], 0) | (qlo(N.rmin[1], 1) << 16);
    Q.w[4] = qlo(N.rmin[2], 2) | (qhi(N.rmax[0], 0) << 16);
    Q.w[5] = qhi(N.rmax[1], 1) | (qhi(N.rmax[2], 2) << 16);
    Q.left = N.left;
    Q.right = N.right;
    qn[i] = Q;
}

// ------------------------------------------------------------------------------------------------
// PLOC: parallel locally-ordered clustering (Meister & Bittner 2018) on the Morton-sorted primitives -- the builder for trees of (near)
// SAH quality built on the device.  Bottom-up: the clusters (at first one leaf per primitive, in Morton order) look for their nearest
// neighbour -- the one whose union box has the smallest surface area -- among the kRadius clusters before and after them in the
// array; mutual nearest neighbours are merged into a new inner node, the array is compacted (order preserved), and the round repeats until
// one cluster is left.  Unlike the Karras hierarchy, whose splits follow the bits of the codes, every merge is chosen by surface area, which
// is what the SAH measures.  Each round is three small kernels, a scan and a stream synchronise.  On scenes whose union areas mostly
// differ (the chess scenes, random soups) the number of clusters falls by 35-45 % per round; where many areas are equal it depends on
// the tie rule alone.
// Ties.  Pairs are ordered by (area, |i - j|, parity of min(i, j), min(i, j)): a strict total order of the unordered pairs within the
// radius, so the best pair of the array is each other's nearest neighbour and every round merges at least one pair.  Among equal areas
// the closest cluster wins and, of the two at one distance, the one that makes a pair (2k, 2k+1): n clusters with identical boxes pair
// up everywhere and finish in ceil(log2 n) rounds with a tree of ceil(log2 n) + 1 levels.  (Ties used to go to the smaller index
// alone: then cluster 0 chose 1 and every other cluster i chose max(0, i - radius), one merge per round, a chain of n levels -- refused
// as too deep from 49 coincident primitives on; a row of 200 equal tiles took 108 rounds, now 9.)  Not a tie and unchanged: boxes nested
// in order of size chain by area alone.  DESIGN.md section 6b has the round counts; tests/bvh_model.py restates these kernels and
// tests/test_gpu_builders_model.py compares the trees node by node.
//   k_ploc_init    cluster i = leaf of the primitive at sorted position i
//   k_ploc_nn      nearest neighbour within +-radius (boxes staged through LDS; ties as above)
//   k_ploc_flags   keep / merge decision per cluster: {stays in the array, creates a node}
//   hipcub scan    positions in the compacted array and indices of the new nodes
//   k_ploc_emit    writes the new nodes (both child boxes, child references) and the next round's cluster array
// ------------------------------------------------------------------------------------------------
constexpr int kPlocMaxRadius = 64;
struct PlocArrays {
    float4 *bmin, *bmax;  // cluster boxes
    int32_t *ref;         // >= 0: inner node index; < 0: ~(global primitive id)
    int32_t *levels;      // levels of the cluster's subtree (a leaf: 1)
};

__global__ __launch_bounds__(kB) void k_ploc_init(int n, BuildScratch S, PlocArrays C) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = S.vals_sorted[i];
    C.bmin[i] = make_float4(S.pmin[3 * p], S.pmin[3 * p + 1], S.pmin[3 * p + 2], 0.f);
    C.bmax[i] = make_float4(S.pmax[3 * p], S.pmax[3 * p + 1], S.pmax[3 * p + 2], 0.f);
    C.ref[i] = ~S.prim_id[p];
    C.levels[i] = 1;
    const float dx = S.pmax[3 * p] - S.pmin[3 * p], dy = S.pmax[3 * p + 1] - S.pmin[3 * p + 1], dz = S.pmax[3 * p + 2] - S.pmin[3 * p + 2];
    atomicAdd(S.diag_sum, (double)sqrtf(dx * dx + dy * dy + dz * dz));  // (mean leaf diagonal: the quantisation rule below)
}

__device__ __forceinline__ float union_half_area(float4 amin, float4 amax, float4 bmin, float4 bmax) {
    const float dx = fmaxf(amax.x, bmax.x) - fminf(amin.x, bmin.x), dy = fmaxf(amax.y, bmax.y) - fminf(amin.y, bmin.y),
                dz = fmaxf(amax.z, bmax.z) - fminf(amin.z, bmin.z);
    return dx * dy + (dy * dz + dz * dx);
}

__global__ __launch_bounds__(kB) void k_ploc_nn(int m, int radius, PlocArrays C, int32_t *__restrict__ nn) {
    __shared__ float4 smin[kB + 2 * kPlocMaxRadius], smax[kB + 2 * kPlocMaxRadius];
    const int base = blockIdx.x * kB;
    for (int t = threadIdx.x; t < kB + 2 * radius; t += kB) {
        const int j = base - radius + t;
        if (j >= 0 && j < m) {
            smin[t] = C.bmin[j];
            smax[t] = C.bmax[j];
        }
    }
    __syncthreads();
    const int i = base + threadIdx.x;
    if (i >= m) return;
    const float4 mn = smin[threadIdx.x + radius], mx = smax[threadIdx.x + radius];
    float best = INFINITY;
    unsigned long long btie = 0;
    int bj = -1;
    for (int d = -radius; d <= radius; ++d) {
        const int j = i + d;
        if (d == 0 || j < 0 || j >= m) continue;
        const float a = union_half_area(mn, mx, smin[threadIdx.x + radius + d], smax[threadIdx.x + radius + d]);
        // equal areas: (|i - j|, parity of min(i, j), min(i, j)) -- like the area a function of the unordered pair, see the header
        const unsigned lo = (unsigned)min(i, j);
        const unsigned long long tie = ((unsigned long long)abs(d) << 33) | ((unsigned long long)(lo & 1u) << 32) | lo;
        if (bj < 0 || a < best || (a == best && tie < btie)) {
            best = a;
            btie = tie;
            bj = j;
        }
    }
    nn[i] = bj;
}

// flags[i] = {1: cluster i stays in the array (alone, or as the new node of its pair)} | {1: it creates a node} << 32
__global__ __launch_bounds__(kB) void k_ploc_flags(int m, const int32_t *__restrict__ nn, unsigned long long *__restrict__ flags) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= m) return;
    const int j = nn[i];
    const bool mutual = j >= 0 && nn[j] == i;
    const unsigned long long stays = (mutual && i > j) ? 0ull : 1ull, creates = (mutual && i < j) ? 1ull : 0ull;
    flags[i] = stays | (creates << 32);
}

__global__ __launch_bounds__(kB) void k_ploc_emit(int m, int node_base, const int32_t *__restrict__ nn, const unsigned long long *__restrict__ flags,
                                                  const unsigned long long *__restrict__ scan, PlocArrays in, PlocArrays out, Node *__restrict__ nodes,
                                                  uint32_t *__restrict__ totals) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= m) return;
    const unsigned long long f = flags[i], s = scan[i];
    if (i == m - 1) {
        totals[0] = (uint32_t)s + (uint32_t)(f & 1ull);        // clusters of the next round
        totals[1] = (uint32_t)(s >> 32) + (uint32_t)(f >> 32);  // nodes created in this round
    }
    if (!(f & 1ull)) return;
    const uint32_t pos = (uint32_t)s;
    float4 mn = in.bmin[i], mx = in.bmax[i];
    int32_t ref = in.ref[i], lv = in.levels[i];
    if (f >> 32) {
        const int j = nn[i];
        const float4 jmn = in.bmin[j], jmx = in.bmax[j];
        const int node = node_base + (int)(uint32_t)(s >> 32);
        Node N;
        N.lmin[0] = mn.x, N.lmin[1] = mn.y, N.lmin[2] = mn.z;
        N.lmax[0] = mx.x, N.lmax[1] = mx.y, N.lmax[2] = mx.z;
        N.rmin[0] = jmn.x, N.rmin[1] = jmn.y, N.rmin[2] = jmn.z;
        N.rmax[0] = jmx.x, N.rmax[1] = jmx.y, N.rmax[2] = jmx.z;
        N.left = ref;
        N.right = in.ref[j];
        N.pad[0] = N.pad[1] = 0;
        nodes[node] = N;
        mn = make_float4(fminf(mn.x, jmn.x), fminf(mn.y, jmn.y), fminf(mn.z, jmn.z), 0.f);
        mx = make_float4(fmaxf(mx.x, jmx.x), fmaxf(mx.y, jmx.y), fmaxf(mx.z, jmx.z), 0.f);
        ref = node;
        lv = 1 + max(lv, in.levels[j]);
    }
    out.bmin[pos] = mn;
    out.bmax[pos] = mx;
    out.ref[pos] = ref;
    out.levels[pos] = lv;
}

template <typename T>
hipError_t dalloc(T *&p, size_t count) {
    p = nullptr;
    return hipMalloc((void **)&p, (count ? count : 1) * sizeof(T));
}

}  // namespace

hipError_t build_lbvh_device(const mcpt_triangle *d_tris, int n_tri, const int32_t *d_sphere_obj, const SphereRec *d_spheres, int n_sph,
                             int quantise, int algo, int ploc_radius, int ploc_top, Node *d_nodes, QNode *d_qnodes, LbvhResult *out, hipStream_t st,
                             const VisTable *vis) {
    const int n = n_tri + n_sph;
    std::memset(out, 0, sizeof *out);
    if (n < 2) return hipErrorInvalidValue;
    if (vis && n_tri > 0 && (vis->n_segs < 1 || !vis->segs)) return hipErrorInvalidValue;
    BuildScratch S;
    std::memset(&S, 0, sizeof S);
    void *temp = nullptr;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    chk(dalloc(S.pmin, 3 * (size_t)n));
    chk(dalloc(S.pmax, 3 * (size_t)n));
    chk(dalloc(S.prim_id, n));
    chk(dalloc(S.bounds, 6));
    chk(dalloc(S.keys, n));
    chk(dalloc(S.keys_sorted, n));
    chk(dalloc(S.vals, n));
    chk(dalloc(S.vals_sorted, n));
    chk(dalloc(S.parent_inner, n));
    chk(dalloc(S.parent_leaf, n));
    chk(dalloc(S.child, n));
    chk(dalloc(S.nmin, 3 * (size_t)n));
    chk(dalloc(S.nmax, 3 * (size_t)n));
    chk(dalloc(S.flag, n));
    chk(dalloc(S.height, 1));
    chk(dalloc(S.diag_sum, 1));
    size_t temp_bytes = 0;
    if (e == hipSuccess) chk(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, S.keys, S.keys_sorted, S.vals, S.vals_sorted, n, 0, 63, st));
    if (e == hipSuccess) chk(hipMalloc(&temp, temp_bytes ? temp_bytes : 1));
    if (e == hipSuccess) {
        const uint32_t init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
        chk(hipMemcpyAsync(S.bounds, init, sizeof init, hipMemcpyHostToDevice, st));
        chk(hipMemsetAsync(S.flag, 0, (size_t)n * sizeof(uint32_t), st));
        chk(hipMemsetAsync(S.height, 0, sizeof(int32_t), st));
        chk(hipMemsetAsync(S.diag_sum, 0, sizeof(double), st));
    }
    if (e == hipSuccess) {
        if (vis)
            hipLaunchKernelGGL(k_prim_boxes_visible, dim3(nblocks(n)), dim3(kB), 0, st, d_tris, n_tri, d_sphere_obj, d_spheres, n_sph, vis->segs, vis->n_segs,
                               vis->n_tri_ids, S);
        else
            hipLaunchKernelGGL(k_prim_boxes, dim3(nblocks(n)), dim3(kB), 0, st, d_tris, n_tri, d_sphere_obj, d_spheres, n_sph, S);
        uint32_t hb[6];
        chk(hipMemcpyAsync(hb, S.bounds, sizeof hb, hipMemcpyDeviceToHost, st));
        chk(hipStreamSynchronize(st));
        if (e == hipSuccess) {
            float3 cmin = make_float3(o2f(hb[0]), o2f(hb[1]), o2f(hb[2]));
            const float3 cmax = make_float3(o2f(hb[3]), o2f(hb[4]), o2f(hb[5]));
            float3 cinv;
            cinv.x = cmax.x > cmin.x ? 1.0f / (cmax.x - cmin.x) : 0.f;
            cinv.y = cmax.y > cmin.y ? 1.0f / (cmax.y - cmin.y) : 0.f;
            cinv.z = cmax.z > cmin.z ? 1.0f / (cmax.z - cmin.z) : 0.f;
            hipLaunchKernelGGL(k_morton, dim3(nblocks(n)), dim3(kB), 0, st, n, cmin, cinv, S);
            chk(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, S.keys, S.keys_sorted, S.vals, S.vals_sorted, n, 0, 63, st));
            float rb[6];
            double diag = 0;
            int32_t h = 0, root = 0;
            if (algo == 0) {
                hipLaunchKernelGGL(k_hierarchy, dim3(nblocks(n - 1)), dim3(kB), 0, st, n, S);
                hipLaunchKernelGGL(k_refit, dim3(nblocks(n)), dim3(kB), 0, st, n, S, d_nodes);
                hipLaunchKernelGGL(k_depth, dim3(nblocks(n)), dim3(kB), 0, st, n, S);
                chk(hipMemcpyAsync(rb, S.nmin, 3 * sizeof(float), hipMemcpyDeviceToHost, st));      // inner node 0 is the root
                chk(hipMemcpyAsync(rb + 3, S.nmax, 3 * sizeof(float), hipMemcpyDeviceToHost, st));
                chk(hipMemcpyAsync(&h, S.height, sizeof h, hipMemcpyDeviceToHost, st));
            } else {
                // ---- PLOC rounds (see k_ploc_*)
                const int radius = std::min(std::max(ploc_radius, 1), kPlocMaxRadius);
                PlocArrays C[2];
                std::memset(C, 0, sizeof C);
                int32_t *nn = nullptr;
                unsigned long long *flags = nullptr, *scan = nullptr;
                uint32_t *totals = nullptr;
                void *scan_temp = nullptr;
                size_t scan_bytes = 0;
                for (int k = 0; k < 2; ++k) {
                    chk(dalloc(C[k].bmin, n));
                    chk(dalloc(C[k].bmax, n));
                    chk(dalloc(C[k].ref, n));
                    chk(dalloc(C[k].levels, n));
                }
                chk(dalloc(nn, n));
                chk(dalloc(flags, n));
                chk(dalloc(scan, n));
                chk(dalloc(totals, 2));
                if (e == hipSuccess) chk(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flags, scan, n, st));
                if (e == hipSuccess) chk(hipMalloc(&scan_temp, scan_bytes ? scan_bytes : 1));
                int m = n, node_base = 0, cur = 0, rounds = 0;
                // the rounds stop at `top` clusters; the tree above them is a binned-SAH build on the host (build_sah_over_clusters): a few
                // thousand boxes, a millisecond or two.  Scenes too small for that are merged down to the root here.
                // Measured (frame rate against the host SAH tree's, A/B on one box): 296 k triangles: no top -3.8 %, 4096 clusters -2.2 %,
                // 16384 -1.6 %; 38 k triangles: no top -6.5 %, 1024 -6.2 %.
                int top = std::min(ploc_top, n / 16);
                if (top < 64) top = 1;
                if (e == hipSuccess) hipLaunchKernelGGL(k_ploc_init, dim3(nblocks(n)), dim3(kB), 0, st, n, S, C[0]);
                while (e == hipSuccess && m > top) {
                    hipLaunchKernelGGL(k_ploc_nn, dim3(nblocks(m)), dim3(kB), 0, st, m, radius, C[cur], nn);
                    hipLaunchKernelGGL(k_ploc_flags, dim3(nblocks(m)), dim3(kB), 0, st, m, nn, flags);
                    chk(hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_bytes, flags, scan, m, st));
                    hipLaunchKernelGGL(k_ploc_emit, dim3(nblocks(m)), dim3(kB), 0, st, m, node_base, nn, flags, scan, C[cur], C[cur ^ 1], d_nodes, totals);
                    uint32_t tot[2] = {0, 0};
                    chk(hipMemcpyAsync(tot, totals, sizeof tot, hipMemcpyDeviceToHost, st));
                    chk(hipStreamSynchronize(st));
                    if (e != hipSuccess) break;
                    if ((int)tot[0] >= m || tot[1] == 0) {  // (cannot happen: the closest pair of the array is always mutual)
                        e = hipErrorUnknown;
                        break;
                    }
                    m = (int)tot[0];
                    node_base += (int)tot[1];
                    cur ^= 1;
                    ++rounds;
                }
                if (e == hipSuccess) {
                    std::vector<float4> bmn((size_t)m), bmx((size_t)m);
                    std::vector<int32_t> cref((size_t)m), clev((size_t)m);
                    chk(hipMemcpyAsync(bmn.data(), C[cur].bmin, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, st));
                    chk(hipMemcpyAsync(bmx.data(), C[cur].bmax, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, st));
                    chk(hipMemcpyAsync(clev.data(), C[cur].levels, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                    chk(hipMemcpyAsync(cref.data(), C[cur].ref, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                    chk(hipStreamSynchronize(st));
                    if (e == hipSuccess) {
                        root = cref[0];
                        h = clev[0];
                        if (m > 1) {  // the top of the tree: SAH over the remaining clusters
                            std::vector<Node> topn;
                            build_sah_over_clusters(m, &bmn[0].x, &bmx[0].x, cref.data(), clev.data(), node_base, topn, root, h);
                            chk(hipMemcpyAsync(d_nodes + node_base, topn.data(), topn.size() * sizeof(Node), hipMemcpyHostToDevice, st));
                            chk(hipStreamSynchronize(st));
                            node_base += (int)topn.size();
                        }
                        for (int a = 0; a < 3; ++a) rb[a] = INFINITY, rb[3 + a] = -INFINITY;
                        for (int i = 0; i < m; ++i) {
                            rb[0] = fminf(rb[0], bmn[(size_t)i].x), rb[1] = fminf(rb[1], bmn[(size_t)i].y), rb[2] = fminf(rb[2], bmn[(size_t)i].z);
                            rb[3] = fmaxf(rb[3], bmx[(size_t)i].x), rb[4] = fmaxf(rb[4], bmx[(size_t)i].y), rb[5] = fmaxf(rb[5], bmx[(size_t)i].z);
                        }
                    }
                }
                if (e == hipSuccess && node_base != n - 1) e = hipErrorUnknown;
                out->rounds = rounds;
                for (void *p : {(void *)C[0].bmin, (void *)C[0].bmax, (void *)C[0].ref, (void *)C[0].levels, (void *)C[1].bmin, (void *)C[1].bmax,
                                (void *)C[1].ref, (void *)C[1].levels, (void *)nn, (void *)flags, (void *)scan, (void *)totals, scan_temp})
                    if (p) (void)hipFree(p);
            }
            chk(hipMemcpyAsync(&diag, S.diag_sum, sizeof diag, hipMemcpyDeviceToHost, st));
            chk(hipStreamSynchronize(st));
            chk(hipGetLastError());
            if (e == hipSuccess) {
                out->root = root;
                out->height = h;
                out->n_nodes = n - 1;
                for (int a = 0; a < 3; ++a) {
                    out->root_min[a] = rb[a];
                    out->root_max[a] = rb[3 + a];
                }
                // quantisation grid: the rule of the host builder, with the MEAN leaf-box diagonal in place of the median
                QGrid G;
                double cell[3];
                bool ok = true;
                for (int a = 0; a < 3; ++a) {
                    const double ext = (double)rb[3 + a] - (double)rb[a];
                    const double pad = ext * 1e-3 + 1e-6;
                    cell[a] = (ext + 2 * pad) / 65535.0;
                    G.origin[a] = (float)((double)rb[a] - pad);
                    G.cell[a] = (float)cell[a];
                    ok = ok && std::isfinite(ext) && G.cell[a] > 0.f;
                }
                const double cd = std::sqrt(cell[0] * cell[0] + cell[1] * cell[1] + cell[2] * cell[2]);
                ok = ok && (quantise == 1 || cd * 8.0 <= diag / n);
                if (quantise == 0) ok = false;
                if (ok && d_qnodes) {
                    hipLaunchKernelGGL(k_quantise, dim3(nblocks(n - 1)), dim3(kB), 0, st, n - 1, d_nodes, d_qnodes, G);
                    chk(hipStreamSynchronize(st));
                    chk(hipGetLastError());
                    out->quantised = 1;
                    for (int a = 0; a < 3; ++a) {
                        out->q_origin[a] = G.origin[a];
                        out->q_cell[a] = G.cell[a];
                    }
                }
            }
        }
    }
    for (void *p : {(void *)S.pmin, (void *)S.pmax, (void *)S.prim_id, (void *)S.bounds, (void *)S.keys, (void *)S.keys_sorted, (void *)S.vals,
                    (void *)S.vals_sorted, (void *)S.parent_inner, (void *)S.parent_leaf, (void *)S.child, (void *)S.nmin, (void *)S.nmax,
                    (void *)S.flag, (void *)S.height, (void *)S.diag_sum, temp})
        if (p) (void)hipFree(p);
    return e;
}

}  // namespace mcpt
