// GPU LBVH builder (csrc/mcpt_lbvh.hip): builds the traversal tree of a scene on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "mcpt_internal.h"

namespace mcpt {

struct LbvhResult {
    int32_t root, height, n_nodes, quantised;
    int32_t rounds;  // PLOC: merge rounds
    float root_min[3], root_max[3];
    float q_origin[3], q_cell[3];
};

// d_tris: the caller's triangles (exact stored vertices) on the device; d_sphere_obj: object index of every sphere object;
// d_spheres: SphereRec array indexed by object index.  Primitive ids: triangle index, or n_tri + object index for a sphere.
// Needs n_tri + n_sph >= 2.  d_nodes / d_qnodes: n - 1 entries each, written by the build (d_qnodes may stay unused: see
// LbvhResult::quantised).  quantise: -1 automatic, 0 never, 1 always.  Synchronises `st`.
// algo 0: linear BVH (Karras hierarchy over the Morton codes: the fastest build); 1: PLOC, parallel locally-ordered clustering with
// search radius `ploc_radius` over the same Morton order (merges chosen by surface area: near-SAH quality, a few ms); the merge rounds
// stop at `ploc_top` clusters and the top of the tree is a binned-SAH build over them on the host (0 / 1: merge down to the root).
//
// Visibility (mcpt_scene_set_visibility).  `vis` == nullptr: every primitive goes into the tree, as above.  Otherwise only the listed
// ones do: vis->segs holds one entry per visible mesh, sorted by first_slot, and builder slot first_slot + k is triangle first_tri + k
// (k < count); n_tri is then the number of VISIBLE triangles (the sum of the counts), vis->n_tri_ids the number of triangles the scene
// stores (sphere ids are n_tri_ids + object index), and d_sphere_obj / n_sph list the visible spheres only.  Slots stay in increasing id
// order, so the tree is the one a scene of the visible primitives alone gets, with the stored ids in its leaves.  The precondition is on
// the visible count: n_tri + n_sph >= 2, and d_nodes / d_qnodes hold n_tri + n_sph - 1 entries.
struct VisSeg {
    int32_t first_slot, first_tri, count;
};
struct VisTable {
    const VisSeg *segs;  // device pointer; n_segs >= 1 whenever n_tri > 0
    int32_t n_segs;
    int32_t n_tri_ids;
};
hipError_t build_lbvh_device(const mcpt_triangle *d_tris, int n_tri, const int32_t *d_sphere_obj, const SphereRec *d_spheres, int n_sph,
                             int quantise, int algo, int ploc_radius, int ploc_top, Node *d_nodes, QNode *d_qnodes, LbvhResult *out, hipStream_t st,
                             const VisTable *vis = nullptr);

}  // namespace mcpt
