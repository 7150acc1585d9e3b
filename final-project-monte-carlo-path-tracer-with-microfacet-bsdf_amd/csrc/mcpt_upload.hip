// Scene create / upload / destroy / info and the BVH dumps of the C ABI (include/mcpt.h); mcpt_last_error and mcpt_version.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>

#include "mcpt_host.h"
#include "mcpt_lbvh.h"
#include "mcpt_move.h"

using namespace mcpt;

thread_local std::string mcpt::g_err;

void Knobs::read() {
    auto off = [](const char *n) { const char *v = std::getenv(n); return v && v[0] == '0'; };
    overlap = !off("MCPT_OVERLAP");
    queue_ahead = !off("MCPT_QUEUE_AHEAD");
    timing = !off("MCPT_TIMING");
    verbose = std::getenv("MCPT_RENDER_VERBOSE") != nullptr;
    sky_cull = !off("MCPT_SKY_CULL");
    small_scene = !off("MCPT_SMALL_SCENE");
    share_rays = !off("MCPT_SHARE_RAYS");
    primary_conductor = !off("MCPT_PRIMARY_CONDUCTOR");
    const char *v;
    if ((v = std::getenv("MCPT_POOLS"))) pools = (v[0] == '2') ? 2 : 1;
    if ((v = std::getenv("MCPT_DRAIN_BATCH"))) drain_batch = std::max(1, std::atoi(v));
    if ((v = std::getenv("MCPT_POOL_MIN_WORK"))) pool_min_work = (uint64_t)std::max(1, std::atoi(v));
    if ((v = std::getenv("MCPT_SHADOW_GRID_PER_CU"))) shadow_grid_per_cu = (uint32_t)std::max(1, std::atoi(v));
    if ((v = std::getenv("MCPT_DIRECT_GRID_PER_CU"))) direct_grid_per_cu = (uint32_t)std::max(0, std::atoi(v));
    if ((v = std::getenv("MCPT_QUERY_CHUNK"))) query_chunk = (uint32_t)std::max(64, std::atoi(v));
#ifdef MCPT_TEST_HOOKS
    if ((v = std::getenv("MCPT_RING_START"))) ring_start = (uint32_t)std::strtoul(v, nullptr, 0);
    if ((v = std::getenv("MCPT_HOST_DELAY_US"))) host_delay_us = std::atoi(v);
    if ((v = std::getenv("MCPT_HALFSPACE_SLACK_SCALE"))) halfspace_slack_scale = (float)std::atof(v);
    if ((v = std::getenv("MCPT_TIR_BOUND_SCALE"))) tir_bound_scale = (float)std::atof(v);
    if ((v = std::getenv("MCPT_CONE_TOL_SCALE"))) cone_tol_scale = (float)std::atof(v);
    if ((v = std::getenv("MCPT_CULL_RHO_SCALE"))) cull_rho_scale = (float)std::atof(v);
    if ((v = std::getenv("MCPT_FAKE_FREE_MB"))) fake_free_mb = (uint64_t)std::max(1, std::atoi(v));
#endif
}

// First use of a device by this process: context creation and the load of this library's code objects cost 100-150 ms (round 2's
// `upload_ms` of 129-155 ms for a 6.8 KB scene was exactly this, not the copies).  It does not depend on the scene, so it runs on a
// helper thread while the calling thread flattens the scene and builds its tree, and it is reported on its own (mcpt_scene_info).
double mcpt::warm_up_device(int device) {
    const auto t0 = Clock::now();
    if (hipSetDevice(device) != hipSuccess) return 0.0;
    uint32_t *p = nullptr;
    if (hipMalloc((void **)&p, 256) == hipSuccess) {
        launch_add_frame(reinterpret_cast<float *>(p), reinterpret_cast<float *>(p), 0u, nullptr);  // (n = 0: no launch; keeps the symbol referenced)
        (void)hipMemset(p, 0, 256);
        launch_mask_unowned(reinterpret_cast<float *>(p), 1, 1, 1, 0, 1, nullptr);  // one tiny kernel of this library: forces its code objects in
        (void)hipDeviceSynchronize();
        (void)hipFree(p);
    }
    (void)hipGetLastError();
    return ms_since(t0);
}

int mcpt::build_scene_host(const mcpt_scene_desc *desc, const mcpt_build_options *options, HostBuild &hb) {
    if (!desc) return fail(MCPT_ERR_ARG, "mcpt_scene_create: null argument");
    const char *err = "";
    const auto t_build = Clock::now();
    hb.choice = resolve_build_choice(options);
    // (a single primitive has no inner node: nothing for the device builder to do)
    if ((hb.choice.builder == MCPT_BUILD_GPU_LBVH || hb.choice.builder == MCPT_BUILD_GPU_PLOC) && desc->objects) {
        int64_t n_prim = desc->n_triangles;
        for (int i = 0; i < desc->n_objects; ++i) n_prim += desc->objects[i].kind == MCPT_OBJ_SPHERE ? 1 : 0;
        if (n_prim < 2) hb.choice.builder = MCPT_BUILD_SAH;
    }
    const int rc = build_host_scene(*desc, hb.hs, &err, hb.choice);
    if (rc != MCPT_OK) return fail(rc, std::string("mcpt_scene_create: ") + err);
    hb.build_ms = ms_since(t_build);
    return MCPT_OK;
}

namespace {

SceneMeta meta_of(const HostScene &hs) {
    SceneMeta m;
    m.root = hs.root;
    m.height = hs.height;
    m.n_inner = hs.root < 0 ? 0 : (int32_t)hs.nodes.size();  // (device builders: set by build_device_tree)
    m.n_leaf_prims = hs.n_leaf_prims;
    for (int k = 0; k < 3; ++k) {
        m.root_min[k] = hs.root_min[k];
        m.root_max[k] = hs.root_max[k];
        m.q_origin[k] = hs.q_origin[k];
        m.q_cell[k] = hs.q_cell[k];
        m.background[k] = hs.background[k];
        m.light_center[k] = hs.light_center[k];
    }
    m.n_triangles = hs.n_triangles;
    m.n_objects = hs.n_objects;
    m.builder = hs.builder;
    m.n_instances = (int32_t)hs.instances.size();
    m.n_sphere_slots = (int32_t)hs.spheres.size();
    m.n_mats = (int32_t)hs.materials.size();
    m.n_lights = (int32_t)hs.lights.size();
    m.n_light_nodes = (int32_t)hs.light_nodes.size();
    m.n_light_tris = (int32_t)hs.light_tris.size();
    m.env_w = hs.env_w;
    m.env_h = hs.env_h;
    m.light_area_sum = hs.light_area_sum;
    m.light_radius = hs.light_radius;
    return m;
}

// What the device builders need to leave hidden objects out (VisTable, csrc/mcpt_lbvh.h): one {first_slot, first_tri, count} entry per
// visible mesh in triangle-array order, and the visible sphere objects.  A few bytes per object; formed on the host from the object list.
struct DevVis {
    DevBuf<VisSeg> segs;
    DevBuf<int32_t> sph;
    int32_t n_segs = 0, n_tri = 0, n_sph = 0;
    bool active = false;  // false: every object is visible, the builders run as they do without a table
};
int32_t count_visible_prims(const SceneSource &S, const std::vector<uint8_t> &visible) {
    int32_t n = 0;
    for (size_t o = 0; o < S.objects.size(); ++o)
        if (visible[o]) n += S.objects[o].kind == MCPT_OBJ_MESH ? S.objects[o].n_tri : 1;
    return n;
}
int upload_vis(const SceneSource &S, const std::vector<uint8_t> &visible, DevVis &dv) {
    dv.active = std::find(visible.begin(), visible.end(), (uint8_t)0) != visible.end();
    if (!dv.active) return MCPT_OK;
    std::vector<VisSeg> segs;
    std::vector<int32_t> sph;
    for (size_t o = 0; o < S.objects.size(); ++o) {
        if (!visible[o]) continue;
        if (S.objects[o].kind == MCPT_OBJ_MESH) segs.push_back(VisSeg{0, S.objects[o].first_tri, S.objects[o].n_tri});
        else sph.push_back((int32_t)o);
    }
    std::sort(segs.begin(), segs.end(), [](const VisSeg &a, const VisSeg &b) { return a.first_tri < b.first_tri; });
    int32_t slot = 0;
    for (VisSeg &sg : segs) {
        sg.first_slot = slot;
        slot += sg.count;
    }
    dv.n_segs = (int32_t)segs.size();
    dv.n_tri = slot;
    dv.n_sph = (int32_t)sph.size();
    HIP_TRY(upload(dv.segs, segs));
    HIP_TRY(upload(dv.sph, sph));
    return MCPT_OK;
}

// The traversal tree of a device-built scene (csrc/mcpt_lbvh.hip), from triangles and sphere records that are on the device, into
// g.nodes / g.qnodes; the tree fields of `meta` are the builder's.
// `dv` active (some object is hidden): the builder gets the visible triangle ranges and the visible spheres, and the node arrays are sized
// by the visible count.  d_spheres: the SphereRec array the builder reads (g's own unless the caller builds a tree alone).
int build_device_tree(const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, int n_sph, const BuildChoice &choice, GeomBufs &g, SceneMeta &meta,
                      const DevVis *dv = nullptr, const SphereRec *d_spheres = nullptr) {
    const bool masked = dv && dv->active;
    const int n_tri = masked ? dv->n_tri : meta.n_triangles;
    if (masked) {
        d_sphere_obj = dv->sph.p;
        n_sph = dv->n_sph;
    }
    const VisTable vt{masked ? dv->segs.p : nullptr, masked ? dv->n_segs : 0, meta.n_triangles};
    const int n_prim = n_tri + n_sph;
    if (n_prim < 2) return fail(MCPT_ERR_ARG, "GPU BVH build: fewer than two visible primitives");
    hipError_t e = g.nodes.alloc((size_t)n_prim - 1);
    if (e == hipSuccess) e = g.qnodes.alloc((size_t)n_prim - 1);
    LbvhResult R;
    if (e == hipSuccess) e = build_lbvh_device(d_tris, n_tri, d_sphere_obj, d_spheres ? d_spheres : g.spheres.p, n_sph, choice.quantise, meta.builder == 3 ? 1 : 0, choice.ploc_radius, choice.ploc_top,
                                             g.nodes.p, g.qnodes.p, &R, nullptr, masked ? &vt : nullptr);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? MCPT_ERR_OOM : MCPT_ERR_HIP, std::string("GPU BVH build: ") + hipGetErrorString(e));
    if (R.height > kMaxBvhHeight) return fail(MCPT_ERR_LIMIT, "the GPU-built BVH is deeper than the traversal stack (kMaxBvhHeight); use MCPT_BUILD_SAH");
    meta.root = R.root;
    meta.height = R.height;
    for (int k = 0; k < 3; ++k) {
        meta.root_min[k] = R.root_min[k];
        meta.root_max[k] = R.root_max[k];
        meta.q_origin[k] = R.q_origin[k];
        meta.q_cell[k] = R.q_cell[k];
    }
    if (!R.quantised) g.qnodes.release();
    meta.n_inner = R.n_nodes;
    return MCPT_OK;
}

// The device tree of an edit's device path: build_device_tree, then the depth check every tree gets before it is swapped in.
int build_device_tree_checked(const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, int n_sph, const BuildChoice &choice, GeomBufs &g, SceneMeta &meta,
                              const DevVis *dv, const SphereRec *d_spheres = nullptr) {
    const int rc = build_device_tree(d_tris, d_sphere_obj, n_sph, choice, g, meta, dv, d_spheres);
    if (rc == MCPT_OK && traversal_stack_entries(meta.height) < meta.height - 1)
        return fail(MCPT_ERR_LIMIT, "the BVH is deeper than the traversal stack (kMaxBvhHeight)");
    return rc;
}

// Copies the arrays of a flattened scene that depend on where its objects are into `g`; for the device builders the tree is then built
// there from d_tris (the triangles `hs` was flattened from).  Shared by mcpt_scene_create and the host path of mcpt_scene_update.
int upload_geometry(const HostScene &hs, const BuildChoice &choice, const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, GeomBufs &g, SceneMeta &meta,
                    double &gpu_build_ms, const DevVis *dv = nullptr) {
    hipError_t e = hipSuccess;
    auto up = [&](auto &buf, const auto &vec) {
        if (e == hipSuccess) e = upload(buf, vec);
    };
    if (hs.builder < 2) {
        up(g.nodes, hs.nodes);
        if (!hs.qnodes.empty()) up(g.qnodes, hs.qnodes);
    }
    up(g.tri_geom, hs.tri_geom);
    up(g.tri_shade, hs.tri_shade);
    up(g.spheres, hs.spheres);
    up(g.lights, hs.lights);
    up(g.light_nodes, hs.light_nodes);
    up(g.light_tris, hs.light_tris);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? MCPT_ERR_OOM : MCPT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    gpu_build_ms = 0.0;
    if (hs.builder >= 2) {  // the traversal tree is built on the device from the caller's triangles (csrc/mcpt_lbvh.hip)
        const auto tb = Clock::now();
        const int rc = build_device_tree(d_tris, d_sphere_obj, (int)hs.sphere_objects.size(), choice, g, meta, dv);
        if (rc != MCPT_OK) return rc;
        gpu_build_ms = ms_since(tb);
    }
    if (traversal_stack_entries(meta.height) < meta.height - 1)  // whatever built the tree: a push beyond the stack (one entry per inner ancestor) would be dropped
        return fail(MCPT_ERR_LIMIT, "the BVH is deeper than the traversal stack (kMaxBvhHeight)");
    return MCPT_OK;
}

// DevScene and the geometry fields of mcpt_scene_info from the scene's arrays and sc->meta: after creation and after every update.
void fill_view(mcpt_scene *sc) {
    const SceneMeta &m = sc->meta;
    const GeomBufs &g = sc->geom;
    DevScene &v = sc->view;
    v.nodes = g.nodes.p;
    v.light_area_sum = m.light_area_sum;
    v.qnodes = g.qnodes.p;  // nullptr: the float nodes are traversed
    v.pnodes = nullptr;     // (set by the SMALL kernels to their LDS copy)
    for (int k = 0; k < 3; ++k) {
        v.q_origin[k] = m.q_origin[k];
        v.q_cell[k] = m.q_cell[k];
    }
    v.tri_geom = g.tri_geom.p;
    v.tri_shade = g.tri_shade.p;
    v.spheres = g.spheres.p;
    v.mats = sc->mats.p;
    v.lights = g.lights.p;
    v.light_nodes = g.light_nodes.p;
    v.light_tris = g.light_tris.p;
    v.inst = m.n_instances == 0 ? nullptr : sc->inst.p;
    v.n_leaf_prims = m.n_leaf_prims;
    v.env = sc->env.p;
    for (int k = 0; k < 3; ++k) {
        v.root_min[k] = m.root_min[k];
        v.root_max[k] = m.root_max[k];
        v.background[k] = m.background[k];
    }
    v.root = m.root;
    v.n_tri = m.n_triangles;
    v.n_lights = m.n_lights;
    v.env_w = m.env_w;
    v.env_h = m.env_h;
    v.height = m.height;
    for (int k = 0; k < 3; ++k) v.light_center[k] = m.light_center[k];
    v.light_radius = m.light_radius;
    {  // the half-space rule's margin (direct_is_zero): relative to every length whose rounding enters, scaled by the checking build's knob
        const float k = kHalfspaceSlack * sc->knobs.halfspace_slack_scale;
        const float c1 = std::fabs(m.light_center[0]) + std::fabs(m.light_center[1]) + std::fabs(m.light_center[2]);
        v.light_plane[0] = m.light_radius + k * (c1 + m.light_radius);
        v.light_plane[1] = k;
    }
    v.tir_bound_factor = 1.001f * sc->knobs.tir_bound_scale;
    v.cone_tol_scale = sc->knobs.cone_tol_scale;
    v.n_inner = m.n_inner;
    v.n_sphere_slots = m.n_sphere_slots;
    v.n_mats = m.n_mats;
    v.n_light_nodes = m.n_light_nodes;
    v.n_light_tris = m.n_light_tris;
    // the LDS-resident flavour (SMALL kernels): everything the traversal and light sampling read fits the kSmall* limits
    v.small = 0;
#if !defined(MCPT_FORCE_RETRY) && !defined(MCPT_LDS_ONLY_STACKS)
    if (sc->knobs.small_scene && !v.inst && v.root >= 0 && v.n_inner <= kSmallNodes && v.n_tri <= kSmallTris && v.n_sphere_slots <= kSmallSphereSlots &&
        v.n_mats <= kSmallMats && v.n_lights <= kSmallLights && v.n_light_nodes <= kSmallLightNodes && v.n_light_tris <= kSmallLightTris &&
        v.height - 1 <= kSmallStk)
        v.small = 1;
#endif
    v.dbg = sc->dbg.p;
    sc->info.builder = m.builder;
    sc->info.quantised = g.qnodes.p ? 1 : 0;
    sc->info.n_instances = m.n_instances;
    sc->info.lds_resident = v.small;
    sc->info.n_nodes = m.n_inner;
    sc->info.bvh_height = m.height;
    sc->info.n_lights = v.n_lights;
    sc->info.n_prims = m.n_triangles + m.n_objects;
    sc->info.scene_bytes = g.nodes.bytes() + g.qnodes.bytes() + g.tri_geom.bytes() + g.tri_shade.bytes() + g.spheres.bytes() + sc->mats.bytes() +
                           g.lights.bytes() + g.light_nodes.bytes() + g.light_tris.bytes() + sc->inst.bytes() + sc->env.bytes() + sc->tris0.bytes() +
                           g.tris.bytes() + sc->sphere_obj.bytes();
}

using mat::emits;  // Material::hasEmission (Material.hpp:262), as build_host_scene decides it

}  // namespace

// The device half of mcpt_scene_create: copies a flattened scene to `device` (and, for MCPT_BUILD_GPU_LBVH, builds the tree there).
// mcpt_group_create builds the host scene ONCE and calls this from one thread per device.
int mcpt::upload_scene(const mcpt_scene_desc *desc, HostBuild &hb, int device, mcpt_scene **out) {
    HostScene &hs = hb.hs;
    const BuildChoice &choice = hb.choice;
    HIP_TRY(hipSetDevice(device));
    const auto t_upload = Clock::now();

    // (an error exit below destroys what exists so far, with this device current)
    std::unique_ptr<mcpt_scene, decltype(&mcpt_scene_destroy)> sc(new (std::nothrow) mcpt_scene(), mcpt_scene_destroy);
    if (!sc) return fail(MCPT_ERR_OOM, "mcpt_scene_create: host allocation failed");
    sc->device = device;
    hipError_t e = hipSuccess;
    sc->knobs.read();
    // One pool by default: two pools measured +1..2 % at equal total size (2772 vs 2748 Msamples/s), within noise.
    sc->n_pools = sc->knobs.pools;
    for (int q = 0; q < sc->n_pools && e == hipSuccess; ++q) {
        PoolCtx &c = sc->pools[q];
        if (q > 0) e = c.main.create();
        if (sc->knobs.overlap) {
            for (int k = 0; k < 2 && e == hipSuccess; ++k) {
                e = c.side[k].create();
                if (e == hipSuccess) e = c.join[k].create();
            }
            if (e == hipSuccess) e = c.book.create();
            if (e == hipSuccess) e = c.shaded.create();
        }
    }
    for (int q = 0; q < sc->n_pools && e == hipSuccess; ++q) e = sc->pools[q].readback.create();
    if (e == hipSuccess) e = sc->fork.create();
    // the creation-time description stays with the scene: mcpt_scene_update starts from it every time
    SceneSource &S = sc->src;
    S.choice = choice;
    S.triangles.assign(desc->triangles, desc->triangles + (desc->triangles ? desc->n_triangles : 0));
    S.objects.assign(desc->objects, desc->objects + desc->n_objects);
    S.materials.assign(desc->materials, desc->materials + desc->n_materials);
    S.moved.assign((size_t)desc->n_objects, 0);
    S.xf.assign((size_t)desc->n_objects * 12, 0.f);
    S.visible.assign((size_t)desc->n_objects, 1);
    S.env = hs.env;
    if (e == hipSuccess) e = upload(sc->mats, hs.materials);
    if (e == hipSuccess) e = upload(sc->env, hs.env);
    if (e == hipSuccess && !hs.instances.empty()) e = upload(sc->inst, hs.instances);
    if (e == hipSuccess && hs.builder >= 2) {  // the device builders read the caller's triangles; they stay resident for the device path of an update
        e = upload(sc->tris0, desc->triangles, (size_t)hs.n_triangles);
        if (e == hipSuccess) e = upload(sc->sphere_obj, hs.sphere_objects);
    }
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? MCPT_ERR_OOM : MCPT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    SceneMeta meta = meta_of(hs);
    double gpu_build_ms = 0.0;
    const int rc = upload_geometry(hs, choice, sc->tris0.p, sc->sphere_obj.p, sc->geom, meta, gpu_build_ms);
    if (rc != MCPT_OK) return rc;
    sc->meta = meta;
#if defined(MCPT_TRAVERSAL_STATS) || defined(MCPT_CHECK_DIRECT_SKIP)
    if (sc->dbg.alloc(36) == hipSuccess) {  // (16 reported by mcpt_debug_counters; the statistics build prints the rest at destruction)
        (void)hipMemset(sc->dbg.p, 0, 36 * sizeof(unsigned long long));
    } else {
        sc->dbg.release();
    }
#endif
    fill_view(sc.get());
    sc->info.build_ms = hb.build_ms + gpu_build_ms;
    sc->info.init_ms = hb.init_ms;
    sc->info.upload_ms = ms_since(t_upload) - gpu_build_ms;
    *out = sc.release();
    return MCPT_OK;
}

int mcpt::check_moves(const mcpt_scene *sc, int32_t n, const mcpt_object_transform *moves, std::vector<uint8_t> &moved, std::vector<float> &xf,
                      std::vector<int32_t> &touched) {
    if (n < 0) return fail(MCPT_ERR_ARG, "mcpt_scene_update: n < 0");
    if (n > 0 && !moves) return fail(MCPT_ERR_ARG, "mcpt_scene_update: null moves");
    for (int32_t i = 0; i < n; ++i)
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(moves[i].m[k])) return fail(MCPT_ERR_ARG, "mcpt_scene_update: move " + std::to_string(i) + ": a matrix entry is not finite");
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < i; ++j)
            if (moves[i].object == moves[j].object) return fail(MCPT_ERR_ARG, "mcpt_scene_update: object " + std::to_string(moves[i].object) + " is listed twice");
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_update: null scene");
    const SceneSource &S = sc->src;
    for (int32_t i = 0; i < n; ++i)
        if (moves[i].object < 0 || moves[i].object >= (int32_t)S.objects.size())
            return fail(MCPT_ERR_ARG, "mcpt_scene_update: object index " + std::to_string(moves[i].object) + " out of range");
    if (S.choice.builder == MCPT_BUILD_SAH && S.choice.instancing == 1)
        return fail(MCPT_ERR_ARG, "mcpt_scene_update: the scene was built with node instancing on (instanced subtrees are shared between objects)");
    moved = S.moved;
    xf = S.xf;
    touched.clear();
    for (int32_t i = 0; i < n; ++i) {
        const int32_t o = moves[i].object;
        moved[(size_t)o] = 1;
        std::memcpy(&xf[(size_t)o * 12], moves[i].m, 12 * sizeof(float));
        touched.push_back(o);
    }
    return MCPT_OK;
}

namespace {

// The nine position floats of every triangle of the listed meshes on the host, item by item: the caller's own arrays, or downloads of
// the arrays given by device pointer (kept in `owned`).  The scene's device must be current.
int host_positions(const SceneSource &S, int32_t n, const mcpt_object_vertices *items, std::vector<std::vector<float>> &owned, std::vector<const float *> &pos) {
    owned.assign((size_t)n, {});
    pos.assign((size_t)n, nullptr);
    for (int32_t i = 0; i < n; ++i) {
        pos[(size_t)i] = items[i].positions;
        const size_t nf = (size_t)S.objects[(size_t)items[i].object].n_tri * 9;
        if (!items[i].on_device || nf == 0) continue;
        owned[(size_t)i].resize(nf);
        HIP_TRY(hipMemcpy(owned[(size_t)i].data(), items[i].positions, nf * sizeof(float), hipMemcpyDeviceToHost));
        pos[(size_t)i] = owned[(size_t)i].data();
    }
    return MCPT_OK;
}

// desc' from the base description: the objects that have a transform get it applied, meshes to their triangles, spheres to their centre.
void apply_current_transforms(std::vector<mcpt_object> &objs, std::vector<mcpt_triangle> &tris, const std::vector<uint8_t> &moved, const std::vector<float> &xf) {
    for (size_t o = 0; o < objs.size(); ++o) {
        if (!moved[o]) continue;
        const float *m = &xf[o * 12];
        if (objs[o].kind == MCPT_OBJ_MESH) {
            for (int32_t k = 0; k < objs[o].n_tri; ++k) mv::move_triangle(m, tris[(size_t)objs[o].first_tri + k], tris[(size_t)objs[o].first_tri + k]);
        } else {
            const mv::V3 c = mv::move_point(m, mv::ld(objs[o].center));
            objs[o].center[0] = c.x;
            objs[o].center[1] = c.y;
            objs[o].center[2] = c.z;
        }
    }
}

// The host path every edit ends in: desc' (objs, tris, mats) is flattened and its tree built as at creation, with the mask `visible`;
// every array that depends on the geometry is copied into g2 (device builders: the moved triangles too, and the tree is built there
// over the spheres listed in d_sphere_obj); `meta` becomes that of the new arrays.  The caller swaps.
struct HostPathTimes {
    double host_build_ms = 0.0, gpu_build_ms = 0.0;
    Clock::time_point upload_start;
};
int flatten_and_upload(mcpt_scene *sc, const std::vector<mcpt_object> &objs, const std::vector<mcpt_triangle> &tris, const std::vector<mcpt_material> &mats,
                       const std::vector<uint8_t> &visible, const int32_t *d_sphere_obj, const char *who, HostScene &hs, GeomBufs &g2, SceneMeta &meta,
                       HostPathTimes &T) {
    const SceneSource &S = sc->src;
    const auto tb = Clock::now();
    mcpt_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_objects = (int32_t)objs.size();
    d.n_triangles = (int32_t)tris.size();
    d.n_materials = (int32_t)mats.size();
    for (int k = 0; k < 3; ++k) d.background[k] = meta.background[k];
    d.objects = objs.data();
    d.triangles = tris.data();
    d.materials = mats.data();
    const char *err = "";
    const bool masked = std::find(visible.begin(), visible.end(), (uint8_t)0) != visible.end();
    int rc = build_host_scene(d, hs, &err, S.choice, masked ? visible.data() : nullptr);
    if (rc != MCPT_OK) return fail(rc, std::string(who) + err);
    T.host_build_ms = ms_since(tb);
    T.upload_start = Clock::now();
    const int32_t env_w = meta.env_w, env_h = meta.env_h;  // (the environment map is not part of desc': it stays where it is)
    meta = meta_of(hs);
    meta.env_w = env_w;
    meta.env_h = env_h;
    DevVis dv;
    if (hs.builder >= 2) {
        HIP_TRY(upload(g2.tris, tris));
        rc = upload_vis(S, visible, dv);
        if (rc != MCPT_OK) return rc;
    }
    return upload_geometry(hs, S.choice, g2.tris.p, d_sphere_obj, g2, meta, T.gpu_build_ms, &dv);
}

// The rebuild behind mcpt_scene_update and mcpt_scene_deform: the scene gets the transform table (moved, xf) and, when `deform` is given,
// the listed meshes (touched[i] = deform[i].object) get new base positions.  Everything is built aside and committed on success.
// `edit` (mcpt_scene_set_materials, path 0): the material table and the objects' material indices of the plan replace the scene's; the
// host path is taken whatever the builder, and the new material table is uploaded aside with the rest.
// `show` (mcpt_scene_set_visibility): the mask the scene gets, `touched` being the objects whose state changes; the other edits rebuild
// with the mask the scene has.  Either way hidden objects keep current records and stay out of the tree and the light tables.  A
// change of visibility alone moves nothing: on the device path only the tree is built again, from the arrays that are live.
int rebuild(mcpt_scene *sc, const std::vector<uint8_t> &moved, const std::vector<float> &xf, const std::vector<int32_t> &touched,
            const mcpt_object_vertices *deform, mcpt_update_info *info, const mat::EditPlan *edit = nullptr, const std::vector<uint8_t> *show = nullptr) {
    const auto t0 = Clock::now();
    mcpt_update_info ui;
    std::memset(&ui, 0, sizeof ui);
    SceneSource &S = sc->src;
    bool emitter = false;
    for (int32_t o : touched) {
        const mcpt_object &ob = S.objects[(size_t)o];
        if (ob.kind == MCPT_OBJ_MESH) ui.n_moved_tris += ob.n_tri;
        emitter = emitter || emits(S.materials[(size_t)ob.material]);
    }
    if (edit) ui.n_moved_tris = edit->n_tris;
    if (touched.empty() && !edit) {
        if (info) *info = ui;
        return MCPT_OK;
    }
    HIP_TRY(hipSetDevice(sc->device));
    HIP_TRY(query_settle(sc));  // a ray query still in flight reads the arrays this call swaps and frees
    GeomBufs g2;  // built aside; swapped in once the new tree is known to be usable
    SceneMeta meta = sc->meta;
    const size_t nt = (size_t)meta.n_triangles;
    const int32_t n_def = deform ? (int32_t)touched.size() : 0;
    DevBuf<mcpt_triangle> base2;              // deformation, device builders: the new base triangles, swapped with tris0 on success
    std::vector<mcpt_triangle> base;          // deformation: the new host copy of the base, swapped with S.triangles on success
    std::vector<std::vector<float>> fetched;  // deformation: positions downloaded from device pointers
    std::vector<const float *> pos;
    DevBuf<MaterialRec> mats2;  // material edit: the new table, swapped with sc->mats on success
    const std::vector<uint8_t> &visible = show ? *show : S.visible;
    DevVis dv;
    if (show && meta.builder >= 2 && !emitter) {
        // ---- device path of a change of visibility: the tables of the visible ranges cross the bus, the device builder runs on the live
        // triangles and sphere records, and the node arrays alone are exchanged
        ui.path = 1;
        const auto tt = Clock::now();
        int rc = upload_vis(S, visible, dv);
        if (rc != MCPT_OK) return rc;
        ui.transform_ms = ms_since(tt);
        const auto tb = Clock::now();
        rc = build_device_tree_checked(sc->geom.tris.p ? sc->geom.tris.p : sc->tris0.p, sc->sphere_obj.p, (int)sc->sphere_obj.n, S.choice, g2, meta, &dv, sc->geom.spheres.p);
        if (rc != MCPT_OK) return rc;
        ui.build_ms = ms_since(tb);
        sc->geom.swap_nodes(g2);
    } else if (meta.builder >= 2 && !emitter && !edit) {
        // ---- device path: the listed triangles and sphere centres are moved in HBM, the device builder runs again
        ui.path = 1;
        const auto tu = Clock::now();
        HIP_TRY(g2.tri_geom.alloc(nt));
        HIP_TRY(g2.tri_shade.alloc(nt));
        HIP_TRY(g2.tris.alloc(nt));
        HIP_TRY(g2.spheres.alloc(sc->geom.spheres.n));
        if (nt) {
            HIP_TRY(hipMemcpyAsync(g2.tri_geom.p, sc->geom.tri_geom.p, nt * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(g2.tri_shade.p, sc->geom.tri_shade.p, nt * sizeof(TriShade), hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(g2.tris.p, sc->geom.tris.p ? sc->geom.tris.p : sc->tris0.p, nt * sizeof(mcpt_triangle), hipMemcpyDeviceToDevice, nullptr));
        }
        if (sc->geom.spheres.n)
            HIP_TRY(hipMemcpyAsync(g2.spheres.p, sc->geom.spheres.p, sc->geom.spheres.bytes(), hipMemcpyDeviceToDevice, nullptr));
        if (deform) {
            HIP_TRY(base2.alloc(nt));
            if (nt) HIP_TRY(hipMemcpyAsync(base2.p, sc->tris0.p, nt * sizeof(mcpt_triangle), hipMemcpyDeviceToDevice, nullptr));
        }
        HIP_TRY(hipStreamSynchronize(nullptr));
        ui.upload_ms = ms_since(tu);
        const auto tt = Clock::now();
        int32_t lanes = 0;
        if (deform) {
            // host positions go through the staging buffer in one copy; device positions are read where they are
            std::vector<float> staged;
            std::vector<size_t> at((size_t)n_def, 0);
            for (int32_t i = 0; i < n_def; ++i) {
                if (deform[i].on_device) continue;
                at[(size_t)i] = staged.size();
                staged.insert(staged.end(), deform[i].positions, deform[i].positions + (size_t)S.objects[(size_t)touched[(size_t)i]].n_tri * 9);
            }
            HIP_TRY(upload(sc->stage, staged));
            std::vector<DeformSeg> dsegs;
            for (int32_t i = 0; i < n_def; ++i) {
                const int32_t o = touched[(size_t)i];
                const mcpt_object &ob = S.objects[(size_t)o];
                if (ob.n_tri <= 0) continue;
                DeformSeg sg;
                std::memset(&sg, 0, sizeof sg);
                sg.first_lane = lanes;
                sg.first_tri = ob.first_tri;
                sg.object = o;
                sg.raw = moved[(size_t)o] ? 0 : 1;
                std::memcpy(sg.m, &xf[(size_t)o * 12], sizeof sg.m);
                sg.positions = deform[i].on_device ? deform[i].positions : sc->stage.p + at[(size_t)i];
                lanes += ob.n_tri;
                dsegs.push_back(sg);
            }
            HIP_TRY(upload(sc->dsegs, dsegs));
            HIP_TRY(sc->dflag.alloc(1));
            HIP_TRY(hipMemsetAsync(sc->dflag.p, 0, sizeof(uint32_t), nullptr));
            launch_deform_objects(sc->dsegs.p, (int32_t)dsegs.size(), lanes, sc->tris0.p, base2.p, g2.tris.p, g2.tri_geom.p, g2.tri_shade.p, sc->dflag.p, nullptr);
            HIP_TRY(hipGetLastError());
            uint32_t flag = 0;  // (a blocking copy on the null stream: the kernel has finished when it returns)
            HIP_TRY(download(&flag, sc->dflag, 1));
            if (flag) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: a position given by device pointer is not finite");
        } else {
            std::vector<MoveSeg> segs;
            for (int32_t o : touched) {
                const mcpt_object &ob = S.objects[(size_t)o];
                MoveSeg sg;
                std::memset(&sg, 0, sizeof sg);
                sg.first_lane = lanes;
                sg.count = ob.kind == MCPT_OBJ_MESH ? ob.n_tri : 1;
                sg.first_tri = ob.kind == MCPT_OBJ_MESH ? ob.first_tri : -1;
                sg.object = o;
                std::memcpy(sg.m, &xf[(size_t)o * 12], sizeof sg.m);
                for (int k = 0; k < 3; ++k) sg.c0[k] = ob.center[k];
                sg.raw = moved[(size_t)o] ? 0 : 1;
                lanes += sg.count;
                segs.push_back(sg);
            }
            HIP_TRY(upload(sc->segs, segs));
            launch_move_objects(sc->segs.p, (int32_t)segs.size(), lanes, sc->tris0.p, g2.tris.p, g2.tri_geom.p, g2.tri_shade.p, g2.spheres.p, nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(nullptr));
        }
        int rc = upload_vis(S, visible, dv);
        if (rc != MCPT_OK) return rc;
        ui.transform_ms = ms_since(tt);
        const auto tb = Clock::now();
        rc = build_device_tree_checked(g2.tris.p, sc->sphere_obj.p, (int)sc->sphere_obj.n, S.choice, g2, meta, &dv);
        if (rc != MCPT_OK) return rc;
        ui.build_ms = ms_since(tb);
        if (deform) {  // the host copy of the base follows at once (36 B per triangle come back for positions given by device pointer)
            rc = host_positions(S, n_def, deform, fetched, pos);
            if (rc != MCPT_OK) return rc;
        }
        sc->geom.swap_prims(g2);
    } else {
        // ---- host path: desc' is flattened and its tree built as at creation; every array that depends on the geometry is copied again
        ui.path = 0;
        const auto tt = Clock::now();
        if (deform) {  // positions given by device pointer are downloaded first, and checked here
            const int rc = host_positions(S, n_def, deform, fetched, pos);
            if (rc != MCPT_OK) return rc;
            for (int32_t i = 0; i < n_def; ++i) {
                if (!deform[i].on_device) continue;
                for (int32_t k = 0; k < S.objects[(size_t)touched[(size_t)i]].n_tri; ++k)
                    if (!mv::positions_finite(pos[(size_t)i] + (size_t)k * 9))
                        return fail(MCPT_ERR_ARG, "mcpt_scene_deform: a position given by device pointer is not finite");
            }
        }
        std::vector<mcpt_triangle> tris = S.triangles;
        for (int32_t i = 0; i < n_def; ++i) {
            const mcpt_object &ob = S.objects[(size_t)touched[(size_t)i]];
            for (int32_t k = 0; k < ob.n_tri; ++k) mv::deform_triangle(pos[(size_t)i] + (size_t)k * 9, tris[(size_t)ob.first_tri + k], tris[(size_t)ob.first_tri + k]);
        }
        if (deform) base = tris;
        std::vector<mcpt_object> objs = edit ? edit->objects : S.objects;
        const std::vector<mcpt_material> &mats = edit ? edit->materials : S.materials;
        apply_current_transforms(objs, tris, moved, xf);
        ui.transform_ms = ms_since(tt);
        HostScene hs;
        HostPathTimes T;
        const int rc = flatten_and_upload(sc, objs, tris, mats, visible, sc->sphere_obj.p,
                                          show ? "mcpt_scene_set_visibility: " : (edit ? "mcpt_scene_set_materials: " : (deform ? "mcpt_scene_deform: " : "mcpt_scene_update: ")),
                                          hs, g2, meta, T);
        if (rc != MCPT_OK) return rc;
        ui.build_ms = T.host_build_ms + T.gpu_build_ms;
        if (deform && hs.builder >= 2) HIP_TRY(upload(base2, base));
        if (edit) HIP_TRY(upload(mats2, hs.materials));
        ui.upload_ms = ms_since(T.upload_start) - T.gpu_build_ms;
        sc->geom.swap_prims(g2);
        sc->geom.swap_lights(g2);
    }
    if (deform) {  // the new base: on the device (device builders) and on the host
        if (meta.builder >= 2) sc->tris0.swap(base2);
        if (ui.path == 1) {  // (the host copy is patched in place)
            for (int32_t i = 0; i < n_def; ++i) {
                const mcpt_object &ob = S.objects[(size_t)touched[(size_t)i]];
                for (int32_t k = 0; k < ob.n_tri; ++k)
                    mv::deform_triangle(pos[(size_t)i] + (size_t)k * 9, S.triangles[(size_t)ob.first_tri + k], S.triangles[(size_t)ob.first_tri + k]);
            }
        } else {
            S.triangles.swap(base);
        }
    }
    if (edit) {  // the material table on the device and the host copy of the description
        sc->mats.swap(mats2);
        S.materials = edit->materials;
        S.objects = edit->objects;
    }
    sc->meta = meta;
    S.moved = moved;
    S.xf = xf;
    if (show) S.visible = *show;
    fill_view(sc);
    ui.total_ms = ms_since(t0);
    if (info) *info = ui;
    return MCPT_OK;
}

}  // namespace

int mcpt::apply_transforms(mcpt_scene *sc, const std::vector<uint8_t> &moved, const std::vector<float> &xf, const std::vector<int32_t> &touched,
                           mcpt_update_info *info) {
    return rebuild(sc, moved, xf, touched, nullptr, info);
}

int mcpt::check_deform(const mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items) {
    if (n < 0) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: n < 0");
    if (n > 0 && !items) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: null items");
    for (int32_t i = 0; i < n; ++i) {
        if (!items[i].positions) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: item " + std::to_string(i) + ": null positions");
        if (items[i].on_device != 0 && items[i].on_device != 1) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: item " + std::to_string(i) + ": on_device is not 0 or 1");
    }
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < i; ++j)
            if (items[i].object == items[j].object) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: object " + std::to_string(items[i].object) + " is listed twice");
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: null scene");
    const SceneSource &S = sc->src;
    for (int32_t i = 0; i < n; ++i) {
        if (items[i].object < 0 || items[i].object >= (int32_t)S.objects.size())
            return fail(MCPT_ERR_ARG, "mcpt_scene_deform: object index " + std::to_string(items[i].object) + " out of range");
        if (S.objects[(size_t)items[i].object].kind != MCPT_OBJ_MESH)
            return fail(MCPT_ERR_ARG, "mcpt_scene_deform: object " + std::to_string(items[i].object) + " is a sphere");
    }
    if (S.choice.builder == MCPT_BUILD_SAH && S.choice.instancing == 1)
        return fail(MCPT_ERR_ARG, "mcpt_scene_deform: the scene was built with node instancing on (instanced subtrees are shared between objects)");
    for (int32_t i = 0; i < n; ++i) {
        if (items[i].on_device) continue;
        for (int32_t k = 0; k < S.objects[(size_t)items[i].object].n_tri; ++k)
            if (!mv::positions_finite(items[i].positions + (size_t)k * 9))
                return fail(MCPT_ERR_ARG, "mcpt_scene_deform: item " + std::to_string(i) + ": a position is not finite");
    }
    return MCPT_OK;
}

int mcpt::apply_deform(mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items, mcpt_update_info *info) {
    std::vector<int32_t> touched;
    for (int32_t i = 0; i < n; ++i) touched.push_back(items[i].object);
    return rebuild(sc, sc->src.moved, sc->src.xf, touched, n > 0 ? items : nullptr, info);
}

int mcpt::check_visibility(const mcpt_scene *sc, int32_t n, const mcpt_object_visibility *items, std::vector<uint8_t> &visible, std::vector<int32_t> &changed) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: null scene");
    if (n < 0) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: n < 0");
    if (n > 0 && !items) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: null items");
    const SceneSource &S = sc->src;
    visible = S.visible;
    changed.clear();
    std::vector<uint8_t> listed(S.objects.size(), 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t o = items[i].object;
        if (o < 0 || o >= (int32_t)S.objects.size()) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: object index " + std::to_string(o) + " out of range");
        if (listed[(size_t)o]) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: object " + std::to_string(o) + " is listed twice");
        if (items[i].visible != 0 && items[i].visible != 1) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: item " + std::to_string(i) + ": visible is not 0 or 1");
        listed[(size_t)o] = 1;
        visible[(size_t)o] = (uint8_t)items[i].visible;
    }
    if (S.choice.builder == MCPT_BUILD_SAH && S.choice.instancing == 1)
        return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: the scene was built with node instancing on (instanced subtrees are shared between objects)");
    for (size_t o = 0; o < visible.size(); ++o)
        if (visible[o] != S.visible[o]) changed.push_back((int32_t)o);
    if (changed.empty()) return MCPT_OK;
    const int32_t n_prims = count_visible_prims(S, visible);
    if (n_prims == 0) return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: no object would be visible (a scene cannot be empty)");
    if (sc->meta.builder >= 2 && n_prims < 2)  // (build_lbvh_device needs two primitives; creation falls back to the host builder, a live scene keeps its builder)
        return fail(MCPT_ERR_ARG, "mcpt_scene_set_visibility: a device-built scene needs at least two visible primitives");
    return MCPT_OK;
}

int mcpt::apply_visibility(mcpt_scene *sc, const std::vector<uint8_t> &visible, const std::vector<int32_t> &changed, mcpt_update_info *info) {
    return rebuild(sc, sc->src.moved, sc->src.xf, changed, nullptr, info, nullptr, &visible);
}

int mcpt::check_add(const mcpt_scene *sc, const mcpt_scene_addition *add) {
    if (!sc || !add) return fail(MCPT_ERR_ARG, "mcpt_scene_add_objects: null argument");
    const SceneSource &S = sc->src;
    const char *err = "";
    const int rc = check_scene_addition((int32_t)S.objects.size(), (int32_t)S.triangles.size(), (int32_t)S.materials.size(), *add, &err);
    if (rc != MCPT_OK) return fail(rc, std::string("mcpt_scene_add_objects: ") + err);
    if (S.choice.builder == MCPT_BUILD_SAH && S.choice.instancing == 1)
        return fail(MCPT_ERR_ARG, "mcpt_scene_add_objects: the scene was built with node instancing on (instanced subtrees are shared between objects)");
    return MCPT_OK;
}

namespace {

// Exchanges everything mcpt_scene_add_objects replaces between the scene and `A`: the commit of apply_add, and its way back.
void exchange_add(mcpt_scene *sc, AddAside &A) {
    sc->geom.swap_prims(A.geom);
    if (A.lights) sc->geom.swap_lights(A.geom);
    sc->tris0.swap(A.tris0);
    sc->sphere_obj.swap(A.sphere_obj);
    sc->mats.swap(A.mats);
    if (sc->has_snapshot) {
        sc->snap_tri.swap(A.snap_tri);
        sc->snap_sph.swap(A.snap_sph);
    }
    std::swap(sc->meta, A.meta);
}

void resize_source(SceneSource &S, size_t n_objects, size_t n_triangles, size_t n_materials) {
    S.objects.resize(n_objects);
    S.triangles.resize(n_triangles);
    S.materials.resize(n_materials);
    S.moved.resize(n_objects, 0);
    S.xf.resize(n_objects * 12, 0.f);
    S.visible.resize(n_objects, 1);
}

}  // namespace

// The scene's own description is extended in place first (mcpt_extend_scene's rule) and cut back if anything below fails; every device
// array that is indexed by primitive or by object is built aside at the new size in `A` and exchanged with the scene's as the last step.
int mcpt::apply_add(mcpt_scene *sc, const mcpt_scene_addition *add, int32_t *first_object, mcpt_update_info *info, AddAside *keep) {
    const auto t0 = Clock::now();
    mcpt_update_info ui;
    std::memset(&ui, 0, sizeof ui);
    ui.n_moved_tris = add->n_triangles;
    SceneSource &S = sc->src;
    HIP_TRY(hipSetDevice(sc->device));
    HIP_TRY(query_settle(sc, true));
    AddAside local;
    AddAside &A = keep ? *keep : local;
    const size_t no = S.objects.size(), nt = S.triangles.size(), nm = S.materials.size();
    const size_t no2 = no + (size_t)add->n_objects, nt2 = nt + (size_t)add->n_triangles;
    A.n_objects = no;
    A.n_triangles = nt;
    A.n_materials = nm;
    struct CutBack {  // a failed call leaves the description as it was
        SceneSource &S;
        size_t no, nt, nm;
        bool keep = false;
        ~CutBack() {
            if (!keep) resize_source(S, no, nt, nm);
        }
    } cut{S, no, nt, nm};
    resize_source(S, no2, nt2, nm + (size_t)add->n_materials);
    for (int32_t i = 0; i < add->n_objects; ++i) {
        mcpt_object &o = S.objects[no + (size_t)i];
        o = add->objects[i];
        if (o.kind == MCPT_OBJ_MESH) o.first_tri += (int32_t)nt;
    }
    std::copy(add->triangles, add->triangles + add->n_triangles, S.triangles.begin() + (ptrdiff_t)nt);
    std::copy(add->materials, add->materials + add->n_materials, S.materials.begin() + (ptrdiff_t)nm);
    bool emitter = false;
    for (size_t o = no; o < no2; ++o) emitter = emitter || emits(S.materials[(size_t)S.objects[o].material]);
    std::vector<int32_t> sph;  // the device builders' sphere list at the new size
    for (size_t o = 0; o < no2; ++o)
        if (S.objects[o].kind == MCPT_OBJ_SPHERE) sph.push_back((int32_t)o);
    SceneMeta meta = sc->meta;
    GeomBufs &g2 = A.geom;
    if (meta.builder >= 2 && !emitter) {
        // ---- device path: the live records are copied into arrays of the new size, a kernel writes the records of the added primitives
        // from their triangles, the device builder runs at the new size
        ui.path = 1;
        const auto tu = Clock::now();
        HIP_TRY(g2.tri_geom.alloc(nt2));
        HIP_TRY(g2.tri_shade.alloc(nt2));
        HIP_TRY(g2.tris.alloc(nt2));
        HIP_TRY(g2.spheres.alloc(no2));
        HIP_TRY(A.tris0.alloc(nt2));
        HIP_TRY(A.sphere_obj.alloc(sph.size()));
        if (nt) {
            HIP_TRY(hipMemcpyAsync(g2.tri_geom.p, sc->geom.tri_geom.p, nt * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(g2.tri_shade.p, sc->geom.tri_shade.p, nt * sizeof(TriShade), hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(g2.tris.p, sc->geom.tris.p ? sc->geom.tris.p : sc->tris0.p, nt * sizeof(mcpt_triangle), hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(A.tris0.p, sc->tris0.p, nt * sizeof(mcpt_triangle), hipMemcpyDeviceToDevice, nullptr));
        }
        HIP_TRY(hipMemcpyAsync(g2.spheres.p, sc->geom.spheres.p, no * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(g2.spheres.p + no, 0, (no2 - no) * sizeof(SphereRec), nullptr));  // (the slots of meshes stay zero, as the host leaves them)
        HIP_TRY(hipStreamSynchronize(nullptr));
        ui.upload_ms = ms_since(tu);
        const auto tt = Clock::now();
        if (add->n_triangles) HIP_TRY(hipMemcpy(A.tris0.p + nt, add->triangles, (size_t)add->n_triangles * sizeof(mcpt_triangle), hipMemcpyHostToDevice));
        if (!sph.empty()) HIP_TRY(hipMemcpy(A.sphere_obj.p, sph.data(), sph.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        std::vector<MaterialRec> recs(S.materials.size());
        for (size_t i = 0; i < recs.size(); ++i) mat::make_record(S.materials[i], recs[i]);
        HIP_TRY(upload(A.mats, recs));
        std::vector<AddSeg> segs;
        int32_t lanes = 0;
        for (size_t o = no; o < no2; ++o) {
            const mcpt_object &ob = S.objects[o];
            const mcpt_material &m = S.materials[(size_t)ob.material];
            const bool mesh = ob.kind == MCPT_OBJ_MESH;
            AddSeg sg;
            std::memset(&sg, 0, sizeof sg);
            sg.first_lane = lanes;
            sg.count = mesh ? ob.n_tri : 1;
            sg.first_tri = mesh ? ob.first_tri : -1;
            sg.object = (int32_t)o;
            sg.mat_bits = mesh ? mat::tri_mat_bits(ob.material, m) : mat::sphere_mat_bits(ob.material, m);
            sg.mat = ob.material;
            sg.radius = ob.radius;
            for (int k = 0; k < 3; ++k) sg.c[k] = ob.center[k];
            lanes += sg.count;
            segs.push_back(sg);
        }
        HIP_TRY(upload(sc->asegs, segs));
        launch_add_objects(sc->asegs.p, (int32_t)segs.size(), lanes, A.tris0.p, g2.tris.p, g2.tri_geom.p, g2.tri_shade.p, g2.spheres.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(nullptr));
        DevVis dv;
        int rc = upload_vis(S, S.visible, dv);
        if (rc != MCPT_OK) return rc;
        ui.transform_ms = ms_since(tt);
        const auto tb = Clock::now();
        meta.n_triangles = (int32_t)nt2;
        meta.n_objects = (int32_t)no2;
        meta.n_sphere_slots = (int32_t)no2;
        meta.n_mats = (int32_t)S.materials.size();
        rc = build_device_tree_checked(g2.tris.p, A.sphere_obj.p, (int)sph.size(), S.choice, g2, meta, &dv);
        if (rc != MCPT_OK) return rc;
        ui.build_ms = ms_since(tb);
    } else {
        // ---- host path: the extended desc' is flattened and uploaded by the creation code
        ui.path = 0;
        A.lights = true;
        const auto tt = Clock::now();
        std::vector<mcpt_triangle> tris = S.triangles;
        std::vector<mcpt_object> objs = S.objects;
        apply_current_transforms(objs, tris, S.moved, S.xf);
        ui.transform_ms = ms_since(tt);
        if (meta.builder >= 2) HIP_TRY(upload(A.sphere_obj, sph));
        HostScene hs;
        HostPathTimes T;
        const int rc = flatten_and_upload(sc, objs, tris, S.materials, S.visible, A.sphere_obj.p, "mcpt_scene_add_objects: ", hs, g2, meta, T);
        if (rc != MCPT_OK) return rc;
        ui.build_ms = T.host_build_ms + T.gpu_build_ms;
        if (hs.builder >= 2) HIP_TRY(upload(A.tris0, S.triangles));
        HIP_TRY(upload(A.mats, hs.materials));
        ui.upload_ms = ms_since(T.upload_start) - T.gpu_build_ms;
    }
    if (sc->has_snapshot) {  // the snapshot at the new size: what it held, then the added objects' records as added
        HIP_TRY(A.snap_tri.alloc(nt2));
        HIP_TRY(A.snap_sph.alloc(no2));
        if (nt) HIP_TRY(hipMemcpyAsync(A.snap_tri.p, sc->snap_tri.p, nt * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
        if (nt2 > nt) HIP_TRY(hipMemcpyAsync(A.snap_tri.p + nt, g2.tri_geom.p + nt, (nt2 - nt) * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(A.snap_sph.p, sc->snap_sph.p, no * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(A.snap_sph.p + no, g2.spheres.p + no, (no2 - no) * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    A.meta = meta;
    exchange_add(sc, A);
    cut.keep = true;
    fill_view(sc);
    ui.total_ms = ms_since(t0);
    if (first_object) *first_object = (int32_t)no;
    if (info) *info = ui;
    return MCPT_OK;
}

int mcpt::undo_add(mcpt_scene *sc, AddAside &A) {
    HIP_TRY(hipSetDevice(sc->device));
    HIP_TRY(query_settle(sc, true));
    exchange_add(sc, A);
    resize_source(sc->src, A.n_objects, A.n_triangles, A.n_materials);
    fill_view(sc);
    return MCPT_OK;
}

int mcpt::check_material_edit(const mcpt_scene *sc, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign, const mcpt_object_material *assign,
                              mat::EditPlan &plan) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_set_materials: null scene");
    const SceneSource &S = sc->src;
    std::string err;
    const int rc = mat::plan_edit(S.materials, S.objects, n_edits, edits, n_assign, assign, plan, err);
    if (rc != MCPT_OK) return fail(rc, "mcpt_scene_set_materials: " + err);
    if (S.choice.builder == MCPT_BUILD_SAH && S.choice.instancing == 1)
        return fail(MCPT_ERR_ARG, "mcpt_scene_set_materials: the scene was built with node instancing on (instanced groups were formed from non-emitting meshes)");
    return MCPT_OK;
}

int mcpt::apply_material_edit(mcpt_scene *sc, const mat::EditPlan &plan, mcpt_update_info *info) {
    SceneSource &S = sc->src;
    if (!plan.in_place)  // some object starts or stops emitting: the creation code forms the light tables again
        return rebuild(sc, S.moved, S.xf, {}, nullptr, info, &plan);
    const auto t0 = Clock::now();
    mcpt_update_info ui;
    std::memset(&ui, 0, sizeof ui);
    ui.path = 2;
    ui.n_moved_tris = plan.n_tris;
    if (plan.mat_hi > plan.mat_lo || plan.n_lanes > 0 || !plan.lights.empty()) {
        HIP_TRY(hipSetDevice(sc->device));
        // the segment table first: after it nothing allocates, so only a failing copy or launch can leave the call half done
        if (plan.n_lanes > 0) HIP_TRY(upload(sc->msegs, plan.segs));
        if (plan.mat_hi > plan.mat_lo) {  // one copy of the span of the table that holds the listed entries
            std::vector<MaterialRec> recs((size_t)(plan.mat_hi - plan.mat_lo));
            for (int32_t i = plan.mat_lo; i < plan.mat_hi; ++i) mat::make_record(plan.materials[(size_t)i], recs[(size_t)(i - plan.mat_lo)]);
            HIP_TRY(hipMemcpy(sc->mats.p + plan.mat_lo, recs.data(), recs.size() * sizeof(MaterialRec), hipMemcpyHostToDevice));
        }
        for (const mat::EditPlan::LightMat &l : plan.lights)
            HIP_TRY(hipMemcpy(&sc->geom.lights.p[l.light].mat, &l.mat, sizeof(int32_t), hipMemcpyHostToDevice));
        if (plan.n_lanes > 0) {
            launch_set_materials(sc->msegs.p, (int32_t)plan.segs.size(), plan.n_lanes, sc->geom.tri_geom.p, sc->geom.tri_shade.p, sc->geom.spheres.p, nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(nullptr));
        }
    }
    S.materials = plan.materials;
    S.objects = plan.objects;
    ui.transform_ms = ui.total_ms = ms_since(t0);
    if (info) *info = ui;
    return MCPT_OK;
}

int mcpt::check_environment(const mcpt_scene *sc, const float *background, int32_t env_w, int32_t env_h, const float *env_pixels) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_set_environment: null scene");
    if (!background) return fail(MCPT_ERR_ARG, "mcpt_scene_set_environment: null background");
    if (env_pixels ? !(env_w > 0 && env_h > 0) : !(env_w == 0 && env_h == 0))
        return fail(MCPT_ERR_ARG, "mcpt_scene_set_environment: env_w and env_h are both positive with a map and both zero without one");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(background[k])) return fail(MCPT_ERR_ARG, "mcpt_scene_set_environment: a background value is not finite");
    const size_t n = (size_t)env_w * (size_t)env_h * 3;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(env_pixels[i])) return fail(MCPT_ERR_ARG, "mcpt_scene_set_environment: a map value is not finite");
    return MCPT_OK;
}

int mcpt::apply_environment(mcpt_scene *sc, const float *background, int32_t env_w, int32_t env_h, const float *env_pixels, mcpt_update_info *info) {
    const auto t0 = Clock::now();
    mcpt_update_info ui;
    std::memset(&ui, 0, sizeof ui);
    ui.path = 2;
    HIP_TRY(hipSetDevice(sc->device));
    const size_t n = (size_t)env_w * (size_t)env_h * 3;
    std::vector<float> host(env_pixels, env_pixels + n);  // (first: the last thing that can fail is the upload)
    DevBuf<float> env2;  // aside; swapped in on success
    HIP_TRY(upload(env2, env_pixels, n));
    sc->env.swap(env2);
    sc->src.env.swap(host);
    for (int k = 0; k < 3; ++k) sc->meta.background[k] = background[k];
    sc->meta.env_w = env_w;
    sc->meta.env_h = env_h;
    fill_view(sc);
    ui.upload_ms = ui.total_ms = ms_since(t0);
    if (info) *info = ui;
    return MCPT_OK;
}

// The layout of mcpt_bvh_dump / mcpt_scene_dump_bvh: per node 12 floats {lmin, lmax, rmin, rmax}, two child references and (qn != nullptr) the
// twelve 16-bit grid coordinates of its quantised boxes.
static void export_nodes(int32_t n, const Node *nodes, const QNode *qn, float *boxes, int32_t *children, uint16_t *qboxes) {
    for (int32_t i = 0; i < n; ++i) {
        const Node &N = nodes[i];
        float *b = boxes + (size_t)i * 12;
        for (int k = 0; k < 3; ++k) {
            b[k] = N.lmin[k];
            b[3 + k] = N.lmax[k];
            b[6 + k] = N.rmin[k];
            b[9 + k] = N.rmax[k];
        }
        children[2 * i] = N.left;
        children[2 * i + 1] = N.right;
        if (!qn) continue;
        uint16_t *q = qboxes + (size_t)i * 12;
        for (int w = 0; w < 6; ++w) {
            q[2 * w] = (uint16_t)(qn[i].w[w] & 0xffffu);
            q[2 * w + 1] = (uint16_t)(qn[i].w[w] >> 16);
        }
    }
}

extern "C" {

const char *mcpt_last_error(void) { return g_err.c_str(); }
const char *mcpt_version(void) {
#if defined(MCPT_TEST_HOOKS) || defined(MCPT_CHECK_DIRECT_SKIP) || defined(MCPT_TRAVERSAL_STATS)
    return "mcpt-hip 0.2 (gfx950) checking build";
#else
    return "mcpt-hip 0.2 (gfx950)";
#endif
}

int mcpt_scene_create(const mcpt_scene_desc *desc, int device, mcpt_scene **out) { return mcpt_scene_create_ex(desc, device, nullptr, out); }

int mcpt_scene_create_ex(const mcpt_scene_desc *desc, int device, const mcpt_build_options *options, mcpt_scene **out) {
    if (!desc || !out) return fail(MCPT_ERR_ARG, "mcpt_scene_create: null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MCPT_ERR_HIP, "mcpt_scene_create: no HIP device available (this library has no CPU fallback)");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= ndev) return fail(MCPT_ERR_ARG, "mcpt_scene_create: device index out of range");
    double init_ms = 0.0;
    std::thread warm([&]() { init_ms = warm_up_device(device); });  // beside the host build
    HostBuild hb;
    const int rc = build_scene_host(desc, options, hb);
    warm.join();
    if (rc != MCPT_OK) return rc;
    hb.init_ms = init_ms;
    return upload_scene(desc, hb, device, out);
}

int mcpt_scene_update(mcpt_scene *sc, int32_t n, const mcpt_object_transform *moves, mcpt_update_info *info) {
    std::vector<uint8_t> moved;
    std::vector<float> xf;
    std::vector<int32_t> touched;
    const int rc = check_moves(sc, n, moves, moved, xf, touched);
    if (rc != MCPT_OK) return rc;
    return apply_transforms(sc, moved, xf, touched, info);
}

int mcpt_scene_deform(mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items, mcpt_update_info *info) {
    const int rc = check_deform(sc, n, items);
    if (rc != MCPT_OK) return rc;
    return apply_deform(sc, n, items, info);
}

int mcpt_scene_set_materials(mcpt_scene *sc, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign, const mcpt_object_material *assign,
                             mcpt_update_info *info) {
    mat::EditPlan plan;
    const int rc = check_material_edit(sc, n_edits, edits, n_assign, assign, plan);
    if (rc != MCPT_OK) return rc;
    return apply_material_edit(sc, plan, info);
}

int mcpt_scene_set_environment(mcpt_scene *sc, const float background[3], int32_t env_w, int32_t env_h, const float *env_pixels, mcpt_update_info *info) {
    const int rc = check_environment(sc, background, env_w, env_h, env_pixels);
    if (rc != MCPT_OK) return rc;
    return apply_environment(sc, background, env_w, env_h, env_pixels, info);
}

int mcpt_scene_set_visibility(mcpt_scene *sc, int32_t n, const mcpt_object_visibility *items, mcpt_update_info *info) {
    std::vector<uint8_t> visible;
    std::vector<int32_t> changed;
    const int rc = check_visibility(sc, n, items, visible, changed);
    if (rc != MCPT_OK) return rc;
    return apply_visibility(sc, visible, changed, info);
}

int mcpt_scene_get_visibility(const mcpt_scene *sc, int32_t n_objects, uint8_t *visible, int32_t *n_visible_prims) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_get_visibility: null scene");
    const SceneSource &S = sc->src;
    if (visible) {
        if (n_objects != (int32_t)S.objects.size()) return fail(MCPT_ERR_ARG, "mcpt_scene_get_visibility: n_objects is not the scene's object count");
        std::memcpy(visible, S.visible.data(), S.visible.size());
    }
    if (n_visible_prims) *n_visible_prims = count_visible_prims(S, S.visible);
    return MCPT_OK;
}

int mcpt_compact_scene(const mcpt_scene_desc *desc, const uint8_t *visible, mcpt_object *objects_out, mcpt_triangle *triangles_out, int32_t *n_objects_out,
                       int32_t *n_triangles_out, int32_t *prim_map) {
    if (!desc || !visible) return fail(MCPT_ERR_ARG, "mcpt_compact_scene: null argument");
    const char *err = "";
    const int rc = compact_scene_desc(*desc, visible, objects_out, triangles_out, n_objects_out, n_triangles_out, prim_map, &err);
    return rc == MCPT_OK ? rc : fail(rc, std::string("mcpt_compact_scene: ") + err);
}

int mcpt_scene_add_objects(mcpt_scene *sc, const mcpt_scene_addition *add, int32_t *first_object, mcpt_update_info *info) {
    const int rc = check_add(sc, add);
    if (rc != MCPT_OK) return rc;
    return apply_add(sc, add, first_object, info);
}

int mcpt_extend_scene(const mcpt_scene_desc *desc, const mcpt_scene_addition *add, mcpt_object *objects_out, mcpt_triangle *triangles_out,
                      mcpt_material *materials_out, int32_t *n_objects_out, int32_t *n_triangles_out, int32_t *n_materials_out) {
    if (!desc || !add) return fail(MCPT_ERR_ARG, "mcpt_extend_scene: null argument");
    const char *err = "";
    const int rc = extend_scene_desc(*desc, *add, objects_out, triangles_out, materials_out, n_objects_out, n_triangles_out, n_materials_out, &err);
    return rc == MCPT_OK ? rc : fail(rc, std::string("mcpt_extend_scene: ") + err);
}

int mcpt_scene_snapshot(mcpt_scene *sc) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_snapshot: null scene");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    const size_t nt = (size_t)sc->meta.n_triangles, ns = (size_t)sc->meta.n_sphere_slots;
    const auto copy_into = [&](DevBuf<TriGeom> &t, DevBuf<SphereRec> &s) -> int {
        if (nt) HIP_TRY(hipMemcpyAsync(t.p, sc->geom.tri_geom.p, nt * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
        if (ns) HIP_TRY(hipMemcpyAsync(s.p, sc->geom.spheres.p, ns * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return MCPT_OK;
    };
    if (sc->has_snapshot && sc->snap_tri.n == nt && sc->snap_sph.n == ns) return copy_into(sc->snap_tri, sc->snap_sph);
    DevBuf<TriGeom> t;  // new arrays aside: a failed allocation leaves the old snapshot as it was
    DevBuf<SphereRec> s;
    HIP_TRY(t.alloc(nt));
    HIP_TRY(s.alloc(ns));
    const int rc = copy_into(t, s);
    if (rc != MCPT_OK) return rc;
    sc->snap_tri.swap(t);
    sc->snap_sph.swap(s);
    sc->has_snapshot = true;
    return MCPT_OK;
}

void mcpt_scene_destroy(mcpt_scene *sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->device);
    (void)query_settle(sc);
#if defined(MCPT_TRAVERSAL_STATS) || defined(MCPT_CHECK_DIRECT_SKIP)
    if (sc->dbg.p) {
        unsigned long long h[36];
        if (hipMemcpy(h, sc->dbg.p, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
            if (h[23])
                std::fprintf(stderr, "[mcpt k_shade stats] %llu waves: %.0f cycles from start to the end of the allocation, of which %.0f in its first half (ballots, first barrier) and %.0f in the second barrier\n",
                             h[23], (double)h[22] / h[23], (double)h[20] / h[23], (double)h[21] / h[23]);
            if (h[24] + h[25] + h[26] + h[27] + h[28])
                std::fprintf(stderr, "[mcpt k_shade stats] waves by the number of material types among their shading lanes: 0: %llu, 1: %llu, 2: %llu, 3: %llu, 4: %llu; shading lanes %llu\n",
                             h[24], h[25], h[26], h[27], h[28], h[29]);
            if (h[16])
                std::fprintf(stderr, "[mcpt k_direct stats] vertices %llu, light samples %llu, zero samples %llu, vertices with only zero samples by cause: emitters behind the tangent plane %llu, Dirac otherwise %llu, rough otherwise %llu\n",
                             h[31], h[16], h[17], h[18], h[19], h[30]);
            if (h[16])
                std::fprintf(stderr, "[mcpt k_direct stats] Dirac otherwise, split: reflection %llu, refraction within the sin2 < 0.81 gate %llu, beyond the gate %llu, of which the total-internal-reflection rule claims %llu\n",
                             h[32], h[33], h[34] + h[35], h[35]);
            if (h[14]) std::fprintf(stderr, "[mcpt direct-skip check] light samples at skipped vertices: %llu, non-zero contributions among them: %llu\n", h[14], h[15]);
            for (int k = 0; k < 2; ++k) {
                const unsigned long long *d = h + 8 * k;
                if (!d[0]) continue;
                std::fprintf(stderr, "[mcpt traversal stats] %s: rays %llu, node visits/ray %.2f, prim tests/ray %.2f, %s %.3f, found %.3f, SIMD efficiency %.3f\n",
                             k ? "shadow" : "closest", d[0], (double)d[1] / d[0], (double)d[2] / d[0], k ? "occluded" : "hit",
                             (double)d[3] / d[0], (double)d[5] / d[0], (double)(d[1] + d[2]) / (double)d[4]);
            }
        }
    }
#endif
    delete sc;  // every member frees what it owns, in the order stated at struct mcpt_scene
}

int mcpt_bvh_dump(const mcpt_scene_desc *desc, mcpt_bvh_info *info, float *boxes, int32_t *children, uint16_t *qboxes,
                  float *inst_shift, int32_t *inst_root_first) {
    if (!desc || !info) return fail(MCPT_ERR_ARG, "mcpt_bvh_dump: null argument");
    HostScene hs;
    const char *err = "";
    const BuildChoice choice = resolve_build_choice(nullptr);
    if (choice.builder == MCPT_BUILD_GPU_LBVH || choice.builder == MCPT_BUILD_GPU_PLOC)
        return fail(MCPT_ERR_ARG, "mcpt_bvh_dump: the tree is built on the device (MCPT_BVH=lbvh / ploc): use mcpt_scene_dump_bvh");
    const int rc = build_host_scene(*desc, hs, &err, choice);
    if (rc != MCPT_OK) return fail(rc, std::string("mcpt_bvh_dump: ") + err);
    std::memset(info, 0, sizeof *info);
    const bool placeholder = hs.root < 0;  // a single primitive: no inner node (the array holds one unused record)
    info->n_nodes = placeholder ? 0 : (int32_t)hs.nodes.size();
    info->root = hs.root;
    info->stack_entries = hs.height;
    info->quantised = hs.qnodes.empty() ? 0 : 1;
    info->n_instances = (int32_t)hs.instances.size();
    info->n_leaf_prims = hs.n_leaf_prims;
    for (int k = 0; k < 3; ++k) {
        info->root_min[k] = hs.root_min[k];
        info->root_max[k] = hs.root_max[k];
        info->q_origin[k] = hs.q_origin[k];
        info->q_cell[k] = hs.q_cell[k];
    }
    for (size_t k = 0; k < hs.instances.size() && inst_shift && inst_root_first; ++k) {
        for (int c = 0; c < 3; ++c) inst_shift[3 * k + c] = hs.instances[k].shift[c];
        inst_root_first[2 * k] = hs.instances[k].root;
        inst_root_first[2 * k + 1] = hs.instances[k].first_tri;
    }
    if (!boxes || !children) return MCPT_OK;
    export_nodes(info->n_nodes, hs.nodes.data(), qboxes && info->quantised ? hs.qnodes.data() : nullptr, boxes, children, qboxes);
    return MCPT_OK;
}

int mcpt_scene_dump_bvh(mcpt_scene *sc, mcpt_bvh_info *info, float *boxes, int32_t *children, uint16_t *qboxes, float *inst_shift,
                        int32_t *inst_root_first) {
    if (!sc || !info) return fail(MCPT_ERR_ARG, "mcpt_scene_dump_bvh: null argument");
    HIP_TRY(hipSetDevice(sc->device));
    std::memset(info, 0, sizeof *info);
    const DevScene &v = sc->view;
    info->n_nodes = sc->meta.n_inner;
    info->root = v.root;
    info->stack_entries = v.height;
    info->quantised = v.qnodes ? 1 : 0;
    info->n_instances = sc->info.n_instances;
    info->n_leaf_prims = v.n_leaf_prims;
    if (info->n_instances > 0 && inst_shift && inst_root_first) {
        std::vector<InstRec> I((size_t)info->n_instances);
        HIP_TRY(download(I.data(), sc->inst, I.size()));
        for (size_t k = 0; k < I.size(); ++k) {
            for (int c = 0; c < 3; ++c) inst_shift[3 * k + c] = I[k].shift[c];
            inst_root_first[2 * k] = I[k].root;
            inst_root_first[2 * k + 1] = I[k].first_tri;
        }
    }
    for (int k = 0; k < 3; ++k) {
        info->root_min[k] = v.root_min[k];
        info->root_max[k] = v.root_max[k];
        info->q_origin[k] = v.q_origin[k];
        info->q_cell[k] = v.q_cell[k];
    }
    if (!boxes || !children || info->n_nodes == 0) return MCPT_OK;
    std::vector<Node> nodes((size_t)info->n_nodes);
    HIP_TRY(download(nodes.data(), sc->geom.nodes, nodes.size()));
    std::vector<QNode> qn;
    if (qboxes && info->quantised) {
        qn.resize(nodes.size());
        HIP_TRY(download(qn.data(), sc->geom.qnodes, qn.size()));
    }
    export_nodes(info->n_nodes, nodes.data(), qn.empty() ? nullptr : qn.data(), boxes, children, qboxes);
    return MCPT_OK;
}

int mcpt_scene_ray_counts(const mcpt_scene *sc, uint64_t *traced, uint64_t *shared) {
    if (!sc || !traced || !shared) return fail(MCPT_ERR_ARG, "mcpt_scene_ray_counts: null argument");
    *traced = sc->last_cont_traced;
    *shared = sc->last_cont_shared;
    return MCPT_OK;
}

int mcpt_scene_primary_conductor_counts(const mcpt_scene *sc, uint64_t *samples, uint64_t *rays) {
    if (!sc || !samples || !rays) return fail(MCPT_ERR_ARG, "mcpt_scene_primary_conductor_counts: null argument");
    *samples = sc->last_pc_samples;
    *rays = sc->last_pc_rays;
    return MCPT_OK;
}

int mcpt_scene_get_info(const mcpt_scene *sc, mcpt_scene_info *info) {
    if (!sc || !info) return fail(MCPT_ERR_ARG, "mcpt_scene_get_info: null argument");
    *info = sc->info;
    return MCPT_OK;
}

}  // extern "C"
