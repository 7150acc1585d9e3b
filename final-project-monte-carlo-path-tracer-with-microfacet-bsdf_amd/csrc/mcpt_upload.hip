// Scene create / upload / destroy / info and the BVH dumps of the C ABI (include/mcpt.h); mcpt_last_error and mcpt_version.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>

#include "mcpt_host.h"

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

SceneMeta mcpt::meta_of(const HostScene &hs) {
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

int32_t mcpt::count_visible_prims(const SceneSource &S, const std::vector<uint8_t> &visible) {
    int32_t n = 0;
    for (size_t o = 0; o < S.objects.size(); ++o)
        if (visible[o]) n += S.objects[o].kind == MCPT_OBJ_MESH ? S.objects[o].n_tri : 1;
    return n;
}

int mcpt::upload_vis(const std::vector<mcpt_object> &objects, const std::vector<uint8_t> &visible, DevVis &dv) {
    dv.active = std::find(visible.begin(), visible.end(), (uint8_t)0) != visible.end();
    if (!dv.active) return MCPT_OK;
    std::vector<VisSeg> segs;
    std::vector<int32_t> sph;
    for (size_t o = 0; o < objects.size(); ++o) {
        if (!visible[o]) continue;
        if (objects[o].kind == MCPT_OBJ_MESH) segs.push_back(VisSeg{0, objects[o].first_tri, objects[o].n_tri});
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
// by the visible count.  d_spheres: the SphereRec array the builder reads (g's own unless the caller builds a tree alone).  Ends with the
// depth check every tree gets before it is used.
int mcpt::build_device_tree_checked(const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, int n_sph, const BuildChoice &choice, GeomBufs &g, SceneMeta &meta,
                                    const DevVis *dv, const SphereRec *d_spheres) {
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
    if (traversal_stack_entries(meta.height) < meta.height - 1) return fail(MCPT_ERR_LIMIT, "the BVH is deeper than the traversal stack (kMaxBvhHeight)");
    return MCPT_OK;
}

int mcpt::upload_geometry(const HostScene &hs, const BuildChoice &choice, const mcpt_triangle *d_tris, const int32_t *d_sphere_obj, GeomBufs &g, SceneMeta &meta,
                          double &gpu_build_ms, const DevVis *dv) {
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
        const int rc = build_device_tree_checked(d_tris, d_sphere_obj, (int)hs.sphere_objects.size(), choice, g, meta, dv);
        if (rc != MCPT_OK) return rc;
        gpu_build_ms = ms_since(tb);
    } else if (traversal_stack_entries(meta.height) < meta.height - 1) {  // (the device builder has checked its own) a push beyond the stack would be dropped
        return fail(MCPT_ERR_LIMIT, "the BVH is deeper than the traversal stack (kMaxBvhHeight)");
    }
    return MCPT_OK;
}

void mcpt::fill_view(mcpt_scene *sc) {
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

int mcpt_compact_scene(const mcpt_scene_desc *desc, const uint8_t *visible, mcpt_object *objects_out, mcpt_triangle *triangles_out, int32_t *n_objects_out,
                       int32_t *n_triangles_out, int32_t *prim_map) {
    if (!desc || !visible) return fail(MCPT_ERR_ARG, "mcpt_compact_scene: null argument");
    const char *err = "";
    const int rc = compact_scene_desc(*desc, visible, objects_out, triangles_out, n_objects_out, n_triangles_out, prim_map, &err);
    return rc == MCPT_OK ? rc : fail(rc, std::string("mcpt_compact_scene: ") + err);
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
