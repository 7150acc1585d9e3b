// The live-edit layer of the C ABI (include/mcpt.h): mcpt_scene_update, mcpt_scene_deform, mcpt_scene_set_materials,
// mcpt_scene_set_visibility and mcpt_scene_add_objects are one path -- say what the edit is, choose a builder, build aside, commit --
// with mcpt_scene_set_environment beside it.  No kernels here: those are in csrc/mcpt_update.hip.  DESIGN.md section 8o.
#include <cmath>

#include "mcpt_host.h"
#include "mcpt_move.h"

using namespace mcpt;

namespace {

using mat::emits;  // Material::hasEmission (Material.hpp:262), as build_host_scene decides it

// ---- what an edit is: its kind and that kind's data, nothing else
struct MoveEdit { const std::vector<uint8_t> *moved; const std::vector<float> *xf; const std::vector<int32_t> *objects; };  // the transform table the scene gets; the objects whose entry differs
struct DeformEdit { int32_t n; const mcpt_object_vertices *items; };  // the listed meshes get these base positions
struct MaterialsEdit { const mat::EditPlan *plan; };                  // (not in place: mcpt::apply_material_edit keeps those)
struct VisibilityEdit { const std::vector<uint8_t> *mask; const std::vector<int32_t> *changed; };  // the mask the scene gets; the objects whose state differs
struct AddEdit { const mcpt_scene_addition *add; };
struct Edit {
    enum Kind { MOVE, DEFORM, MATERIALS, VISIBILITY, ADD } kind;
    union { MoveEdit move; DeformEdit deform; MaterialsEdit materials; VisibilityEdit visibility; AddEdit add; };
};

// What every message of a call starts with, by kind.
const char *const kPrefix[] = {"mcpt_scene_update: ", "mcpt_scene_deform: ", "mcpt_scene_set_materials: ", "mcpt_scene_set_visibility: ", "mcpt_scene_add_objects: "};

// No edit rebuilds a tree whose subtrees are shared.  MCPT_OK when the scene has none.
int refuse_instancing(const SceneSource &S, Edit::Kind k, const char *reason = "(instanced subtrees are shared between objects)") {
    if (S.choice.builder != MCPT_BUILD_SAH || S.choice.instancing != 1) return MCPT_OK;
    return fail(MCPT_ERR_ARG, std::string(kPrefix[k]) + "the scene was built with node instancing on " + reason);
}

// The objects whose records the edit writes: they decide info.n_moved_tris and, by whether one of them emits, the path.
std::vector<int32_t> edited_objects(const SceneSource &S, const Edit &e) {
    std::vector<int32_t> objs;
    if (e.kind == Edit::MOVE) objs = *e.move.objects;
    if (e.kind == Edit::VISIBILITY) objs = *e.visibility.changed;
    for (int32_t i = 0; e.kind == Edit::DEFORM && i < e.deform.n; ++i) objs.push_back(e.deform.items[i].object);
    for (int32_t i = 0; e.kind == Edit::ADD && i < e.add.add->n_objects; ++i) objs.push_back((int32_t)S.objects.size() + i);
    return objs;  // (a material edit that gets here rebuilds the light tables: no object's records alone)
}

// An addition extends the scene's own description in place (mcpt_extend_scene's rule), so that no second copy of the base triangles is
// alive while it is built; cut_to_meta takes that back, when the call fails (CutBack) and in mcpt::undo_add.  sc->meta still, or again,
// has the counts of the arrays the scene holds, and for every other kind the cut changes nothing.
void resize_source(SceneSource &S, size_t n_objects, size_t n_triangles, size_t n_materials) {
    S.objects.resize(n_objects);
    S.triangles.resize(n_triangles);
    S.materials.resize(n_materials);
    S.moved.resize(n_objects, 0);
    S.xf.resize(n_objects * 12, 0.f);
    S.visible.resize(n_objects, 1);
}
void cut_to_meta(mcpt_scene *sc) { resize_source(sc->src, (size_t)sc->meta.n_sphere_slots, (size_t)sc->meta.n_triangles, (size_t)sc->meta.n_mats); }
struct CutBack {
    mcpt_scene *sc;
    bool keep = false;
    ~CutBack() { if (!keep) cut_to_meta(sc); }
};
void extend_source(SceneSource &S, const mcpt_scene_addition &add) {
    const size_t no = S.objects.size(), nt = S.triangles.size(), nm = S.materials.size();
    resize_source(S, no + (size_t)add.n_objects, nt + (size_t)add.n_triangles, nm + (size_t)add.n_materials);
    for (int32_t i = 0; i < add.n_objects; ++i) {
        S.objects[no + (size_t)i] = add.objects[i];
        if (add.objects[i].kind == MCPT_OBJ_MESH) S.objects[no + (size_t)i].first_tri += (int32_t)nt;
    }
    std::copy(add.triangles, add.triangles + add.n_triangles, S.triangles.begin() + (ptrdiff_t)nt);
    std::copy(add.materials, add.materials + add.n_materials, S.materials.begin() + (ptrdiff_t)nm);
}

// The description the scene has after the edit: the caller's own vectors where the kind replaces a part, the scene's otherwise (an
// addition has extended those).  The commit assigns every part; a part the kind leaves alone assigns to itself.
struct After {
    const std::vector<mcpt_object> &objects;
    const std::vector<mcpt_triangle> &triangles;  // the base triangles (before a deformation's new positions: the builders apply those)
    const std::vector<mcpt_material> &materials;
    const std::vector<uint8_t> &moved, &visible;
    const std::vector<float> &xf;
};
After after(const SceneSource &S, const Edit &e) {
    const bool move = e.kind == Edit::MOVE, mats = e.kind == Edit::MATERIALS;
    return After{mats ? e.materials.plan->objects : S.objects, S.triangles, mats ? e.materials.plan->materials : S.materials, move ? *e.move.moved : S.moved,
                 e.kind == Edit::VISIBILITY ? *e.visibility.mask : S.visible, move ? *e.move.xf : S.xf};
}

// ---- the path choice: through the host (path 0), the edited objects' records written in HBM (path 1), or, for a change of visibility,
// which moves no record, the tree alone (path 1).  (A material edit with plan.in_place never gets here: mcpt::apply_material_edit, path 2.)
enum class Route { HOST, DEVICE_RECORDS, DEVICE_TREE };
Route choose_route(const mcpt_scene *sc, const Edit &e, const After &D, const std::vector<int32_t> &edited) {
    bool emitter = false;  // an edited object that emits: the light tables are formed again, which the creation code does
    for (int32_t o : edited) emitter = emitter || emits(D.materials[(size_t)D.objects[(size_t)o].material]);
    if (sc->meta.builder < 2 || emitter || e.kind == Edit::MATERIALS) return Route::HOST;
    return e.kind == Edit::VISIBILITY ? Route::DEVICE_TREE : Route::DEVICE_RECORDS;
}

std::vector<int32_t> sphere_list(const std::vector<mcpt_object> &objects) {  // the device builders' sphere list
    std::vector<int32_t> sph;
    for (size_t o = 0; o < objects.size(); ++o)
        if (objects[o].kind == MCPT_OBJ_SPHERE) sph.push_back((int32_t)o);
    return sph;
}

// ---- builder 1: the tree alone, on the device.  The tables of the visible ranges cross the bus, the device builder runs on the live
// triangles and sphere records.
int build_tree_on_device(mcpt_scene *sc, const After &D, EditAside &A, mcpt_update_info &ui) {
    const auto tt = Clock::now();
    DevVis dv;
    int rc = upload_vis(D.objects, D.visible, dv);
    if (rc != MCPT_OK) return rc;
    ui.transform_ms = ms_since(tt);
    const auto tb = Clock::now();
    rc = build_device_tree_checked(sc->geom.tris.p ? sc->geom.tris.p : sc->tris0.p, sc->sphere_obj.p, (int)sc->sphere_obj.n, sc->src.choice, A.geom, A.meta, &dv,
                                   sc->geom.spheres.p);
    if (rc != MCPT_OK) return rc;
    ui.build_ms = ms_since(tb);
    A.parts |= EditAside::TREE;
    return MCPT_OK;
}

// ---- builder 2: records on the device.  First the live records, copied into arrays of the target size (nt2 triangles, ns2 sphere slots;
// added slots start zero-filled, as the host leaves the slots of meshes); with new_base the base triangles too.
int copy_live_records(const mcpt_scene *sc, size_t nt2, size_t ns2, bool new_base, EditAside &A) {
    const GeomBufs &g = sc->geom;
    GeomBufs &g2 = A.geom;
    const size_t nt = (size_t)sc->meta.n_triangles, ns = g.spheres.n;
    HIP_TRY(g2.tri_geom.alloc(nt2));
    HIP_TRY(g2.tri_shade.alloc(nt2));
    HIP_TRY(g2.tris.alloc(nt2));
    HIP_TRY(g2.spheres.alloc(ns2));
    if (new_base) HIP_TRY(A.tris0.alloc(nt2));
    if (nt) {
        HIP_TRY(hipMemcpyAsync(g2.tri_geom.p, g.tri_geom.p, nt * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(g2.tri_shade.p, g.tri_shade.p, nt * sizeof(TriShade), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(g2.tris.p, g.tris.p ? g.tris.p : sc->tris0.p, nt * sizeof(mcpt_triangle), hipMemcpyDeviceToDevice, nullptr));
        if (new_base) HIP_TRY(hipMemcpyAsync(A.tris0.p, sc->tris0.p, nt * sizeof(mcpt_triangle), hipMemcpyDeviceToDevice, nullptr));
    }
    if (ns) HIP_TRY(hipMemcpyAsync(g2.spheres.p, g.spheres.p, ns * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
    if (ns2 > ns) HIP_TRY(hipMemsetAsync(g2.spheres.p + ns, 0, (ns2 - ns) * sizeof(SphereRec), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MCPT_OK;
}

// Then the kind's segment table and its kernel.  Move: the listed triangles and sphere centres are moved in HBM.
int launch_move(mcpt_scene *sc, const MoveEdit &m, const After &D, EditAside &A) {
    std::vector<MoveSeg> segs;
    int32_t lanes = 0;
    for (int32_t o : *m.objects) {
        const mcpt_object &ob = D.objects[(size_t)o];
        MoveSeg sg;
        std::memset(&sg, 0, sizeof sg);
        sg.first_lane = lanes;
        sg.count = ob.kind == MCPT_OBJ_MESH ? ob.n_tri : 1;
        sg.first_tri = ob.kind == MCPT_OBJ_MESH ? ob.first_tri : -1;
        sg.object = o;
        std::memcpy(sg.m, &D.xf[(size_t)o * 12], sizeof sg.m);
        for (int k = 0; k < 3; ++k) sg.c0[k] = ob.center[k];
        sg.raw = D.moved[(size_t)o] ? 0 : 1;
        lanes += sg.count;
        segs.push_back(sg);
    }
    HIP_TRY(upload(sc->segs, segs));
    launch_move_objects(sc->segs.p, (int32_t)segs.size(), lanes, sc->tris0.p, A.geom.tris.p, A.geom.tri_geom.p, A.geom.tri_shade.p, A.geom.spheres.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MCPT_OK;
}

// Deform: host positions go through the staging buffer in one copy, device positions are read where they are; the kernel writes the new
// base triangles beside the records.
int launch_deform(mcpt_scene *sc, const DeformEdit &d, const After &D, EditAside &A) {
    std::vector<float> staged;
    std::vector<size_t> at((size_t)d.n, 0);
    for (int32_t i = 0; i < d.n; ++i) {
        if (d.items[i].on_device) continue;
        at[(size_t)i] = staged.size();
        staged.insert(staged.end(), d.items[i].positions, d.items[i].positions + (size_t)D.objects[(size_t)d.items[i].object].n_tri * 9);
    }
    HIP_TRY(upload(sc->stage, staged));
    std::vector<DeformSeg> dsegs;
    int32_t lanes = 0;
    for (int32_t i = 0; i < d.n; ++i) {
        const int32_t o = d.items[i].object;
        const mcpt_object &ob = D.objects[(size_t)o];
        if (ob.n_tri <= 0) continue;
        DeformSeg sg;
        std::memset(&sg, 0, sizeof sg);
        sg.first_lane = lanes;
        sg.first_tri = ob.first_tri;
        sg.object = o;
        sg.raw = D.moved[(size_t)o] ? 0 : 1;
        std::memcpy(sg.m, &D.xf[(size_t)o * 12], sizeof sg.m);
        sg.positions = d.items[i].on_device ? d.items[i].positions : sc->stage.p + at[(size_t)i];
        lanes += ob.n_tri;
        dsegs.push_back(sg);
    }
    HIP_TRY(upload(sc->dsegs, dsegs));
    HIP_TRY(sc->dflag.alloc(1));
    HIP_TRY(hipMemsetAsync(sc->dflag.p, 0, sizeof(uint32_t), nullptr));
    launch_deform_objects(sc->dsegs.p, (int32_t)dsegs.size(), lanes, sc->tris0.p, A.tris0.p, A.geom.tris.p, A.geom.tri_geom.p, A.geom.tri_shade.p, sc->dflag.p, nullptr);
    HIP_TRY(hipGetLastError());
    uint32_t flag = 0;  // (a blocking copy on the null stream: the kernel has finished when it returns)
    HIP_TRY(download(&flag, sc->dflag, 1));
    if (flag) return fail(MCPT_ERR_ARG, "mcpt_scene_deform: a position given by device pointer is not finite");
    return MCPT_OK;
}

// Add: the added triangles go behind the base, the sphere list and the material table are made at the new size, and the kernel writes the
// whole records of the added primitives from their triangles.
int launch_add(mcpt_scene *sc, const AddEdit &a, const After &D, EditAside &A) {
    const mcpt_scene_addition &add = *a.add;
    const size_t no = (size_t)sc->meta.n_sphere_slots, nt = (size_t)sc->meta.n_triangles;  // what the scene holds: the description is already extended
    if (add.n_triangles) HIP_TRY(hipMemcpy(A.tris0.p + nt, add.triangles, (size_t)add.n_triangles * sizeof(mcpt_triangle), hipMemcpyHostToDevice));
    HIP_TRY(upload(A.sphere_obj, sphere_list(D.objects)));
    std::vector<MaterialRec> recs(D.materials.size());
    for (size_t i = 0; i < recs.size(); ++i) mat::make_record(D.materials[i], recs[i]);
    HIP_TRY(upload(A.mats, recs));
    std::vector<AddSeg> segs;
    int32_t lanes = 0;
    for (size_t o = no; o < D.objects.size(); ++o) {
        const mcpt_object &ob = D.objects[o];
        const mcpt_material &m = D.materials[(size_t)ob.material];
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
    launch_add_objects(sc->asegs.p, (int32_t)segs.size(), lanes, A.tris0.p, A.geom.tris.p, A.geom.tri_geom.p, A.geom.tri_shade.p, A.geom.spheres.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    A.meta.n_triangles = (int32_t)D.triangles.size();
    A.meta.n_objects = A.meta.n_sphere_slots = (int32_t)D.objects.size();
    A.meta.n_mats = (int32_t)D.materials.size();
    return MCPT_OK;
}

// The nine position floats of every triangle of the listed meshes on the host, item by item: the caller's own arrays, or downloads of
// the arrays given by device pointer (kept in A.fetched).  The scene's device must be current.
int host_positions(const SceneSource &S, const DeformEdit &d, EditAside &A) {
    A.fetched.assign((size_t)d.n, {});
    A.patch.clear();
    for (int32_t i = 0; i < d.n; ++i) {
        const int32_t o = d.items[i].object;
        A.patch.push_back({o, d.items[i].positions});
        const size_t nf = (size_t)S.objects[(size_t)o].n_tri * 9;
        if (!d.items[i].on_device || nf == 0) continue;
        A.fetched[(size_t)i].resize(nf);
        HIP_TRY(hipMemcpy(A.fetched[(size_t)i].data(), d.items[i].positions, nf * sizeof(float), hipMemcpyDeviceToHost));
        A.patch.back().second = A.fetched[(size_t)i].data();
    }
    return MCPT_OK;
}

// The copy block, the kind's launch, then the visibility tables and the tree: move, deform and add differ in the launch alone.
int build_records_on_device(mcpt_scene *sc, const Edit &e, const After &D, EditAside &A, mcpt_update_info &ui) {
    const bool add = e.kind == Edit::ADD, new_base = add || e.kind == Edit::DEFORM;
    const auto tu = Clock::now();
    int rc = copy_live_records(sc, D.triangles.size(), add ? D.objects.size() : sc->geom.spheres.n, new_base, A);
    if (rc != MCPT_OK) return rc;
    ui.upload_ms = ms_since(tu);
    const auto tt = Clock::now();
    rc = add ? launch_add(sc, e.add, D, A) : (e.kind == Edit::DEFORM ? launch_deform(sc, e.deform, D, A) : launch_move(sc, e.move, D, A));
    if (rc != MCPT_OK) return rc;
    DevVis dv;
    rc = upload_vis(D.objects, D.visible, dv);
    if (rc != MCPT_OK) return rc;
    ui.transform_ms = ms_since(tt);
    const auto tb = Clock::now();
    const DevBuf<int32_t> &sph = add ? A.sphere_obj : sc->sphere_obj;
    rc = build_device_tree_checked(A.geom.tris.p, sph.p, (int)sph.n, sc->src.choice, A.geom, A.meta, &dv);
    if (rc != MCPT_OK) return rc;
    ui.build_ms = ms_since(tb);
    if (e.kind == Edit::DEFORM) {  // the host copy of the base follows at the commit (36 B per triangle come back for positions given by device pointer)
        rc = host_positions(sc->src, e.deform, A);
        if (rc != MCPT_OK) return rc;
        A.parts |= EditAside::PATCH;
    }
    A.parts |= EditAside::TREE | EditAside::PRIMS | (new_base ? EditAside::TRIS0 : 0u) | (add ? EditAside::SPHERE_OBJ | EditAside::MATS : 0u);
    return MCPT_OK;
}

// ---- builder 3: through the host.
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

// A deformation's positions applied to `tris`, the base triangles; positions given by device pointer are downloaded first, and checked here.
int deform_on_host(const SceneSource &S, const DeformEdit &d, EditAside &A, std::vector<mcpt_triangle> &tris) {
    const int rc = host_positions(S, d, A);
    if (rc != MCPT_OK) return rc;
    for (int32_t i = 0; i < d.n; ++i) {
        const mcpt_object &ob = S.objects[(size_t)d.items[i].object];
        const float *pos = A.patch[(size_t)i].second;
        for (int32_t k = 0; k < ob.n_tri; ++k) {
            if (d.items[i].on_device && !mv::positions_finite(pos + (size_t)k * 9))
                return fail(MCPT_ERR_ARG, "mcpt_scene_deform: a position given by device pointer is not finite");
            mv::deform_triangle(pos + (size_t)k * 9, tris[(size_t)ob.first_tri + k], tris[(size_t)ob.first_tri + k]);
        }
    }
    return MCPT_OK;
}

// The transforms are applied to the kind's description; desc' (objs, tris, D.materials) is flattened and its tree built as at creation,
// with the mask D.visible; every array that depends on the geometry is copied into the aside (device builders: the moved triangles too,
// and the tree is built there); then the base triangles (device builders, when the kind replaces them) and the material table (when
// the kind replaces it).
int build_through_host(mcpt_scene *sc, const Edit &e, const After &D, EditAside &A, mcpt_update_info &ui) {
    const bool add = e.kind == Edit::ADD, new_base = add || e.kind == Edit::DEFORM, new_mats = add || e.kind == Edit::MATERIALS;
    const auto tt = Clock::now();
    std::vector<mcpt_triangle> tris = D.triangles;
    if (e.kind == Edit::DEFORM) {
        const int rc = deform_on_host(sc->src, e.deform, A, tris);
        if (rc != MCPT_OK) return rc;
        A.triangles = tris;  // the new base
        A.parts |= EditAside::TRIANGLES;
    }
    std::vector<mcpt_object> objs = D.objects;
    apply_current_transforms(objs, tris, D.moved, D.xf);
    ui.transform_ms = ms_since(tt);
    if (add && A.meta.builder >= 2) HIP_TRY(upload(A.sphere_obj, sphere_list(D.objects)));
    const auto tb = Clock::now();
    mcpt_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_objects = (int32_t)objs.size();
    d.n_triangles = (int32_t)tris.size();
    d.n_materials = (int32_t)D.materials.size();
    for (int k = 0; k < 3; ++k) d.background[k] = A.meta.background[k];
    d.objects = objs.data();
    d.triangles = tris.data();
    d.materials = D.materials.data();
    HostScene hs;
    const char *err = "";
    const bool masked = std::find(D.visible.begin(), D.visible.end(), (uint8_t)0) != D.visible.end();
    int rc = build_host_scene(d, hs, &err, sc->src.choice, masked ? D.visible.data() : nullptr);
    if (rc != MCPT_OK) return fail(rc, std::string(kPrefix[e.kind]) + err);
    const double host_build_ms = ms_since(tb);
    const auto tu = Clock::now();
    const int32_t env_w = A.meta.env_w, env_h = A.meta.env_h;  // (the environment map is not part of desc': it stays where it is)
    A.meta = meta_of(hs);
    A.meta.env_w = env_w;
    A.meta.env_h = env_h;
    DevVis dv;
    if (hs.builder >= 2) {
        HIP_TRY(upload(A.geom.tris, tris));
        rc = upload_vis(objs, D.visible, dv);
        if (rc != MCPT_OK) return rc;
    }
    double gpu_build_ms = 0.0;
    rc = upload_geometry(hs, sc->src.choice, A.geom.tris.p, add ? A.sphere_obj.p : sc->sphere_obj.p, A.geom, A.meta, gpu_build_ms, &dv);
    if (rc != MCPT_OK) return rc;
    ui.build_ms = host_build_ms + gpu_build_ms;
    if (new_base && hs.builder >= 2) {
        HIP_TRY(upload(A.tris0, add ? D.triangles : A.triangles));
        A.parts |= EditAside::TRIS0;
    }
    if (new_mats) HIP_TRY(upload(A.mats, hs.materials));
    ui.upload_ms = ms_since(tu) - gpu_build_ms;
    A.parts |= EditAside::TREE | EditAside::PRIMS | EditAside::LIGHTS | (new_mats ? EditAside::MATS : 0u) | (add ? EditAside::SPHERE_OBJ : 0u);
    return MCPT_OK;
}

// ---- an addition alone: the snapshot at the new size, what it held and then the added objects' records as added
int extend_snapshot(const mcpt_scene *sc, const After &D, EditAside &A) {
    const size_t nt = (size_t)sc->meta.n_triangles, nt2 = D.triangles.size(), no = (size_t)sc->meta.n_sphere_slots, no2 = D.objects.size();
    HIP_TRY(A.snap_tri.alloc(nt2));
    HIP_TRY(A.snap_sph.alloc(no2));
    if (nt) HIP_TRY(hipMemcpyAsync(A.snap_tri.p, sc->snap_tri.p, nt * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
    if (nt2 > nt) HIP_TRY(hipMemcpyAsync(A.snap_tri.p + nt, A.geom.tri_geom.p + nt, (nt2 - nt) * sizeof(TriGeom), hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(A.snap_sph.p, sc->snap_sph.p, no * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(A.snap_sph.p + no, A.geom.spheres.p + no, (no2 - no) * sizeof(SphereRec), hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    A.parts |= EditAside::SNAPSHOT;
    return MCPT_OK;
}

// ---- the commit: the device arrays the aside holds are exchanged with the scene's, part by part, and the description becomes D.  Nothing
// here can fail.  Afterwards the aside holds the arrays the scene had: committing it again with the scene's own description puts them
// back (mcpt::undo_add).
void commit(mcpt_scene *sc, EditAside &A, const After &D) {
    SceneSource &S = sc->src;
    const auto has = [&](uint32_t part) { return (A.parts & part) != 0; };
    if (has(EditAside::PRIMS)) sc->geom.swap_prims(A.geom);  // (the tree with them)
    else if (has(EditAside::TREE)) sc->geom.swap_nodes(A.geom);
    if (has(EditAside::LIGHTS)) sc->geom.swap_lights(A.geom);
    if (has(EditAside::TRIS0)) sc->tris0.swap(A.tris0);
    if (has(EditAside::SPHERE_OBJ)) sc->sphere_obj.swap(A.sphere_obj);
    if (has(EditAside::MATS)) sc->mats.swap(A.mats);
    if (has(EditAside::SNAPSHOT)) {
        sc->snap_tri.swap(A.snap_tri);
        sc->snap_sph.swap(A.snap_sph);
    }
    std::swap(sc->meta, A.meta);
    S.objects = D.objects;
    S.materials = D.materials;
    S.moved = D.moved;
    S.xf = D.xf;
    S.visible = D.visible;
    if (has(EditAside::TRIANGLES)) S.triangles.swap(A.triangles);  // a deformation through the host: the new base
    if (has(EditAside::PATCH))  // a deformation on the device path: the host copy of the base is patched in place
        for (const auto &[o, pos] : A.patch) {
            const mcpt_object &ob = S.objects[(size_t)o];
            for (int32_t k = 0; k < ob.n_tri; ++k) mv::deform_triangle(pos + (size_t)k * 9, S.triangles[(size_t)ob.first_tri + k], S.triangles[(size_t)ob.first_tri + k]);
        }
    fill_view(sc);
}

// ---- the one path.  Everything is built aside (in *keep when the caller wants what the scene had: mcpt_group_add_objects) and committed
// once the new tree is known to be usable, so a failed call leaves the description and every device array as they were.
int run_edit(mcpt_scene *sc, const Edit &e, mcpt_update_info *info, EditAside *keep = nullptr) {
    const auto t0 = Clock::now();
    mcpt_update_info ui;
    std::memset(&ui, 0, sizeof ui);
    const SceneSource &S = sc->src;
    const std::vector<int32_t> edited = edited_objects(S, e);
    for (int32_t o : edited)
        if (e.kind != Edit::ADD && S.objects[(size_t)o].kind == MCPT_OBJ_MESH) ui.n_moved_tris += S.objects[(size_t)o].n_tri;
    if (e.kind == Edit::MATERIALS) ui.n_moved_tris = e.materials.plan->n_tris;
    if (e.kind == Edit::ADD) ui.n_moved_tris = e.add.add->n_triangles;
    if (edited.empty() && e.kind != Edit::MATERIALS) {  // nothing changes: no device call
        if (info) *info = ui;
        return MCPT_OK;
    }
    HIP_TRY(hipSetDevice(sc->device));
    HIP_TRY(query_settle(sc, e.kind == Edit::ADD));  // a ray query still in flight reads the arrays this call swaps and frees
    EditAside local;
    EditAside &A = keep ? *keep : local;
    CutBack cut{sc};  // a failed call leaves the description as it was
    if (e.kind == Edit::ADD) extend_source(sc->src, *e.add.add);
    A.meta = sc->meta;
    const After D = after(S, e);
    const Route route = choose_route(sc, e, D, edited);
    ui.path = route == Route::HOST ? 0 : 1;
    int rc = route == Route::HOST             ? build_through_host(sc, e, D, A, ui)
             : route == Route::DEVICE_RECORDS ? build_records_on_device(sc, e, D, A, ui)
                                              : build_tree_on_device(sc, D, A, ui);
    if (rc == MCPT_OK && e.kind == Edit::ADD && sc->has_snapshot) rc = extend_snapshot(sc, D, A);
    if (rc != MCPT_OK) return rc;
    commit(sc, A, D);
    cut.keep = true;
    ui.total_ms = ms_since(t0);
    if (info) *info = ui;
    return MCPT_OK;
}

}  // namespace

// ---- the checks of each call, before any device call, and the call itself
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
    if (const int rc = refuse_instancing(S, Edit::MOVE)) return rc;
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

int mcpt::apply_transforms(mcpt_scene *sc, const std::vector<uint8_t> &moved, const std::vector<float> &xf, const std::vector<int32_t> &touched,
                           mcpt_update_info *info) {
    Edit e{Edit::MOVE, {}};
    e.move = MoveEdit{&moved, &xf, &touched};
    return run_edit(sc, e, info);
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
    if (const int rc = refuse_instancing(S, Edit::DEFORM)) return rc;
    for (int32_t i = 0; i < n; ++i) {
        if (items[i].on_device) continue;
        for (int32_t k = 0; k < S.objects[(size_t)items[i].object].n_tri; ++k)
            if (!mv::positions_finite(items[i].positions + (size_t)k * 9))
                return fail(MCPT_ERR_ARG, "mcpt_scene_deform: item " + std::to_string(i) + ": a position is not finite");
    }
    return MCPT_OK;
}

int mcpt::apply_deform(mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items, mcpt_update_info *info) {
    Edit e{Edit::DEFORM, {}};
    e.deform = DeformEdit{n, items};
    return run_edit(sc, e, info);
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
    if (const int rc = refuse_instancing(S, Edit::VISIBILITY)) return rc;
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
    Edit e{Edit::VISIBILITY, {}};
    e.visibility = VisibilityEdit{&visible, &changed};
    return run_edit(sc, e, info);
}

int mcpt::check_add(const mcpt_scene *sc, const mcpt_scene_addition *add) {
    if (!sc || !add) return fail(MCPT_ERR_ARG, "mcpt_scene_add_objects: null argument");
    const SceneSource &S = sc->src;
    const char *err = "";
    const int rc = check_scene_addition((int32_t)S.objects.size(), (int32_t)S.triangles.size(), (int32_t)S.materials.size(), *add, &err);
    if (rc != MCPT_OK) return fail(rc, std::string("mcpt_scene_add_objects: ") + err);
    return refuse_instancing(S, Edit::ADD);
}

int mcpt::apply_add(mcpt_scene *sc, const mcpt_scene_addition *add, int32_t *first_object, mcpt_update_info *info, AddAside *keep) {
    const int32_t first = (int32_t)sc->src.objects.size();
    Edit e{Edit::ADD, {}};
    e.add = AddEdit{add};
    const int rc = run_edit(sc, e, info, keep);
    if (rc == MCPT_OK && first_object) *first_object = first;
    return rc;
}

int mcpt::undo_add(mcpt_scene *sc, AddAside &A) {
    HIP_TRY(hipSetDevice(sc->device));
    HIP_TRY(query_settle(sc, true));
    commit(sc, A, after(sc->src, Edit{Edit::ADD, {}}));  // (the description as it is: only the arrays go back, then the cut)
    cut_to_meta(sc);
    return MCPT_OK;
}

int mcpt::check_material_edit(const mcpt_scene *sc, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign, const mcpt_object_material *assign,
                              mat::EditPlan &plan) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_set_materials: null scene");
    const SceneSource &S = sc->src;
    std::string err;
    const int rc = mat::plan_edit(S.materials, S.objects, n_edits, edits, n_assign, assign, plan, err);
    if (rc != MCPT_OK) return fail(rc, "mcpt_scene_set_materials: " + err);
    return refuse_instancing(S, Edit::MATERIALS, "(instanced groups were formed from non-emitting meshes)");
}

int mcpt::apply_material_edit(mcpt_scene *sc, const mat::EditPlan &plan, mcpt_update_info *info) {
    if (!plan.in_place) {  // some object starts or stops emitting: the creation code forms the light tables again
        Edit e{Edit::MATERIALS, {}};
        e.materials = MaterialsEdit{&plan};
        return run_edit(sc, e, info);
    }
    // path 2: the live records are patched where they are; nothing is built aside, so the description follows at the end
    SceneSource &S = sc->src;
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

extern "C" {

int mcpt_scene_update(mcpt_scene *sc, int32_t n, const mcpt_object_transform *moves, mcpt_update_info *info) {
    std::vector<uint8_t> moved;
    std::vector<float> xf;
    std::vector<int32_t> touched;
    const int rc = check_moves(sc, n, moves, moved, xf, touched);
    return rc != MCPT_OK ? rc : apply_transforms(sc, moved, xf, touched, info);
}

int mcpt_scene_deform(mcpt_scene *sc, int32_t n, const mcpt_object_vertices *items, mcpt_update_info *info) {
    const int rc = check_deform(sc, n, items);
    return rc != MCPT_OK ? rc : apply_deform(sc, n, items, info);
}

int mcpt_scene_set_materials(mcpt_scene *sc, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign, const mcpt_object_material *assign,
                             mcpt_update_info *info) {
    mat::EditPlan plan;
    const int rc = check_material_edit(sc, n_edits, edits, n_assign, assign, plan);
    return rc != MCPT_OK ? rc : apply_material_edit(sc, plan, info);
}

int mcpt_scene_set_environment(mcpt_scene *sc, const float background[3], int32_t env_w, int32_t env_h, const float *env_pixels, mcpt_update_info *info) {
    const int rc = check_environment(sc, background, env_w, env_h, env_pixels);
    return rc != MCPT_OK ? rc : apply_environment(sc, background, env_w, env_h, env_pixels, info);
}

int mcpt_scene_set_visibility(mcpt_scene *sc, int32_t n, const mcpt_object_visibility *items, mcpt_update_info *info) {
    std::vector<uint8_t> visible;
    std::vector<int32_t> changed;
    const int rc = check_visibility(sc, n, items, visible, changed);
    return rc != MCPT_OK ? rc : apply_visibility(sc, visible, changed, info);
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

int mcpt_scene_add_objects(mcpt_scene *sc, const mcpt_scene_addition *add, int32_t *first_object, mcpt_update_info *info) {
    const int rc = check_add(sc, add);
    return rc != MCPT_OK ? rc : apply_add(sc, add, first_object, info);
}

}  // extern "C"
