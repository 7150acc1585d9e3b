/*
 * mcpt_material.h -- what a material means to the device tables, and the plan of an in-place material edit (include/mcpt.h:
 * mcpt_scene_set_materials).
 *
 * Host only, no HIP: the scene builder (csrc/mcpt_scene.cpp), the edit call (csrc/mcpt_edit.hip) and the CPU tests
 * (tests/native/material_driver.cpp, built with g++) all compile these functions, so the MaterialRec of an edited entry is the one a
 * fresh scene would hold bit for bit, and the decision between the in-place path and the host path is one predicate.
 */
#ifndef MCPT_MATERIAL_H
#define MCPT_MATERIAL_H

#include <math.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mcpt_internal.h"

namespace mcpt {
namespace mat {

// Material::hasEmission (Material.hpp:262): the norm in Eigen's 3-term order, against EPSILON.
inline bool emits(const mcpt_material &m) {
    const float *e = m.emission;
    return sqrtf(e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])) > kEps;
}

inline bool type_ok(const mcpt_material &m) { return m.type >= 0 && m.type <= 3; }

inline bool finite(const mcpt_material &m) {
    const float f[9] = {m.roughness, m.iorA, m.iorB, m.base_reflectance[0], m.base_reflectance[1], m.base_reflectance[2],
                        m.emission[0], m.emission[1], m.emission[2]};
    bool ok = true;
    for (float v : f) ok = ok && (v - v == 0.f);  // (a NaN fails every comparison)
    return ok;
}

// The device record of a material, Material.hpp:245-262.  m.type must be in range (type_ok).
inline void make_record(const mcpt_material &m, MaterialRec &r) {
    std::memset(&r, 0, sizeof r);
    r.type = m.type;
    r.textured = m.textured ? 1 : 0;
    r.isDirac = (m.type == MCPT_SMOOTH_CONDUCTOR || m.type == MCPT_SMOOTH_DIELECTRIC);
    r.roughness = m.roughness;
    r.iorA = m.iorA;
    r.iorB = m.iorB;
    for (int k = 0; k < 3; ++k) {
        r.refl[k] = m.base_reflectance[k];
        r.emit[k] = m.emission[k];
    }
    r.hasEmission = emits(m);  // Material::hasEmission, Material.hpp:262
    const float wavelen[3] = {0.700f, 0.5461f, 0.4358f};  // WaveLen.hpp:7-18
    for (int k = 0; k < 3; ++k) {
        const float wl = wavelen[k];
        r.ior[k] = m.iorA + m.iorB / (wl * wl);          // Material.hpp:178-183
        r.inv_ior[k] = (float)(1. / (double)r.ior[k]);   // Material.hpp:299 `1. / ior`
    }
}

// The material words of a primitive's records, as build_host_scene forms them.
inline uint32_t tri_mat_bits(int32_t material, const mcpt_material &m) {
    return (uint32_t)material | (emits(m) ? kMatEmissive : 0u) | (m.textured ? kMatTextured : 0u);
}
inline uint32_t sphere_mat_bits(int32_t material, const mcpt_material &m) { return (uint32_t)material | (emits(m) ? kMatEmissive : 0u); }

// One run of lanes of k_set_materials (csrc/mcpt_update.hip): the triangles of one mesh, or one sphere.
struct alignas(16) MatSeg {
    int32_t first_lane;  // lanes [first_lane, first_lane + count) work on this segment
    int32_t count;       // mesh: its triangles; sphere: 1
    int32_t first_tri;   // mesh: its first triangle; sphere: -1
    int32_t object;      // sphere: its slot in the SphereRec array
    uint32_t mat_bits;   // the new TriGeom::mat_bits / SphereRec::mat_bits
    int32_t mat;         // the new TriShade::mat / SphereRec::mat
    int32_t pad[2];
};
static_assert(sizeof(MatSeg) == 32, "MatSeg must be 32 bytes");

// What mcpt_scene_set_materials is about to do, decided on the host before any device call.
struct EditPlan {
    std::vector<mcpt_material> materials;  // the table after the call
    std::vector<mcpt_object> objects;      // the objects after the call (only .material differs)
    bool in_place = true;                  // every object emits after the call iff it emitted before: path 2
    int32_t mat_lo = 0, mat_hi = 0;        // the listed material entries lie in [mat_lo, mat_hi) (empty: none listed)
    std::vector<MatSeg> segs;              // the primitives whose records change, in object order
    int32_t n_lanes = 0, n_tris = 0;       // lanes of the kernel; triangle records among them
    struct LightMat {
        int32_t light, mat;
    };
    std::vector<LightMat> lights;          // LightRec::mat of the reassigned emitters (the light table is in object order)
};

// The argument checks of mcpt_scene_set_materials that need no scene handle, then the plan.  Returns MCPT_OK or MCPT_ERR_ARG with `err`.
// An object is affected when it is listed in `assign`, or when it is a mesh whose material's `textured` flag changes.
inline int plan_edit(const std::vector<mcpt_material> &mats, const std::vector<mcpt_object> &objs, int32_t n_edits, const mcpt_material_edit *edits,
                     int32_t n_assign, const mcpt_object_material *assign, EditPlan &P, std::string &err) {
    const auto bad = [&](const std::string &m) {
        err = m;
        return (int)MCPT_ERR_ARG;
    };
    if (n_edits < 0 || n_assign < 0) return bad("a negative count");
    if ((n_edits > 0 && !edits) || (n_assign > 0 && !assign)) return bad("a positive count with a null list");
    const int32_t nm = (int32_t)mats.size(), no = (int32_t)objs.size();
    for (int32_t i = 0; i < n_edits; ++i) {
        if (edits[i].index < 0 || edits[i].index >= nm) return bad("material index " + std::to_string(edits[i].index) + " out of range");
        if (!type_ok(edits[i].material)) return bad("edit " + std::to_string(i) + ": material type out of range");
        if (!finite(edits[i].material)) return bad("edit " + std::to_string(i) + ": a material value is not finite");
    }
    for (int32_t i = 0; i < n_assign; ++i) {
        if (assign[i].object < 0 || assign[i].object >= no) return bad("object index " + std::to_string(assign[i].object) + " out of range");
        if (assign[i].material < 0 || assign[i].material >= nm) return bad("material index " + std::to_string(assign[i].material) + " out of range");
    }
    std::vector<uint8_t> seen_m((size_t)nm, 0), listed((size_t)no, 0);
    for (int32_t i = 0; i < n_edits; ++i) {
        if (seen_m[(size_t)edits[i].index]) return bad("material " + std::to_string(edits[i].index) + " is listed twice");
        seen_m[(size_t)edits[i].index] = 1;
    }
    for (int32_t i = 0; i < n_assign; ++i) {
        if (listed[(size_t)assign[i].object]) return bad("object " + std::to_string(assign[i].object) + " is listed twice");
        listed[(size_t)assign[i].object] = 1;
    }
    P = EditPlan();
    P.materials = mats;
    P.objects = objs;
    P.mat_lo = nm;
    for (int32_t i = 0; i < n_edits; ++i) {
        P.materials[(size_t)edits[i].index] = edits[i].material;
        P.mat_lo = std::min(P.mat_lo, edits[i].index);
        P.mat_hi = std::max(P.mat_hi, edits[i].index + 1);
    }
    if (n_edits == 0) P.mat_lo = P.mat_hi = 0;
    for (int32_t i = 0; i < n_assign; ++i) P.objects[(size_t)assign[i].object].material = assign[i].material;
    int32_t light = 0;
    for (int32_t o = 0; o < no; ++o) {
        const mcpt_object &was = objs[(size_t)o], &is = P.objects[(size_t)o];
        if (was.material < 0 || was.material >= nm) return bad("object " + std::to_string(o) + " holds a material index out of range");
        const mcpt_material &m0 = mats[(size_t)was.material], &m1 = P.materials[(size_t)is.material];
        const bool e0 = emits(m0), e1 = emits(m1);
        if (e0 != e1) P.in_place = false;
        if (e1 && listed[(size_t)o]) P.lights.push_back({light, is.material});
        light += e1 ? 1 : 0;
        const bool mesh = is.kind == MCPT_OBJ_MESH;
        if (!(listed[(size_t)o] || (mesh && (m0.textured != 0) != (m1.textured != 0)))) continue;
        MatSeg sg;
        std::memset(&sg, 0, sizeof sg);
        sg.first_lane = P.n_lanes;
        sg.count = mesh ? is.n_tri : 1;
        sg.first_tri = mesh ? is.first_tri : -1;
        sg.object = o;
        sg.mat_bits = mesh ? tri_mat_bits(is.material, m1) : sphere_mat_bits(is.material, m1);
        sg.mat = is.material;
        if (sg.count <= 0) continue;
        P.n_lanes += sg.count;
        P.n_tris += mesh ? sg.count : 0;
        P.segs.push_back(sg);
    }
    return MCPT_OK;
}

}  // namespace mat
}  // namespace mcpt

#endif /* MCPT_MATERIAL_H */
