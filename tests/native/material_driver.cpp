// Host build of csrc/mcpt_material.h for tests/test_scene_materials_cpu.py.  Compiled into a shared library with
// g++ -std=c++17 -O2 -ffp-contract=off: mat::make_record is the function the scene builder and mcpt_scene_set_materials both call,
// mat::emits the predicate that selects the path, mat::plan_edit the argument checks and the segment table of k_set_materials.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mcpt_material.h"

using namespace mcpt;

extern "C" void material_records(int32_t n, const mcpt_material *mats, MaterialRec *out, int32_t *emits) {
    for (int32_t i = 0; i < n; ++i) {
        mat::make_record(mats[i], out[i]);
        emits[i] = mat::emits(mats[i]) ? 1 : 0;
    }
}

// head = {return code, in_place, n_lanes, n_tris, n_segs, n_lights, mat_lo, mat_hi}; segs: up to seg_cap MatSeg; lights: up to light_cap
// {light, mat} pairs; mats_out / objs_out: the description after the call (n_mats / n_objs records); err: the message (up to 255 chars)
extern "C" void material_plan(int32_t n_mats, const mcpt_material *mats, int32_t n_objs, const mcpt_object *objs, int32_t n_edits,
                              const mcpt_material_edit *edits, int32_t n_assign, const mcpt_object_material *assign, int32_t *head, mat::MatSeg *segs,
                              int32_t seg_cap, int32_t *lights, int32_t light_cap, mcpt_material *mats_out, mcpt_object *objs_out, char *err) {
    const std::vector<mcpt_material> M(mats, mats + n_mats);
    const std::vector<mcpt_object> O(objs, objs + n_objs);
    mat::EditPlan P;
    std::string e;
    head[0] = mat::plan_edit(M, O, n_edits, edits, n_assign, assign, P, e);
    std::strncpy(err, e.c_str(), 255);
    err[255] = 0;
    if (head[0] != MCPT_OK) return;
    head[1] = P.in_place ? 1 : 0;
    head[2] = P.n_lanes;
    head[3] = P.n_tris;
    head[4] = (int32_t)P.segs.size();
    head[5] = (int32_t)P.lights.size();
    head[6] = P.mat_lo;
    head[7] = P.mat_hi;
    for (int32_t i = 0; i < head[4] && i < seg_cap; ++i) segs[i] = P.segs[(size_t)i];
    for (int32_t i = 0; i < head[5] && i < light_cap; ++i) {
        lights[2 * i] = P.lights[(size_t)i].light;
        lights[2 * i + 1] = P.lights[(size_t)i].mat;
    }
    std::memcpy(mats_out, P.materials.data(), (size_t)n_mats * sizeof(mcpt_material));
    std::memcpy(objs_out, P.objects.data(), (size_t)n_objs * sizeof(mcpt_object));
}
