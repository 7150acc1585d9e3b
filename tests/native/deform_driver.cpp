// Host build of the deformation arithmetic of csrc/mcpt_move.h for tests/test_scene_deform_cpu.py.  Compiled into a shared library with
// g++ -std=c++17 -O2 -ffp-contract=off: mv::deform_triangle forms the new base triangle, mv::move_triangle applies the object's transform
// unless `raw`, mv::derive_triangle gives the edges, the normal and the area -- the steps of a lane of k_deform_objects and of the host
// path of mcpt_scene_deform, in their order.
#include <cstdint>

#include "mcpt_move.h"

using namespace mcpt;

// out[i]: the moved triangle; derived[10 i ..]: e1, e2, n, area; finite[i]: mv::positions_finite of the nine floats
extern "C" void deform_lanes(int64_t n, const float *positions, const mcpt_triangle *in, int raw, const float *m, mcpt_triangle *out, float *derived,
                             int32_t *finite) {
    for (int64_t i = 0; i < n; ++i) {
        finite[i] = mv::positions_finite(positions + 9 * i) ? 1 : 0;
        mcpt_triangle t;
        mv::deform_triangle(positions + 9 * i, in[i], t);
        if (!raw) mv::move_triangle(m, t, t);
        out[i] = t;
        const mv::TriDerived D = mv::derive_triangle(mv::ld(t.v0), mv::ld(t.v1), mv::ld(t.v2));
        float *d = derived + 10 * i;
        d[0] = D.e1.x, d[1] = D.e1.y, d[2] = D.e1.z;
        d[3] = D.e2.x, d[4] = D.e2.y, d[5] = D.e2.z;
        d[6] = D.n.x, d[7] = D.n.y, d[8] = D.n.z;
        d[9] = D.area;
    }
}
