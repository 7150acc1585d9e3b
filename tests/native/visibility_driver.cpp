// Driver of tests/test_scene_visibility_cpu.py (a stand-alone program, no GPU): on random descriptions and masks the masked host build,
// build_host_scene(desc, mask), must equal the host build of the compacted description, build_host_scene(compact(desc, mask)), with
// primitive ids and sphere slots translated through prim_map: node boxes, quantised nodes, child references, height, root, light tables,
// the emitters' bounding sphere; and the records of every object, hidden or not, must be those of the unmasked build.
// Usage: visibility_driver <builder: 1 sah | 2 reference> <trials>.  Prints "ok <trials that built>" or the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "mcpt_internal.h"

using namespace mcpt;

template <typename T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static int fail_at(int trial, const char *what) {
    std::printf("trial %d: %s differs\n", trial, what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    BuildChoice choice;
    choice.builder = std::atoi(argv[1]);
    const int trials = std::atoi(argv[2]);
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> pos(-50.f, 50.f), ext(0.1f, 6.f);
    int built = 0;
    for (int trial = 0; trial < trials; ++trial) {
        const int no = 1 + (int)(rng() % 9);
        std::vector<mcpt_object> objs((size_t)no);
        std::vector<mcpt_triangle> tris;
        std::vector<mcpt_material> mats(3);
        std::memset(mats.data(), 0, mats.size() * sizeof(mcpt_material));
        mats[2].emission[0] = mats[2].emission[1] = mats[2].emission[2] = 5.f;
        for (int o = 0; o < no; ++o) {
            std::memset(&objs[(size_t)o], 0, sizeof(mcpt_object));
            objs[(size_t)o].material = (int32_t)(rng() % 3);
            if (rng() % 3 == 0) {
                objs[(size_t)o].kind = MCPT_OBJ_SPHERE;
                objs[(size_t)o].radius = ext(rng);
                for (int k = 0; k < 3; ++k) objs[(size_t)o].center[k] = pos(rng);
                continue;
            }
            objs[(size_t)o].kind = MCPT_OBJ_MESH;
            objs[(size_t)o].first_tri = (int32_t)tris.size();
            objs[(size_t)o].n_tri = 1 + (int32_t)(rng() % 70);
            const bool tied = rng() % 4 == 0;  // a mesh of identical triangles: every split decision is a tie
            const float c[3] = {pos(rng), pos(rng), pos(rng)};
            for (int k = 0; k < objs[(size_t)o].n_tri; ++k) {
                mcpt_triangle t;
                std::memset(&t, 0, sizeof t);
                for (int a = 0; a < 3; ++a) {
                    const float b = tied ? c[a] : c[a] + ext(rng) * 3.f;
                    t.v0[a] = b;
                    t.v1[a] = b + (tied ? 1.f + (float)a : ext(rng));
                    t.v2[a] = b - (tied ? 2.f - (float)a : ext(rng));
                }
                tris.push_back(t);
            }
        }
        std::vector<uint8_t> vis((size_t)no);
        for (uint8_t &v : vis) v = rng() % 3 != 0;
        mcpt_scene_desc d;
        std::memset(&d, 0, sizeof d);
        d.n_objects = no;
        d.objects = objs.data();
        d.n_triangles = (int32_t)tris.size();
        d.triangles = tris.data();
        d.n_materials = (int32_t)mats.size();
        d.materials = mats.data();
        const char *err = "";
        int32_t n_o = -1, n_t = -1;
        std::vector<int32_t> map(tris.size() + (size_t)no, -7);
        if (compact_scene_desc(d, vis.data(), nullptr, nullptr, &n_o, &n_t, map.data(), &err) != MCPT_OK) continue;  // every object hidden
        std::vector<mcpt_object> oo((size_t)n_o);
        std::vector<mcpt_triangle> tt((size_t)n_t);  // exactly the reported sizes
        if (compact_scene_desc(d, vis.data(), oo.data(), tt.data(), &n_o, &n_t, map.data(), &err) != MCPT_OK) return fail_at(trial, "second compaction");
        mcpt_scene_desc c = d;
        c.n_objects = n_o;
        c.objects = oo.data();
        c.n_triangles = n_t;
        c.triangles = tt.data();
        HostScene A, B, U;
        if (build_host_scene(c, A, &err, choice) != MCPT_OK) continue;  // (too deep, say: nothing to compare)
        if (build_host_scene(d, B, &err, choice, vis.data()) != MCPT_OK) return fail_at(trial, "the masked build's return code");
        if (build_host_scene(d, U, &err, choice) != MCPT_OK) return fail_at(trial, "the unmasked build's return code");
        ++built;
        const int32_t nt = d.n_triangles;
        const auto same_ref = [&](int32_t a, int32_t b) { return (a >= 0 || a == kNoChild) ? a == b : (b < 0 && b != kNoChild && map[(size_t)~b] == ~a); };
        if (A.root != B.root && !same_ref(A.root, B.root)) return fail_at(trial, "root");
        if (A.height != B.height || A.nodes.size() != B.nodes.size() || A.qnodes.size() != B.qnodes.size()) return fail_at(trial, "tree size");
        if (std::memcmp(A.root_min, B.root_min, 12) || std::memcmp(A.root_max, B.root_max, 12) || std::memcmp(A.q_origin, B.q_origin, 12) ||
            std::memcmp(A.q_cell, B.q_cell, 12))
            return fail_at(trial, "root box or grid");
        for (size_t i = 0; i < A.nodes.size(); ++i) {
            if (std::memcmp(A.nodes[i].lmin, B.nodes[i].lmin, 48)) return fail_at(trial, "node boxes");
            if (!same_ref(A.nodes[i].left, B.nodes[i].left) || !same_ref(A.nodes[i].right, B.nodes[i].right)) return fail_at(trial, "child references");
        }
        for (size_t i = 0; i < A.qnodes.size(); ++i)
            if (std::memcmp(A.qnodes[i].w, B.qnodes[i].w, 24) || !same_ref(A.qnodes[i].left, B.qnodes[i].left) || !same_ref(A.qnodes[i].right, B.qnodes[i].right))
                return fail_at(trial, "quantised nodes");
        // light tables: the same records, LightTri::prim and a sphere's slot translated
        if (A.lights.size() != B.lights.size() || A.light_nodes.size() != B.light_nodes.size() || A.light_tris.size() != B.light_tris.size())
            return fail_at(trial, "light table sizes");
        if (std::memcmp(&A.light_area_sum, &B.light_area_sum, 4) || std::memcmp(A.light_center, B.light_center, 12) || std::memcmp(&A.light_radius, &B.light_radius, 4))
            return fail_at(trial, "emitters' bounding sphere");
        if (!same_bytes(A.light_nodes, B.light_nodes)) return fail_at(trial, "light nodes");
        for (size_t i = 0; i < A.lights.size(); ++i) {
            LightRec a = A.lights[i], b = B.lights[i];
            if (a.kind == MCPT_OBJ_SPHERE) {
                if (map[(size_t)nt + (size_t)b.root] != n_t + a.root) return fail_at(trial, "a sphere light's slot");
                a.root = b.root = 0;
            }
            if (std::memcmp(&a, &b, sizeof a)) return fail_at(trial, "light records");
        }
        bool mesh_light = false;  // (without one the array holds a single placeholder record)
        for (const LightRec &l : A.lights) mesh_light = mesh_light || l.kind == MCPT_OBJ_MESH;
        if (mesh_light)
            for (size_t i = 0; i < A.light_tris.size(); ++i) {
                LightTri a = A.light_tris[i], b = B.light_tris[i];
                if (map[(size_t)b.prim] != a.prim) return fail_at(trial, "LightTri::prim");
                a.prim = b.prim = 0;
                if (std::memcmp(&a, &b, sizeof a)) return fail_at(trial, "light triangles");
            }
        // records: every object's, hidden or not, are those of the unmasked build, in the same places
        if (!same_bytes(B.tri_geom, U.tri_geom) || !same_bytes(B.tri_shade, U.tri_shade) || !same_bytes(B.spheres, U.spheres))
            return fail_at(trial, "primitive records");
    }
    std::printf("ok %d\n", built);
    return 0;
}
