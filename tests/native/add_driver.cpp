// Driver of tests/test_scene_add_cpu.py (a stand-alone program, no GPU): on random small descriptions and additions the host build of
// the extended description, build_host_scene(extend(desc, add)), must equal the host build of a description concatenated by hand here
// (objects, then added objects with first_tri shifted; triangles, then added triangles; materials, then added materials): the tree,
// the quantised nodes, the primitive records, the material records and the light tables, byte for byte.  Additions list their meshes'
// triangle ranges in random order and may leave triangles unused.
// Usage: add_driver <builder: 1 sah | 2 reference> <trials>.  Prints "ok <trials that built>" or the first difference.
#include <algorithm>
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

struct Desc {
    std::vector<mcpt_object> objs;
    std::vector<mcpt_triangle> tris;
    std::vector<mcpt_material> mats;
};

// n_obj random objects over their own triangle array; materials index [0, n_mat_total).  shuffle: the meshes' ranges in random order.
static void random_objects(std::mt19937 &rng, int n_obj, int n_mat_total, bool shuffle, Desc &D) {
    std::uniform_real_distribution<float> pos(-50.f, 50.f), ext(0.1f, 6.f);
    D.objs.assign((size_t)n_obj, mcpt_object{});
    for (int o = 0; o < n_obj; ++o) {
        mcpt_object &ob = D.objs[(size_t)o];
        std::memset(&ob, 0, sizeof ob);
        ob.material = (int32_t)(rng() % (unsigned)n_mat_total);
        if (rng() % 3 == 0) {
            ob.kind = MCPT_OBJ_SPHERE;
            ob.radius = ext(rng);
            for (int k = 0; k < 3; ++k) ob.center[k] = pos(rng);
        } else {
            ob.kind = MCPT_OBJ_MESH;
            ob.n_tri = 1 + (int32_t)(rng() % 40);
        }
    }
    std::vector<int> order;
    for (int o = 0; o < n_obj; ++o)
        if (D.objs[(size_t)o].kind == MCPT_OBJ_MESH) order.push_back(o);
    if (shuffle) std::shuffle(order.begin(), order.end(), rng);
    int32_t at = 0;
    for (int o : order) {
        if (shuffle && rng() % 4 == 0) at += 1 + (int32_t)(rng() % 3);  // triangles no object uses
        D.objs[(size_t)o].first_tri = at;
        at += D.objs[(size_t)o].n_tri;
    }
    D.tris.assign((size_t)at, mcpt_triangle{});
    for (mcpt_triangle &t : D.tris) {
        std::memset(&t, 0, sizeof t);
        for (int a = 0; a < 3; ++a) {
            const float b = pos(rng);
            t.v0[a] = b;
            t.v1[a] = b + ext(rng);
            t.v2[a] = b - ext(rng);
        }
        t.t0[0] = ext(rng);
        t.t1[1] = ext(rng);
        t.t2[0] = ext(rng);
    }
}

static void random_materials(std::mt19937 &rng, int n, std::vector<mcpt_material> &mats) {
    mats.assign((size_t)n, mcpt_material{});
    for (mcpt_material &m : mats) {
        std::memset(&m, 0, sizeof m);
        m.type = (int32_t)(rng() % 4);
        m.textured = (int32_t)(rng() % 2);
        m.roughness = 0.3f;
        m.iorA = 1.5f;
        if (rng() % 4 == 0) m.emission[0] = m.emission[1] = m.emission[2] = 5.f;
    }
}

static mcpt_scene_desc desc_of(const Desc &D) {
    mcpt_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_objects = (int32_t)D.objs.size();
    d.objects = D.objs.data();
    d.n_triangles = (int32_t)D.tris.size();
    d.triangles = D.tris.data();
    d.n_materials = (int32_t)D.mats.size();
    d.materials = D.mats.data();
    return d;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    BuildChoice choice;
    choice.builder = std::atoi(argv[1]);
    const int trials = std::atoi(argv[2]);
    std::mt19937 rng(11);
    int built = 0;
    for (int trial = 0; trial < trials; ++trial) {
        Desc base, add;
        const int nm0 = 1 + (int)(rng() % 3), nm1 = (int)(rng() % 3);
        random_materials(rng, nm0, base.mats);
        random_materials(rng, nm1, add.mats);
        random_objects(rng, 1 + (int)(rng() % 6), nm0, false, base);
        random_objects(rng, 1 + (int)(rng() % 4), nm0 + nm1, true, add);
        const mcpt_scene_desc d = desc_of(base);
        mcpt_scene_addition a;
        std::memset(&a, 0, sizeof a);
        a.n_objects = (int32_t)add.objs.size();
        a.objects = add.objs.data();
        a.n_triangles = (int32_t)add.tris.size();
        a.triangles = add.tris.empty() ? nullptr : add.tris.data();
        a.n_materials = nm1;
        a.materials = nm1 ? add.mats.data() : nullptr;
        const char *err = "";
        int32_t no = -1, nt = -1, nm = -1;
        if (extend_scene_desc(d, a, nullptr, nullptr, nullptr, &no, &nt, &nm, &err) != MCPT_OK) return fail_at(trial, err);
        Desc ext;  // exactly the reported sizes
        ext.objs.resize((size_t)no);
        ext.tris.resize((size_t)nt);
        ext.mats.resize((size_t)nm);
        if (extend_scene_desc(d, a, ext.objs.data(), ext.tris.data(), ext.mats.data(), &no, &nt, &nm, &err) != MCPT_OK) return fail_at(trial, "second extension");
        Desc hand = base;
        for (mcpt_object o : add.objs) {
            if (o.kind == MCPT_OBJ_MESH) o.first_tri += (int32_t)base.tris.size();
            hand.objs.push_back(o);
        }
        hand.tris.insert(hand.tris.end(), add.tris.begin(), add.tris.end());
        hand.mats.insert(hand.mats.end(), add.mats.begin(), add.mats.end());
        if (!same_bytes(ext.objs, hand.objs) || !same_bytes(ext.tris, hand.tris) || !same_bytes(ext.mats, hand.mats)) return fail_at(trial, "the extended description");
        HostScene A, B;
        const int ra = build_host_scene(desc_of(ext), A, &err, choice), rb = build_host_scene(desc_of(hand), B, &err, choice);
        if (ra != rb) return fail_at(trial, "the build's return code");
        if (ra != MCPT_OK) continue;  // (too deep, say: nothing to compare)
        ++built;
        if (A.root != B.root || A.height != B.height || A.n_triangles != B.n_triangles || A.n_objects != B.n_objects) return fail_at(trial, "tree header");
        if (!same_bytes(A.nodes, B.nodes) || !same_bytes(A.qnodes, B.qnodes)) return fail_at(trial, "tree");
        if (!same_bytes(A.tri_geom, B.tri_geom) || !same_bytes(A.tri_shade, B.tri_shade) || !same_bytes(A.spheres, B.spheres)) return fail_at(trial, "primitive records");
        if (!same_bytes(A.materials, B.materials)) return fail_at(trial, "material records");
        if (!same_bytes(A.lights, B.lights) || !same_bytes(A.light_nodes, B.light_nodes) || !same_bytes(A.light_tris, B.light_tris)) return fail_at(trial, "light tables");
        if (A.sphere_objects != B.sphere_objects) return fail_at(trial, "sphere list");
        // a refused addition writes nothing and says why
        mcpt_scene_addition bad = a;
        bad.reserved[2] = 1;
        if (extend_scene_desc(d, bad, nullptr, nullptr, nullptr, &no, &nt, &nm, &err) != MCPT_ERR_ARG || !err[0]) return fail_at(trial, "a refusal");
    }
    std::printf("ok %d\n", built);
    return 0;
}
