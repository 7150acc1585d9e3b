// CPU build of the arithmetic of specular motion (csrc/mcpt_specular_motion.h, through csrc/mcpt_temporal.h), for
// tests/test_specular_motion_cpu.py.  Compiled into a shared library with g++ -std=c++17 -O2 -ffp-contract=off; every sample goes through the
// header functions the kernel k_motion_chain calls.  With -DSPECULAR_MOTION_MAIN it is a stand-alone program that runs the same functions on
// the test shapes and on out-of-range inputs (huge, infinite and NaN planes, points and cameras): the one to build with a sanitizer.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "mcpt_temporal.h"

using namespace mcpt;

// scale and aspect as the library's camera rays have them (make_camera, csrc/mcpt_wavefront.hip)
static tp::Cam cam_of(const mcpt_camera &c) {
    tp::Cam k;
    k.width = c.width;
    k.height = c.height;
    const float half = c.fov * 0.5f;
    const float rad = (float)((double)(half * 3.141592653589793f) / 180.0);
    k.scale = (float)std::tan((double)rad);
    k.aspect = c.width / (float)c.height;
    for (int i = 0; i < 3; ++i) k.eye[i] = c.position[i];
    for (int i = 0; i < 9; ++i) k.orient[i] = c.orientation[i];
    return k;
}

// the k planes of sample s ({anchor, normal}: 6 floats each, in the order the chain meets them) composed into both maps
static void compose_sample(int k, const float *planes_cur, const float *planes_prev, float A_cur[12], float A_prev[12]) {
    for (int r = 0; r < k; ++r) tp::chain_reflect(A_cur, A_prev, r, planes_cur + 6 * r, planes_cur + 6 * r + 3, planes_prev + 6 * r, planes_prev + 6 * r + 3);
}

extern "C" {

// n samples of k reflections each (k >= 0): maps[24 s ..] = A_cur, A_prev (left as they are for k = 0), v_cur / v_prev[3 s ..] = A(q)
void sm_unfold(long long n, int k, const float *planes_cur, const float *planes_prev, const float *q_cur, const float *q_prev, float *maps, float *v_cur,
               float *v_prev) {
    for (long long s = 0; s < n; ++s) {
        float *Ac = maps + 24 * s, *Ap = Ac + 12;
        compose_sample(k, planes_cur + (size_t)s * k * 6, planes_prev + (size_t)s * k * 6, Ac, Ap);
        tp::apply_map(Ac, k, q_cur + 3 * s, v_cur + 3 * s);
        tp::apply_map(Ap, k, q_prev + 3 * s, v_prev + 3 * s);
    }
}

// ... and their motion records out[4 s ..]
void sm_motion(long long n, int k, const mcpt_camera *cam, const mcpt_camera *prev_cam, const float *planes_cur, const float *planes_prev, const float *q_cur,
               const float *q_prev, float *out) {
    const tp::Cam c = cam_of(*cam), p = cam_of(*prev_cam);
    for (long long s = 0; s < n; ++s) {
        float Ac[12], Ap[12];
        compose_sample(k, planes_cur + (size_t)s * k * 6, planes_prev + (size_t)s * k * 6, Ac, Ap);
        tp::chain_motion(c, p, Ac, Ap, k, q_cur + 3 * s, q_prev + 3 * s, out + 4 * s);
    }
}

// the unit normals of n triangle records (9 floats each: v0, e1, e2)
void sm_tri_normal(long long n, const float *geom, float *out) {
    for (long long s = 0; s < n; ++s) tp::tri_normal(geom + 9 * s, out + 3 * s);
}

// one reflect bounce on a triangle (records g_cur, g_prev, barycentrics uv) or on a sphere (hit p, normal nrm, centres) from maps that are none
void sm_reflect_tri(long long n, const float *g_cur, const float *g_prev, const float *uv, float *maps) {
    for (long long s = 0; s < n; ++s) tp::chain_reflect_tri(maps + 24 * s, maps + 24 * s + 12, 0, g_cur + 9 * s, g_prev + 9 * s, uv[2 * s], uv[2 * s + 1]);
}
void sm_reflect_sphere(long long n, const float *p, const float *nrm, const float *c_cur, const float *c_prev, float *maps) {
    for (long long s = 0; s < n; ++s) tp::chain_reflect_sphere(maps + 24 * s, maps + 24 * s + 12, 0, p + 3 * s, nrm + 3 * s, c_cur + 3 * s, c_prev + 3 * s);
}

}  // extern "C"

#ifdef SPECULAR_MOTION_MAIN
int main() {
    mcpt_camera cam{};
    cam.width = 48, cam.height = 48, cam.fov = 50.f;
    cam.position[0] = 0.f, cam.position[1] = 14.f, cam.position[2] = -28.f;
    cam.orientation[0] = cam.orientation[4] = cam.orientation[8] = 1.f;
    const float nan = std::nanf(""), inf = INFINITY;
    const float specials[] = {0.f, 1.f, -3.5f, 250.f, 1e30f, -1e30f, 3e38f, inf, -inf, nan};
    const int n_special = (int)(sizeof specials / sizeof specials[0]);
    unsigned state = 12345u;
    const auto rnd = [&]() {
        state = state * 1664525u + 1013904223u;
        return (float)(state >> 8) / (float)(1u << 24);
    };
    long long records = 0, valid = 0;
    for (int shape : {1, 15, 17 * 33}) {         // the sample counts of the test shapes (1 x 1, 3 x 5, 17 x 33)
        for (int k : {0, 1, 2, 4, 8}) {
            for (int kind = 0; kind < 2; ++kind) {  // 0: coordinates of a few hundred units; 1: out-of-range values mixed in
                const size_t n = (size_t)shape;
                std::vector<float> pc(n * (size_t)k * 6 + 1), pp(n * (size_t)k * 6 + 1), qc(n * 3), qp(n * 3), maps(n * 24), vc(n * 3), vp(n * 3), out(n * 4);
                const auto fill = [&](std::vector<float> &v) {
                    for (float &x : v) x = kind && rnd() < 0.2f ? specials[(int)(rnd() * n_special) % n_special] : (rnd() - 0.5f) * 600.f;
                };
                fill(pc), fill(pp), fill(qc), fill(qp);
                sm_unfold((long long)n, k, pc.data(), pp.data(), qc.data(), qp.data(), maps.data(), vc.data(), vp.data());
                sm_motion((long long)n, k, &cam, &cam, pc.data(), pp.data(), qc.data(), qp.data(), out.data());
                std::vector<float> g(n * 9), nrm(n * 3), uv(n * 2);
                fill(g), fill(uv);
                sm_tri_normal((long long)n, g.data(), nrm.data());
                sm_reflect_tri((long long)n, g.data(), g.data(), uv.data(), maps.data());
                sm_reflect_sphere((long long)n, qc.data(), nrm.data(), qp.data(), vc.data(), maps.data());
                std::vector<float> folded(4);
                tp::fold_pixel(out.data(), (int32_t)n, folded.data());
                records += (long long)n;
                for (size_t s = 0; s < n; ++s) valid += out[4 * s + 3] > 0.f;
            }
        }
    }
    std::printf("specular motion driver: %lld records, %lld valid\n", records, valid);
    return 0;
}
#endif
