// CPU build of the arithmetic of temporal reuse (csrc/mcpt_temporal.h), for tests/test_temporal_cpu.py and tests/test_gpu_temporal.py.
// Compiled into a shared library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loops mirror csrc/mcpt_temporal.hip, every pixel and
// sample through the same header functions as the kernels.
#include <cmath>
#include <cstddef>

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

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range, a null array or a bad frame size
int tp_blend(int W, int H, const float *color, const float *motion, const float *prev_color, const float *prev_depth, const float *prev_len,
             const mcpt_temporal_opts *opts, float *out_color, float *out_len) {
    tp::Opts o;
    if (!color || !motion || !prev_color || !prev_depth || !prev_len || !opts || !out_color || !out_len) return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) tp::blend_pixel(W, H, i, j, color, motion, prev_color, prev_depth, prev_len, o, out_color, out_len);
    return 0;
}

// xy[2k..]: the screen position of point k; ok[k]: 0 when q.z <= 0
void tp_project(long long n, const mcpt_camera *cam, const float *points, float *xy, int *ok) {
    const tp::Cam c = cam_of(*cam);
    for (long long k = 0; k < n; ++k) {
        float sx = 0.f, sy = 0.f;
        ok[k] = tp::project(c, points + 3 * k, sx, sy) ? 1 : 0;
        xy[2 * k] = sx;
        xy[2 * k + 1] = sy;
    }
}

void tp_sample_motion(long long n, const mcpt_camera *cam, const mcpt_camera *prev_cam, const float *p_cur, const float *p_prev, float *out) {
    const tp::Cam c = cam_of(*cam), p = cam_of(*prev_cam);
    for (long long k = 0; k < n; ++k) tp::sample_motion(c, p, p_cur + 3 * k, p_prev + 3 * k, out + 4 * k);
}

void tp_fold(long long n_pix, int spp, const float *samples, float *out) {
    for (long long m = 0; m < n_pix; ++m) tp::fold_pixel(samples + (size_t)m * spp * 4, spp, out + 4 * m);
}

}  // extern "C"
