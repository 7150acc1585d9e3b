// Sensors (include/mcpt.h: mcpt_query_radiance, mcpt_sensor_rays): a source of first rays other than the camera.  A set of n sensors is
// rendered as a frame whose pixels are the sensors: position i of the list is sensor i, the Philox key of its paths is (seed, i), and its
// samples are folded in sample order like a pixel's.  What differs is where the first ray of (sensor i, sample k) comes from: sensor_ray
// below, the one statement of it, included by the kernels that trace it (k_sensor_primary, k_sensor_primary_retrace) and by the kernel
// behind mcpt_sensor_rays (k_sensor_rays), all in csrc/mcpt_kernels.hip.
#pragma once
#include "mcpt_device.h"

namespace mcpt {

// The caller's tight arrays, in the memory of the scene's device (mcpt_sensor_buffers).
struct SensorConst {
    const float *origins;  // n*3  RAY: ray origin.  HEMISPHERE: surface point p
    const float *dirs;     // n*3  RAY: direction, used as given.  HEMISPHERE: unit normal
    int32_t kind;          // MCPT_SENSOR_*, or kSensorSphere
    int32_t indirect_only = 0;  // 1 (mcpt_query_probes_ex): a first ray whose closest hit is an emitter contributes 0 (k_sensor_primary_indirect)
};

constexpr uint32_t kSensorStream = 4u;  // Philox stream of the hemisphere and sphere samples: the channel paths use 0..2, the camera 3
constexpr uint32_t kDirectStream = 5u;  // Philox stream of the light samples of the sampled direct term (csrc/mcpt_direct.h)
// The whole-sphere source of the light probes (mcpt_query_probes, mcpt_probe_rays): internal, the public enum does not have it, and
// mcpt_query_radiance and mcpt_sensor_rays refuse it.
constexpr int32_t kSensorSphere = 2;

// The first ray of sample k (absolute: sample_offset included) of sensor i.
//   RAY         (origins[i], dirs[i]) for every k; no random numbers.
//   HEMISPHERE  a cosine-weighted direction about the normal n = dirs[i], from the offset point p + n EPSILON (Scene.cpp:114): with the
//               uniforms u of block (seed, i, k, stream 4), r = sqrt(u0), phi = 2 pi u1, local = (r cos phi, r sin phi, sqrt(1 - u0)),
//               direction = normalized(toWorld(local, n)) (Material.hpp:95-106).  The mean over k is E / pi.
//   sphere      (kSensorSphere) a uniform direction from origins[i] itself, a point in free space: with the same uniforms z = 1 - 2 u0,
//               r = sqrt(max(0, 1 - z z)), phi = 2 pi u1, direction = normalized((r cos phi, r sin phi, z)); pdf 1 / (4 pi).
// Consecutive lanes are consecutive samples of one sensor, so the six loads are broadcasts within a wave.
MCPT_DI void sensor_ray(const SensorConst &sn, uint32_t seed, uint32_t i, uint32_t k, f3 &pos, f3 &dir) {
    const size_t j = 3 * (size_t)i;
    const f3 o = mk3(sn.origins[j], sn.origins[j + 1], sn.origins[j + 2]);
    pos = o;
    if (sn.kind == kSensorSphere) {  // (sn.dirs is not read: it may be null)
        const RngKey rk{seed, i, k, kSensorStream};
        float u[4];
        rng_block(rk, 0u, 0u, u);
        const float z = 1 - 2 * u[0];
        const float r = sqrtf(fmaxf(0.f, 1 - z * z));
        float s, c;
        mcpt_sincosf(2 * kPi * u[1], &s, &c);
        dir = normalized(mk3(r * c, r * s, z));
        return;
    }
    const f3 d = mk3(sn.dirs[j], sn.dirs[j + 1], sn.dirs[j + 2]);
    dir = d;
    if (sn.kind == MCPT_SENSOR_HEMISPHERE) {
        const RngKey rk{seed, i, k, kSensorStream};
        float u[4];
        rng_block(rk, 0u, 0u, u);
        const float r = sqrtf(u[0]);
        float s, c;
        mcpt_sincosf(2 * kPi * u[1], &s, &c);
        const f3 local = mk3(r * c, r * s, sqrtf(1 - u[0]));
        dir = normalized(tan_to_world(local, d));
        pos = o + d * kEps;
    }
}

}  // namespace mcpt
