// Host-callable interface of the ambient-occlusion pass and of the any-hit diagnostic (device/ao.inc, compiled into kernels.hip;
// DESIGN.md s4k).  The declarations are WEAK, as those of device/denoise.h: abi.cpp tests them for null, so a build of the host half
// alone still links and loads, and the entry points report RT_ERR_NO_DEVICE there.
#pragma once
#include <cmath>
#include <cstdint>

#include "../host/scene.h"
#include "denoise.h"
#include "device.h"
#include "rtamd.h"

namespace rtamd {

// LDS of one workgroup on the devices this library is built for: what the entry points decide with before they touch a device
// (the launch decides again, by the same functions, with the LDS of the device at hand)
static const size_t AO_LDS_MAX = 160 * 1024;

// kernel 2's walk under render_aov_device's conditions, decided from the committed scene and the call alone: a usable accel, every ray
// origin within the region the f32 boxes were padded for (o_abs: the largest |coordinate| of an origin), t_min >= 0, and the per-lane
// stacks of a 64-lane workgroup within lds_max bytes
inline bool ao_accel_usable(const FlatView& v, double o_abs, double t_min, size_t lds_max = AO_LDS_MAX) {
    const bool origin_ok = o_abs <= v.origin_limit2 && std::isfinite(o_abs) && t_min >= 0.;
    return v.accel_ok && origin_ok && (size_t)v.stack2 * 64 * sizeof(uint32_t) <= lds_max;
}
// The one place that picks rt_ao_render's walk.  kernel: 0 (automatic), 1 or 2, checked by the caller.  Refuses rt_render_aov's scenes
// (aov_refuse) and kernel 2 without a usable accel; returns 1 or 2 (kernel 0: 2 where the accel is usable, else 1).  abi.cpp calls it
// with AO_LDS_MAX before it asks for a device, render_ao_device again with that device's LDS.
inline int ao_choose_walk(const rt_scene& s, const CameraDev& cam, double t_min, int kernel, size_t lds_max = AO_LDS_MAX) {
    aov_refuse(s);
    const double cam_abs = std::fmax(std::fmax(std::fabs(cam.origin[0]), std::fabs(cam.origin[1])), std::fabs(cam.origin[2])) + std::fabs(cam.lens_radius);
    const bool usable = ao_accel_usable(s.flat.view, cam_abs, t_min, lds_max);
    if (kernel == 2 && !usable)
        throw RtError(RT_ERR_UNSUPPORTED, "kernel 2 requested but no usable accel for this scene/camera (unbounded item, depth overflow, stacks "
                                          "larger than LDS, negative t_min, or camera farther than 64x the scene extent); use kernel 0/1");
    return kernel == 0 ? (usable ? 2 : 1) : kernel;
}

// rt_ao_render_device on the current device: d_out[height][width][8] is DEVICE memory, the launch goes to `stream` (a hipStream_t);
// returns after the kernel has completed on it.  kernel: 0, 1 or 2 as the caller asked (ao_choose_walk).  cfg has been validated.
__attribute__((weak)) void render_ao_device(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel,
                                            const rt_ao_config& cfg, double* d_out, void* stream, rt_stats* st);
// rt_ao_render: the same into out_host[height][width][8] (HOST)
__attribute__((weak)) void render_ao(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel,
                                     const rt_ao_config& cfg, double* out_host, rt_stats* st);
// rt_debug_occluded_device on the current device (the arguments, the scene and the accel were checked by the caller): rays n*7 =
// {origin, direction, t_max}, out n doubles (1.0: occluded), through the device function the pass calls.  walk: 1 or 2.
__attribute__((weak)) void debug_occluded_device(const rt_scene& s, int walk, size_t n, const double* rays, double t_min, double* out);

}  // namespace rtamd
