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
// (the launch decides again, by the same functions -- choose_pixel_walk of denoise.h, accel2_usable of device.h -- with the LDS of the
// device at hand)
static const size_t AO_LDS_MAX = 160 * 1024;

// rt_ao_render_device on the current device: d_out[height][width][8] is DEVICE memory, the launch goes to `stream` (a hipStream_t);
// returns after the kernel has completed on it.  kernel: 0, 1 or 2 as the caller asked (choose_pixel_walk).  cfg has been validated.
__attribute__((weak)) void render_ao_device(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel,
                                            const rt_ao_config& cfg, double* d_out, void* stream, rt_stats* st);
// rt_ao_render: the same into out_host[height][width][8] (HOST)
__attribute__((weak)) void render_ao(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel,
                                     const rt_ao_config& cfg, double* out_host, rt_stats* st);
// rt_debug_occluded_device on the current device (the arguments, the scene and the accel were checked by the caller): rays n*7 =
// {origin, direction, t_max}, out n doubles (1.0: occluded), through the device function the pass calls.  walk: 1 or 2.
__attribute__((weak)) void debug_occluded_device(const rt_scene& s, int walk, size_t n, const double* rays, double t_min, double* out);

}  // namespace rtamd
