// Host-callable interface of the guide-buffer kernel (device/aov.inc, compiled into kernels.hip) and of the a-trous filter
// (device/denoise.hip).  The declarations are WEAK: abi.cpp tests them for null, so a build of the host half alone (the sanitizer
// builds link abi.cpp against a stub of device.h) still links and loads, and the entry points report RT_ERR_NO_DEVICE there.
#pragma once
#include <cstdint>

#include "../host/scene.h"
#include "rtamd.h"

namespace rtamd {

// rt_render_aov on the current device: out_host[height][width][8] (HOST).  kernel: 0 auto, 1 reference-order walk, 2 accel walk.
__attribute__((weak)) void render_aov(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel,
                                      int aov_spp, double* out_host, rt_stats* st);
// rt_denoise_device on the current device, `stream` a hipStream_t; every pointer is DEVICE memory, variance / aov / out_variance may be
// null.  cfg has been validated.  Returns after the passes have completed on `stream`.
__attribute__((weak)) void denoise_device(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance,
                                          const double* aov, double* out_rgb, double* out_variance, void* stream);
// rt_denoise: the same on HOST buffers (copies in and out, synchronous)
__attribute__((weak)) void denoise_host(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance,
                                        const double* aov, double* out_rgb, double* out_variance);

}  // namespace rtamd
