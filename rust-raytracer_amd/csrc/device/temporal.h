// Host-callable interface of the temporal accumulation step (device/temporal.hip).  The declarations are WEAK, as those of
// device/denoise.h: abi.cpp and host/frame.cpp test them for null, so a build of the host half alone still links and loads, and the
// entry points report RT_ERR_NO_DEVICE there.
#pragma once
#include <cstdint>

#include "rtamd.h"

namespace rtamd {

// rt_temporal_accumulate_device on the current device, `stream` a hipStream_t; every pointer is DEVICE memory; cam_prev, prev_history and
// prev_aov are all null on a first frame; variance / out_variance may be null.  cfg has been validated.  Returns after the kernel has
// completed on `stream`.
__attribute__((weak)) void temporal_device(const rt_temporal_config& cfg, int width, int height, const rt_camera_frame* cam_prev,
                                           const rt_camera_frame& cam_cur, const double* rgb, const double* aov, const double* variance,
                                           const double* prev_history, const double* prev_aov, double* out_history, double* out_variance,
                                           void* stream);
// rt_temporal_accumulate: the same on HOST buffers (copies in and out, synchronous)
__attribute__((weak)) void temporal_host(const rt_temporal_config& cfg, int width, int height, const rt_camera_frame* cam_prev,
                                         const rt_camera_frame& cam_cur, const double* rgb, const double* aov, const double* variance,
                                         const double* prev_history, const double* prev_aov, double* out_history, double* out_variance);
// rt_sequence_frame between the step and the filter: rgb[npix][3] = the colour of history[npix][6].  DEVICE memory; returns after the
// kernel has completed on `stream`.
__attribute__((weak)) void temporal_history_colour(int64_t npix, const double* history, double* rgb, void* stream);

}  // namespace rtamd
