// Host-callable interface of the guide-buffer kernel (device/aov.inc, compiled into kernels.hip) and of the a-trous filter
// (device/denoise.hip).  The declarations are WEAK: abi.cpp tests them for null, so a build of the host half alone (the sanitizer
// builds link abi.cpp against a stub of device.h) still links and loads, and the entry points report RT_ERR_NO_DEVICE there.
#pragma once
#include <cstdint>

#include "../host/scene.h"
#include "device.h"
#include "rtamd.h"

namespace rtamd {

// what rt_render_aov does not render, decided from the committed scene alone (no device): render_aov_device refuses with these codes and
// messages, and rt_denoised_render asks before it renders the frame
inline void aov_refuse(const rt_scene& s) {
    if (!s.committed) throw RtError(RT_ERR_NOT_COMMITTED, "scene not committed");
    if (s.flat.view.kinds_mask & (1u << NK_MSPHERE))
        throw RtError(RT_ERR_UNSUPPORTED, "rt_render_aov has no ray time: scenes with moving spheres are not supported");
    if (s.flat.view.kinds_mask & (1u << NK_MEDIUM_BEGIN))
        throw RtError(RT_ERR_UNSUPPORTED, "rt_render_aov: the first hit in a scene with a ConstantMedium depends on the path's random stream (no guides through media)");
}
// The one place that picks the walk of the one-launch pixel passes (rt_render_aov, rt_ao_render; 64-lane workgroups).  kernel: 0
// (automatic), 1 or 2; any other value is handed back for the caller to refuse.  Refuses rt_render_aov's scenes (aov_refuse) and kernel 2
// without a usable accel (device.h: accel2_usable); kernel 0 becomes 2 where the accel is usable, else 1.  abi.cpp calls it with
// AO_LDS_MAX before it asks for a device, the launches again with that device's LDS.
inline int choose_pixel_walk(const rt_scene& s, const CameraDev& cam, double t_min, int kernel, size_t lds_max) {
    aov_refuse(s);
    const bool usable = accel2_usable(s.flat.view, camera_reach(cam), t_min, 64, lds_max);
    if (kernel == 2 && !usable) refuse_kernel2();
    return kernel == 0 ? (usable ? 2 : 1) : kernel;
}

// rt_render_aov on the current device: out_host[height][width][8] (HOST).  kernel: 0 auto, 1 reference-order walk, 2 accel walk.
__attribute__((weak)) void render_aov(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel,
                                      int aov_spp, double* out_host, rt_stats* st);
// the same into d_out[height][width][8], DEVICE memory of the current device, launched on `stream` (a hipStream_t); returns after the
// kernel has completed on it.  render_aov is this plus the copy to the host.
__attribute__((weak)) void render_aov_device(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min,
                                             int kernel, int aov_spp, double* d_out, void* stream, rt_stats* st);
// rt_denoise_device on the current device, `stream` a hipStream_t; every pointer is DEVICE memory, variance / aov / out_variance may be
// null.  cfg has been validated.  Returns after the passes have completed on `stream`.
__attribute__((weak)) void denoise_device(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance,
                                          const double* aov, double* out_rgb, double* out_variance, void* stream);
// rt_denoise: the same on HOST buffers (copies in and out, synchronous)
__attribute__((weak)) void denoise_host(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance,
                                        const double* aov, double* out_rgb, double* out_variance);
// rt_denoise_sym_device / rt_denoise_sym: the same two with the symmetric luminance stop sqrt(v_p + v_q); variance is not null
__attribute__((weak)) void denoise_sym_device(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance,
                                              const double* aov, double* out_rgb, double* out_variance, void* stream);
__attribute__((weak)) void denoise_sym_host(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance,
                                            const double* aov, double* out_rgb, double* out_variance);
// rt_denoised_render between the render and the filter: accum (S, the sums of all plan.spp samples) and half (S_h, their snapshot after
// plan.spp / 2), tile-major accumulators of a whole frame (world 1) -> noisy[height][width][3] = S / spp (finalize_kernel's division) and
// variance[height][width] = ((l_A - l_B) (l_A - l_B)) / 4 of the half means A = S_h / h, B = (S - S_h) / h, row-major; the pixels of edge
// tiles that lie outside the image are dropped.  DEVICE memory; returns after the kernel has completed on `stream`.
__attribute__((weak)) void denoise_split_halves(const RenderPlan& plan, const double* accum, const double* half, double* noisy, double* variance,
                                                void* stream);

}  // namespace rtamd
