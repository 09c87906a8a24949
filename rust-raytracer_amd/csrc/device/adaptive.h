// Host-callable interface of the tile-adaptive sampling kernels (device/adaptive.inc, compiled into kernels.hip); render_adaptive in
// host/frame.cpp drives them between render_tiles passes.  WEAK declarations, as in device/denoise.h: a build of the host half
// alone (the sanitizer builds) still links, and the entry point reports RT_ERR_NO_DEVICE there.
#pragma once
#include <cstdint>

#include "device.h"

namespace rtamd {

// Tile copy between tile-major accumulators ([tile][64][3] f64, DEVICE memory): for i < n, tile (dst_list ? dst_list[i] : i) of dst :=
// tile (src_list ? src_list[i] : i) of src.  Lists are DEVICE int32.  Returns after the copy has completed on `stream`.
__attribute__((weak)) void adaptive_copy_tiles(double* dst, const int32_t* dst_list, const double* src, const int32_t* src_list, int64_t n,
                                               void* stream);
// The stopping test after a pass that ends at n = 2m samples, for the active tiles list[0 .. n_active) (image tiles of plan's frame,
// world 1): e_T from accum (S_n) and half (S_m), full-frame tile-major accumulators.  stop[i] = (e_T < threshold), err[i] = e_T; the
// tiles that go on get half := accum.  stop / err: DEVICE, n_active entries.  Returns after the test has completed on `stream`.
__attribute__((weak)) void adaptive_test(const RenderPlan& plan, const double* accum, double* half, const int32_t* list, int64_t n_active, int n,
                                         int m, double threshold, int32_t* stop, double* err, void* stream);
// pixel_color /= n_T: tiles = accum / tile_spp[tile] inside the image, 0 outside (finalize_tiles with a divisor per tile; world 1)
__attribute__((weak)) void adaptive_finalize(const RenderPlan& plan, const double* accum, const int32_t* tile_spp, double* tiles, void* stream);

}  // namespace rtamd
