// Host-callable interface of the crop kernel of rt_region_render (device/region.inc, compiled into kernels.hip); render_regions in
// host/frame.cpp calls it after ONE render_tiles over the tiles the regions touch.  A WEAK declaration, as in
// device/adaptive.h and device/denoise.h: a build of the host half alone (the sanitizer builds) still links, and the entry points report
// RT_ERR_NO_DEVICE there.
#pragma once
#include <cstdint>

#include "device.h"

namespace rtamd {

// one region as the crop kernel reads it: pixels [x0, x0 + w) x [y0, y0 + h) of the frame; `first` = the index of its first PIXEL in the
// packed output (the sum of the areas of the regions before it), so region i's values are out[3 * first ..)
struct RegionDev {
    int32_t x0, y0, w, h;
    int64_t first;
};

// out[v] for every v < n_values = 3 * (sum of the areas): value v is channel v % 3 of packed pixel v / 3, which lies in the last region
// whose `first` is <= v / 3 (regions: DEVICE, n_regions >= 1, `first` ascending from 0).  The pixel's running sum is read from
// accum ([n_tiles][64][3] f64, slot j = image tile tiles[j]; tiles: DEVICE int32, ascending, unique, holding every tile a region touches)
// and divided by (double)spp, finalize_kernel's division.  out: DEVICE.  Returns after the crop has completed on `stream`.
__attribute__((weak)) void region_crop(const double* accum, const int32_t* tiles, int64_t n_tiles, const RegionDev* regions, int n_regions,
                                       int64_t n_values, int tiles_x, int spp, double* out, void* stream);

}  // namespace rtamd
