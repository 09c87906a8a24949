// rt_region_render (DESIGN.md s4j): the crop behind the one render_tiles launch of a region call.  Included at the end of kernels.hip; the
// launch itself is render_tiles over the sorted list of the tiles the regions touch (RenderPlan::tile_list) into a compact accumulator.
//
//   region_crop_kernel   one thread per f64 of the packed output, all regions of the call in one launch: consecutive threads write
//                        consecutive values (a region's rows are contiguous in the output, so the writes along a row coalesce, and the
//                        reads are contiguous within each 8-pixel tile row).  A thread finds its region by a binary search of the
//                        regions' first-pixel offsets and its pixel's accumulator slot by a binary search of the sorted tile list --
//                        no table the size of the frame -- and writes sum / (double)spp, finalize_kernel's division.

#include "region.h"

namespace rtamd {

__global__ void __launch_bounds__(256) region_crop_kernel(const double* __restrict__ accum, const int32_t* __restrict__ tiles, int n_tiles,
                                                          const RegionDev* __restrict__ regions, int n_regions, int64_t n_values, int tiles_x,
                                                          int spp, double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_values) return;
    const int64_t px = v / 3;
    const int c = (int)(v - px * 3);
    int lo = 0, hi = n_regions - 1;  // the last region whose first pixel is <= px (regions[0].first == 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (regions[mid].first <= px) lo = mid;
        else hi = mid - 1;
    }
    const RegionDev r = regions[lo];
    const int64_t local = px - r.first;
    const int ry = (int)(local / r.w), rx = (int)(local - (int64_t)ry * r.w);
    const int x = r.x0 + rx, y = r.y0 + ry;
    const int tile = (y >> 3) * tiles_x + (x >> 3);
    int a = 0, b = n_tiles - 1;  // the slot of `tile`: the list holds it (the host built the list from these regions); a stays inside it anyway
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (tiles[mid] < tile) a = mid + 1;
        else b = mid;
    }
    const int pix = ((y & 7) << 3) | (x & 7);
    out[v] = accum[((int64_t)a * TILE_PIX + pix) * 3 + c] / (double)spp;
}

void region_crop(const double* accum, const int32_t* tiles, int64_t n_tiles, const RegionDev* regions, int n_regions, int64_t n_values,
                 int tiles_x, int spp, double* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_values > 0) {
        const int64_t blocks = (n_values + 255) / 256;
        if (n_tiles < 1 || n_tiles > 0x7FFFFFFF || n_regions < 1 || blocks > 0x7FFFFFFF) throw RtError(RT_ERR_UNSUPPORTED, "regions too large for one crop launch");
        hipLaunchKernelGGL(region_crop_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, accum, tiles, (int)n_tiles, regions, n_regions, n_values,
                           tiles_x, spp, out);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream));
}

}  // namespace rtamd
