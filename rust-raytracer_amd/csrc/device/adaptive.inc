// rt_render_adaptive (DESIGN.md s4f): the kernels between the passes of tile-adaptive sampling.  Included at the end of kernels.hip; the
// passes themselves are render_tiles over a list of active tiles (RenderPlan::tile_list) into a compact accumulator.
//
//   adaptive_copy_kernel      one block per tile, one thread per f64: gathers the active tiles' sums into the compact accumulator of a
//                             pass, scatters them back, takes the first half snapshot
//   adaptive_test_kernel      one wave per active tile, lane = pixel: the two-buffer error e_T of Dammertz et al. (WSCG 2009) in the
//                             operation order of rtamd.h, the stop flag, the half snapshot S_m := S_n of the tiles that go on
//   adaptive_finalize_kernel  finalize_kernel with the tile's own sample count as divisor

#include "adaptive.h"

namespace rtamd {

__global__ void __launch_bounds__(TILE_PIX * 3) adaptive_copy_kernel(double* __restrict__ dst, const int32_t* __restrict__ dst_list,
                                                                    const double* __restrict__ src, const int32_t* __restrict__ src_list, int64_t n) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const int64_t d = dst_list ? (int64_t)dst_list[i] : i, s = src_list ? (int64_t)src_list[i] : i;
    dst[d * (TILE_PIX * 3) + threadIdx.x] = src[s * (TILE_PIX * 3) + threadIdx.x];
}

__global__ void __launch_bounds__(TILE_PIX) adaptive_test_kernel(const double* __restrict__ accum, double* __restrict__ half,
                                                                 const int32_t* __restrict__ list, int64_t n_active, int n, int m, int width,
                                                                 int height, int tiles_x, double threshold, int32_t* __restrict__ stop,
                                                                 double* __restrict__ err) {
    __shared__ double ep[TILE_PIX];
    __shared__ int go_on;
    const int64_t i = blockIdx.x;
    if (i >= n_active) return;
    const int lane = (int)threadIdx.x;
    const int64_t tile = list[i];
    const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
    const int x = tx * TILE_W + (lane & 7), y = ty * TILE_H + (lane >> 3);
    const size_t o = ((size_t)tile * TILE_PIX + (size_t)lane) * 3;
    double e = 0.;
    if (x < width && y < height) {
        const double nn = (double)n, mm = (double)m;
        const double ir = accum[o] / nn, ig = accum[o + 1] / nn, ib = accum[o + 2] / nn;  // I = S_n / n, A = S_m / m: finalize_kernel's divisions
        const double ar = half[o] / mm, ag = half[o + 1] / mm, ab = half[o + 2] / mm;
        const double s = (ir + ig) + ib;
        e = s > 0. ? ((fabs(ir - ar) + fabs(ig - ag)) + fabs(ib - ab)) / sqrt(s) : 0.;
    }
    ep[lane] = e;
    __syncthreads();
    if (lane == 0) {  // the documented order: in-image pixels in pixel index order (row-major inside the tile), one at a time from 0.0
        const int w_in = min(TILE_W, width - tx * TILE_W), h_in = min(TILE_H, height - ty * TILE_H);
        double sum = 0.;
        for (int py = 0; py < h_in; py++)
            for (int px = 0; px < w_in; px++) sum = sum + ep[py * TILE_W + px];
        const double et = sum / (double)(w_in * h_in);
        const bool st = et < threshold;  // (a NaN error never stops a tile)
        stop[i] = st ? 1 : 0;
        err[i] = et;
        go_on = st ? 0 : 1;
    }
    __syncthreads();
    if (go_on) {
        half[o] = accum[o];
        half[o + 1] = accum[o + 1];
        half[o + 2] = accum[o + 2];
    }
}

__global__ void adaptive_finalize_kernel(const double* __restrict__ accum, const int32_t* __restrict__ tile_spp, double* __restrict__ tiles,
                                         int64_t n_pix, int width, int height, int tiles_x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const int64_t tile = i >> 6;
    const int pix = (int)(i & 63);
    const int x = (int)(tile % tiles_x) * TILE_W + (pix & 7), y = (int)(tile / tiles_x) * TILE_H + (pix >> 3);
    const bool inside = x < width && y < height;
    const double n = (double)tile_spp[tile];
    tiles[3 * i] = inside ? accum[3 * i] / n : 0.;
    tiles[3 * i + 1] = inside ? accum[3 * i + 1] / n : 0.;
    tiles[3 * i + 2] = inside ? accum[3 * i + 2] / n : 0.;
}

void adaptive_copy_tiles(double* dst, const int32_t* dst_list, const double* src, const int32_t* src_list, int64_t n, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n > 0) {
        if (n > 0x7FFFFFFF) throw RtError(RT_ERR_UNSUPPORTED, "too many tiles");
        hipLaunchKernelGGL(adaptive_copy_kernel, dim3((unsigned)n), dim3(TILE_PIX * 3), 0, stream, dst, dst_list, src, src_list, n);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream));
}

void adaptive_test(const RenderPlan& plan, const double* accum, double* half, const int32_t* list, int64_t n_active, int n, int m, double threshold,
                   int32_t* stop, double* err, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_active > 0) {
        if (n_active > 0x7FFFFFFF) throw RtError(RT_ERR_UNSUPPORTED, "too many tiles");
        hipLaunchKernelGGL(adaptive_test_kernel, dim3((unsigned)n_active), dim3(TILE_PIX), 0, stream, accum, half, list, n_active, n, m, plan.width,
                           plan.height, plan.tiles_x, threshold, stop, err);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream));
}

void adaptive_finalize(const RenderPlan& plan, const double* accum, const int32_t* tile_spp, double* tiles, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n_pix = plan.tiles_total * TILE_PIX;
    if (n_pix > 0) {
        hipLaunchKernelGGL(adaptive_finalize_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, stream, accum, tile_spp, tiles, n_pix,
                           plan.width, plan.height, plan.tiles_x);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream));
}

}  // namespace rtamd
