// rt_temporal_accumulate / rt_temporal_accumulate_device: one step of temporal accumulation with reprojection, f64, one
// thread per pixel; and the kernel of rt_sequence_frame that hands the accumulated colour to the filter.  Every operation and its order
// are fixed (include/rtamd.h, rt_temporal_config): the library is built with -ffp-contract=off and the step uses only + - * / floor fmin
// fmax fabs and comparisons, so tests/temporal_ref.py restates it bit for bit in numpy.  Every comparison is written so that a NaN fails
// it, and no index is formed before the value it comes from has passed its range test.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../host/scene.h"
#include "temporal.h"

namespace rtamd {

#define TP_CHECK(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            throw RtError((_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? RT_ERR_NO_DEVICE : RT_ERR_HIP, \
                          std::string(#expr) + ": " + hipGetErrorString(_e));                            \
    } while (0)

struct TemporalK {
    int width, height;
    int has_prev;  // 0: every pixel resets (cam_prev is not read, prev_history / prev_aov are null)
    double alpha, plane_tol2, normal_min, albedo_tolerance, min_weight, max_history;  // plane_tol2 = plane_tolerance * plane_tolerance
};

static const int TP_BX = 16, TP_BY = 16;

struct V3 {
    double x, y, z;
};
__device__ inline V3 v3(const double* p) { return V3{p[0], p[1], p[2]}; }
__device__ inline V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// the point at parameter t along the ray through the centre of pixel (x, y), lens ignored
__device__ inline V3 centre(const rt_camera_frame& c, int width, int height, int x, int y, double t) {
    const double u = ((double)x + 0.5) / (double)(width - 1);
    const double v = ((double)y + 0.5) / (double)(height - 1);
    const double st = 1.0 - v;
    const V3 d{((c.lower_left_corner[0] + c.horizontal[0] * u) + c.vertical[0] * st) - c.origin[0],
               ((c.lower_left_corner[1] + c.horizontal[1] * u) + c.vertical[1] * st) - c.origin[1],
               ((c.lower_left_corner[2] + c.horizontal[2] * u) + c.vertical[2] * st) - c.origin[2]};
    return V3{c.origin[0] + d.x * t, c.origin[1] + d.y * t, c.origin[2] + d.z * t};
}

// rgb [H][W][3], aov / prev_aov [H][W][8] = {normal[3], t, albedo[3], coverage}, variance (null: none) / out_variance (null: not written)
// [H][W], prev_history / out_history [H][W][6] = {r, g, b, m1, m2, n}.
__global__ void __launch_bounds__(TP_BX * TP_BY) temporal_kernel(TemporalK k, rt_camera_frame cam_prev, rt_camera_frame cam_cur,
                                                               const double* __restrict__ rgb, const double* __restrict__ aov,
                                                               const double* __restrict__ variance, const double* __restrict__ prev_history,
                                                               const double* __restrict__ prev_aov, double* __restrict__ out_history,
                                                               double* __restrict__ out_variance) {
    const int x = (int)(blockIdx.x * TP_BX + threadIdx.x), y = (int)(blockIdx.y * TP_BY + threadIdx.y);
    if (x >= k.width || y >= k.height) return;
    const size_t p = (size_t)y * (size_t)k.width + (size_t)x;
    const double c0 = rgb[3 * p], c1 = rgb[3 * p + 1], c2 = rgb[3 * p + 2];
    const double l = (0.2126 * c0 + 0.7152 * c1) + 0.0722 * c2;
    // the reset: what stays when any test below fails
    double o0 = c0, o1 = c1, o2 = c2, m1 = l, m2 = l * l, n = 1.0, a = 1.0;
    const double* g = aov + 8 * p;
    if (k.has_prev && g[7] > 0.0) {
        const V3 o_cur = v3(cam_cur.origin), o_prev = v3(cam_prev.origin), hor = v3(cam_prev.horizontal), ver = v3(cam_prev.vertical);
        const V3 P = centre(cam_cur, k.width, k.height, x, y, g[3]);
        const V3 q = sub(P, o_prev);
        const V3 D0 = sub(v3(cam_prev.lower_left_corner), o_prev);
        const V3 N0 = cross(hor, ver);
        const double s = dot(q, N0) / dot(D0, N0);
        if (s > 0.0) {
            const V3 r{q.x / s - D0.x, q.y / s - D0.y, q.z / s - D0.z};
            const double up = dot(r, hor) / dot(hor, hor);
            const double stp = dot(r, ver) / dot(ver, ver);
            const double fx = up * (double)(k.width - 1) - 0.5;
            const double fy = (1.0 - stp) * (double)(k.height - 1) - 0.5;
            if (fx > -1.0 && fx < (double)k.width && fy > -1.0 && fy < (double)k.height) {
                const double fx0 = floor(fx), fy0 = floor(fy);
                const int x0 = (int)fx0, y0 = (int)fy0;  // in [-1, width - 1], [-1, height - 1]
                const double wx = fx - fx0, wy = fy - fy0;
                const V3 reach = sub(P, o_cur);
                const double reach2 = dot(reach, reach);
                const V3 nc = v3(g);
                double Wsum = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0, A3 = 0.0, A4 = 0.0, nmin = __builtin_inf();
                for (int j = 0; j < 2; j++)
                    for (int i = 0; i < 2; i++) {
                        const int xq = x0 + i, yq = y0 + j;
                        if (xq < 0 || xq >= k.width || yq < 0 || yq >= k.height) continue;
                        const double b = (i ? wx : 1.0 - wx) * (j ? wy : 1.0 - wy);
                        if (!(b > 0.0)) continue;
                        const size_t pq = (size_t)yq * (size_t)k.width + (size_t)xq;
                        const double* h = prev_history + 6 * pq;
                        const double* gq = prev_aov + 8 * pq;
                        if (!(h[5] > 0.0) || !(gq[7] > 0.0)) continue;
                        const V3 Pq = centre(cam_prev, k.width, k.height, xq, yq, gq[3]);
                        const double dn = dot(sub(Pq, P), nc);
                        if (!(dn * dn <= k.plane_tol2 * reach2)) continue;
                        if (!(dot(nc, v3(gq)) >= k.normal_min)) continue;
                        if (!((fabs(g[4] - gq[4]) + fabs(g[5] - gq[5])) + fabs(g[6] - gq[6]) <= k.albedo_tolerance)) continue;
                        Wsum += b;
                        A0 += b * h[0];
                        A1 += b * h[1];
                        A2 += b * h[2];
                        A3 += b * h[3];
                        A4 += b * h[4];
                        nmin = fmin(nmin, h[5]);
                    }
                if (Wsum >= k.min_weight) {
                    n = fmin(nmin + 1.0, k.max_history);
                    a = fmax(k.alpha, 1.0 / n);
                    o0 = (1.0 - a) * (A0 / Wsum) + a * c0;
                    o1 = (1.0 - a) * (A1 / Wsum) + a * c1;
                    o2 = (1.0 - a) * (A2 / Wsum) + a * c2;
                    m1 = (1.0 - a) * (A3 / Wsum) + a * l;
                    m2 = (1.0 - a) * (A4 / Wsum) + a * (l * l);
                }
            }
        }
    }
    double* o = out_history + 6 * p;
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
    o[3] = m1;
    o[4] = m2;
    o[5] = n;
    if (out_variance) {
        const double Vf = (variance && n < 4.0) ? variance[p] : fmax(0.0, m2 - m1 * m1);
        out_variance[p] = Vf * a;
    }
}

void temporal_device(const rt_temporal_config& cfg, int width, int height, const rt_camera_frame* cam_prev, const rt_camera_frame& cam_cur,
                     const double* rgb, const double* aov, const double* variance, const double* prev_history, const double* prev_aov,
                     double* out_history, double* out_variance, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TemporalK k;
    k.width = width;
    k.height = height;
    k.has_prev = cam_prev != nullptr;
    k.alpha = cfg.alpha;
    k.plane_tol2 = cfg.plane_tolerance * cfg.plane_tolerance;
    k.normal_min = cfg.normal_min;
    k.albedo_tolerance = cfg.albedo_tolerance;
    k.min_weight = cfg.min_weight;
    k.max_history = (double)cfg.max_history;
    const dim3 grid((unsigned)((width + TP_BX - 1) / TP_BX), (unsigned)((height + TP_BY - 1) / TP_BY)), block(TP_BX, TP_BY);
    hipLaunchKernelGGL(temporal_kernel, grid, block, 0, stream, k, cam_prev ? *cam_prev : cam_cur, cam_cur, rgb, aov, variance, prev_history,
                       prev_aov, out_history, out_variance);
    TP_CHECK(hipGetLastError());
    TP_CHECK(hipStreamSynchronize(stream));
}

namespace {
struct TpBuf {
    void* p = nullptr;
    TpBuf() = default;
    TpBuf(const TpBuf&) = delete;
    TpBuf& operator=(const TpBuf&) = delete;
    ~TpBuf() {
        if (p) (void)hipFree(p);
    }
    double* upload(const double* host, size_t n) {  // n doubles; a null host buffer stays null on the device
        if (!host) return nullptr;
        alloc(n);
        TP_CHECK(hipMemcpy(p, host, n * sizeof(double), hipMemcpyHostToDevice));
        return (double*)p;
    }
    double* alloc(size_t n) {
        TP_CHECK(hipMalloc(&p, n * sizeof(double)));
        return (double*)p;
    }
};
}  // namespace

void temporal_host(const rt_temporal_config& cfg, int width, int height, const rt_camera_frame* cam_prev, const rt_camera_frame& cam_cur,
                   const double* rgb, const double* aov, const double* variance, const double* prev_history, const double* prev_aov,
                   double* out_history, double* out_variance) {
    const size_t npix = (size_t)width * (size_t)height;
    TpBuf d_rgb, d_aov, d_var, d_hist, d_paov, d_out, d_out_var;
    const double* rgb_d = d_rgb.upload(rgb, npix * 3);
    const double* aov_d = d_aov.upload(aov, npix * 8);
    const double* var_d = d_var.upload(variance, npix);
    const double* hist_d = d_hist.upload(prev_history, npix * 6);
    const double* paov_d = d_paov.upload(prev_aov, npix * 8);
    double* out_d = d_out.alloc(npix * 6);
    double* out_var_d = out_variance ? d_out_var.alloc(npix) : nullptr;
    temporal_device(cfg, width, height, cam_prev, cam_cur, rgb_d, aov_d, var_d, hist_d, paov_d, out_d, out_var_d, nullptr);
    TP_CHECK(hipMemcpy(out_history, out_d, npix * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_variance) TP_CHECK(hipMemcpy(out_variance, out_var_d, npix * sizeof(double), hipMemcpyDeviceToHost));
}

// ---- rt_sequence_frame: the accumulated colour of a history, as the filter reads it ----
__global__ void __launch_bounds__(256) history_colour_kernel(const double* __restrict__ history, double* __restrict__ rgb, int64_t npix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    rgb[3 * i] = history[6 * i];
    rgb[3 * i + 1] = history[6 * i + 1];
    rgb[3 * i + 2] = history[6 * i + 2];
}

void temporal_history_colour(int64_t npix, const double* history, double* rgb, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(history_colour_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, history, rgb, npix);
    TP_CHECK(hipGetLastError());
    TP_CHECK(hipStreamSynchronize(stream));
}

}  // namespace rtamd
