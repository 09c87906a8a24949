// rt_denoise / rt_denoise_device and rt_denoise_sym / rt_denoise_sym_device: the edge-aware a-trous wavelet filter, f64,
// one thread per pixel and pass; and the kernel of rt_denoised_render that turns the two accumulators of a frame into the filter's inputs.
// The tap order and every operation are fixed (include/rtamd.h, rt_denoise_config): the library is built with -ffp-contract=off and the
// filter uses only + - * / sqrt fmax, so tests/denoise_ref.py restates it bit for bit in numpy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "denoise.h"

namespace rtamd {

#define DN_CHECK(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            throw RtError((_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? RT_ERR_NO_DEVICE : RT_ERR_HIP, \
                          std::string(#expr) + ": " + hipGetErrorString(_e));                            \
    } while (0)

struct DenoiseK {
    int width, height, step;
    int npow;               // normal_power_log2
    int use_n, use_z, use_a;  // guides present and selected
    double sigma_depth, sigma_albedo, sigma_luma, eps;
};

static const int DN_BX = 16, DN_BY = 16;

// One pass at step k.step.  c_in / c_out: [H][W][3]; v_in (null: no luminance weight) / v_out (null: not written): [H][W];
// aov (null when no guide is used): [H][W][8] = {normal[3], t, albedo[3], coverage}.
// SYM (rt_denoise_sym; v_in is not null): the luminance stop of a tap is sigma_luma * sqrt(v_p + v_q) + eps, the same from p to q as from q
// to p, in place of the centre's sigma_luma * sqrt(v_p) + eps.  Nothing else differs, and SYM == false is rt_denoise's kernel as it was.
template <bool SYM>
__global__ void __launch_bounds__(DN_BX * DN_BY) atrous_kernel(DenoiseK k, const double* __restrict__ c_in, const double* __restrict__ v_in,
                                                             const double* __restrict__ aov, double* __restrict__ c_out, double* __restrict__ v_out) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= k.width || y >= k.height) return;
    const double H[3] = {0.375, 0.25, 0.0625};
    const size_t p = (size_t)y * (size_t)k.width + (size_t)x;
    const double* cp = c_in + 3 * p;
    const double lp = (0.2126 * cp[0] + 0.7152 * cp[1]) + 0.0722 * cp[2];
    const double lden = (!SYM && v_in) ? k.sigma_luma * sqrt(v_in[p]) + k.eps : 1.;
    const double vp = SYM ? v_in[p] : 0.;
    const double* gp = aov ? aov + 8 * p : nullptr;
    const double zden = k.sigma_depth * (double)k.step;
    double W = 0., C0 = 0., C1 = 0., C2 = 0., V = 0.;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + k.step * dy;
        if (qy < 0 || qy >= k.height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + k.step * dx;
            if (qx < 0 || qx >= k.width) continue;
            const size_t q = (size_t)qy * (size_t)k.width + (size_t)qx;
            const double* cq = c_in + 3 * q;
            const double h = H[dx < 0 ? -dx : dx] * H[dy < 0 ? -dy : dy];
            double w = h;
            if (dx != 0 || dy != 0) {
                double wn = 1., wz = 1., wa = 1., wl = 1.;
                const double* gq = aov ? aov + 8 * q : nullptr;
                if (k.use_n) {
                    wn = fmax(0., (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2]);
                    for (int i = 0; i < k.npow; i++) wn = wn * wn;
                }
                if (k.use_z) wz = 1. / (1. + fabs(gp[3] - gq[3]) / zden);
                if (k.use_a) wa = 1. / (1. + ((fabs(gp[4] - gq[4]) + fabs(gp[5] - gq[5])) + fabs(gp[6] - gq[6])) / k.sigma_albedo);
                if (v_in) {
                    const double lq = (0.2126 * cq[0] + 0.7152 * cq[1]) + 0.0722 * cq[2];
                    wl = 1. / (1. + fabs(lp - lq) / (SYM ? k.sigma_luma * sqrt(vp + v_in[q]) + k.eps : lden));
                }
                w = h * wn * wz * wa * wl;
            }
            W += w;
            C0 += w * cq[0];
            C1 += w * cq[1];
            C2 += w * cq[2];
            if (v_in) V += (w * w) * v_in[q];
        }
    }
    double* co = c_out + 3 * p;
    co[0] = C0 / W;
    co[1] = C1 / W;
    co[2] = C2 / W;
    if (v_out) v_out[p] = V / (W * W);
}

namespace {
struct DnBuf {
    void* p = nullptr;
    DnBuf() = default;
    DnBuf(const DnBuf&) = delete;
    DnBuf& operator=(const DnBuf&) = delete;
    ~DnBuf() {
        if (p) (void)hipFree(p);
    }
    double* alloc(size_t n) {
        DN_CHECK(hipMalloc(&p, n ? n : 16));
        return (double*)p;
    }
};
}  // namespace

template <bool SYM>
static void run_passes(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance, const double* aov,
                       double* out_rgb, double* out_variance, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const size_t npix = (size_t)width * (size_t)height;
    const int n = cfg.iterations;
    // pass i reads what pass i - 1 wrote: two scratch frames (colour, and variance when there is one) alternate, the last pass writes the outputs
    const int n_tmp = n > 2 ? 2 : n - 1;
    DnBuf tc[2], tv[2];
    for (int i = 0; i < n_tmp; i++) {
        tc[i].alloc(npix * 3 * sizeof(double));
        if (variance) tv[i].alloc(npix * sizeof(double));
    }
    DenoiseK k;
    k.width = width;
    k.height = height;
    k.npow = cfg.normal_power_log2;
    k.use_n = aov && (cfg.guides & 1);
    k.use_z = aov && (cfg.guides & 2);
    k.use_a = aov && (cfg.guides & 4);
    k.sigma_depth = cfg.sigma_depth;
    k.sigma_albedo = cfg.sigma_albedo;
    k.sigma_luma = cfg.sigma_luma;
    k.eps = cfg.eps;
    const double* g = (k.use_n || k.use_z || k.use_a) ? aov : nullptr;
    const dim3 grid((unsigned)((width + DN_BX - 1) / DN_BX), (unsigned)((height + DN_BY - 1) / DN_BY)), block(DN_BX, DN_BY);
    for (int i = 0; i < n; i++) {
        k.step = 1 << i;
        const double* c_src = i == 0 ? rgb : (const double*)tc[(i - 1) & 1].p;
        const double* v_src = !variance ? nullptr : i == 0 ? variance : (const double*)tv[(i - 1) & 1].p;
        double* c_dst = i == n - 1 ? out_rgb : (double*)tc[i & 1].p;
        double* v_dst = !variance ? nullptr : i == n - 1 ? out_variance : (double*)tv[i & 1].p;
        hipLaunchKernelGGL(atrous_kernel<SYM>, grid, block, 0, stream, k, c_src, v_src, g, c_dst, v_dst);
        DN_CHECK(hipGetLastError());
    }
    DN_CHECK(hipStreamSynchronize(stream));  // (the scratch frames are freed on return)
}

void denoise_device(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance, const double* aov,
                    double* out_rgb, double* out_variance, void* stream) {
    run_passes<false>(cfg, width, height, rgb, variance, aov, out_rgb, out_variance, stream);
}
void denoise_sym_device(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance, const double* aov,
                        double* out_rgb, double* out_variance, void* stream) {
    run_passes<true>(cfg, width, height, rgb, variance, aov, out_rgb, out_variance, stream);
}

template <bool SYM>
static void run_host(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance, const double* aov,
                     double* out_rgb, double* out_variance) {
    const size_t npix = (size_t)width * (size_t)height;
    DnBuf d_rgb, d_var, d_aov, d_out, d_out_var;
    d_rgb.alloc(npix * 3 * sizeof(double));
    d_out.alloc(npix * 3 * sizeof(double));
    DN_CHECK(hipMemcpy(d_rgb.p, rgb, npix * 3 * sizeof(double), hipMemcpyHostToDevice));
    if (variance) {
        d_var.alloc(npix * sizeof(double));
        DN_CHECK(hipMemcpy(d_var.p, variance, npix * sizeof(double), hipMemcpyHostToDevice));
    }
    if (aov) {
        d_aov.alloc(npix * 8 * sizeof(double));
        DN_CHECK(hipMemcpy(d_aov.p, aov, npix * 8 * sizeof(double), hipMemcpyHostToDevice));
    }
    if (out_variance) d_out_var.alloc(npix * sizeof(double));
    run_passes<SYM>(cfg, width, height, (const double*)d_rgb.p, (const double*)d_var.p, (const double*)d_aov.p, (double*)d_out.p,
                    (double*)d_out_var.p, nullptr);
    DN_CHECK(hipMemcpy(out_rgb, d_out.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_variance) DN_CHECK(hipMemcpy(out_variance, d_out_var.p, npix * sizeof(double), hipMemcpyDeviceToHost));
}
void denoise_host(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance, const double* aov,
                  double* out_rgb, double* out_variance) {
    run_host<false>(cfg, width, height, rgb, variance, aov, out_rgb, out_variance);
}
void denoise_sym_host(const rt_denoise_config& cfg, int width, int height, const double* rgb, const double* variance, const double* aov,
                      double* out_rgb, double* out_variance) {
    run_host<true>(cfg, width, height, rgb, variance, aov, out_rgb, out_variance);
}

// ---- rt_denoised_render: the frame's two accumulators -> the filter's inputs ----
// One thread per image pixel (row-major, as assemble_kernel walks them): its slot in the tile-major accumulators of a whole frame is
// (tile * 64 + pixel in tile) * 3.  noisy = S / spp is finalize_kernel's division; the half means divide by h = spp / 2 the same way.
__global__ void __launch_bounds__(256) split_halves_kernel(const double* __restrict__ accum, const double* __restrict__ half, double* __restrict__ noisy,
                                                           double* __restrict__ variance, int width, int height, int tiles_x, int spp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)width * height) return;
    const int x = (int)(i % width), y = (int)(i / width);
    const int64_t tile = (int64_t)(y >> 3) * tiles_x + (x >> 3);
    const int pix = ((y & 7) << 3) | (x & 7);
    const double* S = accum + (tile * TILE_PIX + pix) * 3;
    const double* Sh = half + (tile * TILE_PIX + pix) * 3;
    const double n = (double)spp, h = (double)(spp / 2);
    noisy[3 * i] = S[0] / n;
    noisy[3 * i + 1] = S[1] / n;
    noisy[3 * i + 2] = S[2] / n;
    const double a0 = Sh[0] / h, a1 = Sh[1] / h, a2 = Sh[2] / h;
    const double b0 = (S[0] - Sh[0]) / h, b1 = (S[1] - Sh[1]) / h, b2 = (S[2] - Sh[2]) / h;
    const double la = (0.2126 * a0 + 0.7152 * a1) + 0.0722 * a2;
    const double lb = (0.2126 * b0 + 0.7152 * b1) + 0.0722 * b2;
    variance[i] = ((la - lb) * (la - lb)) / 4.0;
}

void denoise_split_halves(const RenderPlan& plan, const double* accum, const double* half, double* noisy, double* variance, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n = (int64_t)plan.width * plan.height;
    hipLaunchKernelGGL(split_halves_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, accum, half, noisy, variance, plan.width,
                       plan.height, plan.tiles_x, plan.spp);
    DN_CHECK(hipGetLastError());
    DN_CHECK(hipStreamSynchronize(stream));
}

}  // namespace rtamd
