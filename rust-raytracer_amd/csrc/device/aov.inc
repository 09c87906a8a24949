// rt_render_aov (DESIGN.md s4e): the first-hit guide buffers of the a-trous filter (device/denoise.hip).  Included at the end of
// kernels.hip, whose walks, materialize and tex_color it uses as they are; no render kernel changes.
//
// One pixel per thread.  Sample s of pixel (x, y) is pt_kernel's camera ray -- stream (seed, y * width + x, s), the same jitter and
// lens draws -- and its first hit World::hit(ray, t_min, +inf), by the reference-order walk (ACCEL false, kernel 1) or kernel 2's
// accel walk (stacks in LDS, stride blockDim.x, as hit_kernel keeps them).  GENERAL 3 is the chain walk of nested Transforms.  The hit
// record is built with uv for every primitive, as the closest-hit diagnostic builds it; the albedo is tex_color of the material's one
// texture (noise textures included: the GENERAL >= 2 form).  Sums in sample order, f64; out[pix] = {normal[3], t, albedo[3], coverage}.
// render_aov_device leaves the guides in the caller's device memory (rt_denoised_render filters them there); render_aov copies them out.

#include "denoise.h"

namespace rtamd {

template <bool ACCEL, int GENERAL>
__global__ void __launch_bounds__(64) aov_kernel(FlatView sv, CamK cam, int width, int height, uint64_t seed, double t_min, int aov_spp,
                                                 double* out, int* err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)width * (size_t)height) return;
    Acc A = make_acc(sv.base, sv.base, sv);
    uint32_t* stk = (uint32_t*)smem + threadIdx.x;
    const int x = (int)(pix % (size_t)width), y = (int)(pix / (size_t)width);
    double n0 = 0., n1 = 0., n2 = 0., tt = 0., a0 = 0., a1 = 0., a2 = 0.;
    int hits = 0;
    for (int s = 0; s < aov_spp; s++) {
        // pt_kernel's camera ray
        Rng rng;
        rng.seed_stream(seed, (uint64_t)y * (uint64_t)width + (uint64_t)x, (uint64_t)s);
        double u, st;
        D3 rd, o, d;
        camera_draw(cam, width, height, x, y, rng, u, st, rd);
        camera_ray(cam, u, st, rd, o, d);
        const Hit h = ACCEL ? traverse2<GENERAL, false, false>(A, stk, (int)blockDim.x, o, d, t_min, INFINITY) : traverse<GENERAL>(A, o, d, t_min, INFINITY);
        if (h.node < 0) continue;
        const Rec rec = materialize<GENERAL, true>(A, h, o, d, err);
        const D3 alb = tex_color<(GENERAL >= 2 ? GENERAL : 2)>(A, A.mats[rec.mat].tex, rec);
        n0 += rec.normal.x; n1 += rec.normal.y; n2 += rec.normal.z;
        tt += h.t;
        a0 += alb.x; a1 += alb.y; a2 += alb.z;
        hits++;
    }
    double* q = out + 8 * pix;
    if (hits == 0) {
        for (int k = 0; k < 8; k++) q[k] = 0.;
        return;
    }
    const double nh = (double)hits;
    q[0] = n0 / nh; q[1] = n1 / nh; q[2] = n2 / nh;
    q[3] = tt / nh;
    q[4] = a0 / nh; q[5] = a1 / nh; q[6] = a2 / nh;
    q[7] = nh / (double)aov_spp;
}

void render_aov_device(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel, int aov_spp, double* d_out,
                       void* stream_, rt_stats* st) {
    hipStream_t stream = (hipStream_t)stream_;
    aov_refuse(s);  // (before the upload: a refused scene touches no device)
    double upload_ms = 0.;
    const DeviceView dv = device_view(s, &upload_ms);
    const FlatView& view = dv.view;
    const int walk = choose_pixel_walk(s, cam, t_min, kernel, dv.di.lds_max);  // (denoise.h: rt_ao_render's chooser)
    if (walk != 1 && walk != 2) throw RtError(RT_ERR_ARG, "rt_render_aov walks with kernel 1 or 2");
    typedef void (*aov_fn)(FlatView, CamK, int, int, uint64_t, double, int, double*, int*);
    const aov_fn fn = WALK_PASS_KERNEL(aov_kernel, walk == 2, s.flat.xf_nest != 0u);
    const size_t smem = walk_pass_lds(view, walk, (const void*)fn);
    run_pixel_pass(s, "rt_render_aov", width, height, aov_spp, walk, upload_ms, stream, st, [&](unsigned blocks, int* err) {
        hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), smem, stream, view, to_camk(cam), width, height, seed, t_min, aov_spp, d_out, err);
    });
}

void render_aov(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel, int aov_spp, double* out_host,
                rt_stats* st) {
    aov_refuse(s);  // (before the allocation: a refused scene touches no device)
    const size_t npix = (size_t)width * (size_t)height;
    DevBuf dout;
    dout.alloc(npix * 8 * sizeof(double));
    render_aov_device(s, cam, width, height, seed, t_min, kernel, aov_spp, (double*)dout.p, nullptr, st);
    dout.download(out_host, npix * 8 * sizeof(double));
}

}  // namespace rtamd
