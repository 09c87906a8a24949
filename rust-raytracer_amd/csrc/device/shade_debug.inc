// rt_debug_shade_device, rt_debug_light_sample_device, rt_debug_light_pdf_device (rtamd.h "diagnostics"): what a path does after its
// hit, on explicit inputs.  Included at the end of kernels.hip, whose shade, mixture_step, light_random and light_pdf_value it calls as
// the render kernels call them; no render kernel changes.  One row per thread, the scene in global memory.  unit()'s sticky flag goes
// to the row's own int of a global buffer (err + row), which the launcher copies into the row's status field.

namespace rtamd {

static const int SHADE_IN = 17, SHADE_OUT = 22, LIGHT_SAMPLE_IN = 4, LIGHT_SAMPLE_OUT = 6;

// the two 32-bit halves of the stream's next step, as exact doubles (the stream itself stays where it is)
DEV void next_draw(Rng rng, double* out2) {
    uint32_t hi, lo;
    rng.step(hi, lo);
    out2[0] = (double)hi;
    out2[1] = (double)lo;
}

template <int GENERAL>
__global__ void shade_eval_kernel(FlatView sv, size_t n, const double* __restrict__ in, const uint64_t* __restrict__ keys, double* __restrict__ out, int* err) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const Acc A = make_acc(sv.base, sv.base, sv);
    const double* x = in + SHADE_IN * k;
    double* y = out + SHADE_OUT * k;
    Rec rec;
    rec.mat = (int)x[0];  // checked by the launcher
    const D3 rdir = mk(x[5], x[6], x[7]);
    rec.p = mk(x[8], x[9], x[10]);
    rec.normal = mk(x[11], x[12], x[13]);
    rec.front_face = x[14] != 0.;
    rec.u = x[15];
    rec.v = x[16];
    Rng rng;
    rng.seed_stream(keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]);
    D3 emitted = mk(0., 0., 0.), att = mk(0., 0., 0.), out_dir = mk(0., 0., 0.);
    bool diffuse = false;
    const bool scattered = shade<GENERAL>(A, rec, rdir, rng, emitted, att, out_dir, diffuse, err + k);
    bool mixed = false, cont = false;
    D3 beta = mk(1., 1., 1.), dir = out_dir;
    if (scattered && diffuse && x[1] != 0.) {
        mixed = true;
        cont = mixture_step(A, rec, rng, att, beta, dir, err + k);
    }
    y[0] = scattered ? 1. : 0.;
    y[1] = diffuse ? 1. : 0.;
    y[2] = out_dir.x; y[3] = out_dir.y; y[4] = out_dir.z;
    y[5] = att.x; y[6] = att.y; y[7] = att.z;
    y[8] = emitted.x; y[9] = emitted.y; y[10] = emitted.z;
    y[11] = mixed ? 1. : 0.;
    y[12] = cont ? 1. : 0.;
    y[13] = beta.x; y[14] = beta.y; y[15] = beta.z;
    y[16] = dir.x; y[17] = dir.y; y[18] = dir.z;
    y[19] = 0.;  // the row's unit-zero status: the launcher's
    next_draw(rng, y + 20);
}

// mode 0: in n x {o, light index}, out n x {dir, status, next draw}; mode 1: in n x {o, d}, out n x n_lights pdfs
__global__ void light_eval_kernel(FlatView sv, int mode, size_t n, const double* __restrict__ in, const uint64_t* __restrict__ keys, double* __restrict__ out, int* err) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const Acc A = make_acc(sv.base, sv.base, sv);
    if (mode == 0) {
        const double* x = in + LIGHT_SAMPLE_IN * k;
        double* y = out + LIGHT_SAMPLE_OUT * k;
        Rng rng;
        rng.seed_stream(keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]);
        const D3 d = light_random(A, A.lights[(uint32_t)x[3]], mk(x[0], x[1], x[2]), rng, err + k);  // the index: checked by the launcher
        y[0] = d.x; y[1] = d.y; y[2] = d.z;
        y[3] = 0.;
        next_draw(rng, y + 4);
    } else {
        const double* x = in + 6 * k;
        const D3 o = mk(x[0], x[1], x[2]), d = mk(x[3], x[4], x[5]);
        for (uint32_t i = 0; i < A.n_lights; i++) out[(size_t)A.n_lights * k + i] = light_pdf_value(A, A.lights[i], o, d);
    }
}

// (the scene and the index columns were checked by abi.cpp)  Runs `launch(view, d_in, d_keys, d_out, d_err)` over n rows and folds every row's unit-zero flag into out[row * n_out + status_col]
template <class F>
static void shade_debug_run(const rt_scene& s, size_t n, const double* in, size_t n_in, const uint64_t* keys, double* out, size_t n_out, int status_col, F launch) {
    const FlatView view = device_view(s).view;
    DevBuf din, dkeys, dout, derr;
    din.upload(in, n * n_in * sizeof(double));
    if (keys) dkeys.upload(keys, n * 3 * sizeof(uint64_t));
    else dkeys.alloc(n * 3 * sizeof(uint64_t));
    dout.alloc(n * n_out * sizeof(double));
    derr.zeros(n * sizeof(int));
    launch(view, (const double*)din.p, (const uint64_t*)dkeys.p, (double*)dout.p, (int*)derr.p);
    HIP_CHECK(hipGetLastError());
    dout.download(out, n * n_out * sizeof(double));
    if (status_col >= 0) {
        std::vector<int> e(n);
        derr.download(e.data(), n * sizeof(int));
        for (size_t k = 0; k < n; k++) out[k * n_out + (size_t)status_col] = (e[k] & 1) ? 1. : 0.;
    }
}
void debug_shade_device(const rt_scene& s, size_t n, const double* in, const uint64_t* keys, double* out) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    shade_debug_run(s, n, in, SHADE_IN, keys, out, SHADE_OUT, 19, [&](const FlatView& view, const double* di, const uint64_t* dk, double* dout, int* derr) {
        if (view.has_noise) hipLaunchKernelGGL(shade_eval_kernel<2>, grid, block, 0, 0, view, n, di, dk, dout, derr);  // as render_tiles chooses
        else hipLaunchKernelGGL(shade_eval_kernel<1>, grid, block, 0, 0, view, n, di, dk, dout, derr);
    });
}
void debug_light_eval_device(const rt_scene& s, int mode, size_t n, const double* in, const uint64_t* keys, double* out) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    shade_debug_run(s, n, in, mode == 0 ? LIGHT_SAMPLE_IN : 6, mode == 0 ? keys : nullptr, out, mode == 0 ? (size_t)LIGHT_SAMPLE_OUT : (size_t)s.flat.view.n_lights,
                    mode == 0 ? 3 : -1, [&](const FlatView& view, const double* di, const uint64_t* dk, double* dout, int* derr) {
                        hipLaunchKernelGGL(light_eval_kernel, grid, block, 0, 0, view, mode, n, di, dk, dout, derr);
                    });
}

}  // namespace rtamd
