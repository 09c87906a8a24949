// rt_debug_walk_device (rtamd.h "diagnostics"): the closest hit of explicit rays that carry what a path's segment carries -- a ray
// time and a random stream -- so that scenes with a ConstantMedium or a moving sphere, which rt_debug_hit_device refuses, can be asked
// ray by ray.  Included at the end of kernels.hip, whose traverse, traverse2, traverse2_media and materialize it calls as pt_kernel
// calls them; no render kernel changes.  One row per thread, blocks of 64, the scene's tables in global memory.
//
// Dynamic LDS of a block: [kernel 3: the NodeW table, staged as hit_kernel stages it] [kernels 2 / 3: the stack columns, stack2 x 64
// words] [scenes with moving spheres: 64 ray times, 8 bytes per lane].  Every section is a multiple of 8 bytes, so the times are
// 8-aligned.  Kernel 1 has nothing in front of the times, and LDS address 0 is what Acc::time_lds == 0 ("no moving sphere, every time is
// 0") looks like: its slots start 8 bytes in.  (pt_kernel's slots lie behind its launch constants and cannot be at 0.)
// debug_walk_lds_bytes (device.h) is this map's size: abi.cpp refuses with it, the launch allocates it.

namespace rtamd {

static_assert(NODEW_CHUNK == 129u && NODEW_FAR == 4128u, "nodew_bytes(const FlatView&) of device.h restates the kernels' nodew_bytes(n_nodes)");

// accel 1: traverse over the reference-order program; 2: the accel walk over the Node2 array in global memory (pt_kernel<false, ..>);
// 3: over the NodeW table in LDS (pt_kernel<true, ..>'s walk).  times: the scene has moving spheres.
template <int GENERAL, bool MEDIA>
__global__ void __launch_bounds__(64) walk_kernel(FlatView sv, int accel, int times, size_t n, const double* __restrict__ rays, const uint64_t* __restrict__ keys,
                                                  double t_min, double* __restrict__ out, int* err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Acc A = make_acc(sv.base, sv.base, sv);
    const uint32_t table = (accel == 3) ? nodew_bytes(sv.n_nodes2) : 0u;
    const uint32_t stacks = (accel == 1) ? 0u : (uint32_t)walk_stack_bytes(sv.stack2, 64);
    if (GENERAL >= 2 && times) {  // every lane's slot is written before any walk, an idle lane's too (ray_time reads A.time_lds + 8 * lane)
        A.time_lds = (uint32_t)(uintptr_t)(AS_L char*)(smem + table + stacks + (accel == 1 ? 8u : 0u));
        *(AS_L double*)(uintptr_t)(A.time_lds + 8u * threadIdx.x) = (i < n) ? rays[7 * i + 6] : 0.;
    }
    if (accel == 3) {
        stage_nodew(sv, smem, 0.f);  // the blob's pads, as hit_kernel's mode 3
        __syncthreads();
        A.n2w_lds = (uint32_t)(uintptr_t)(AS_L char*)smem;
    }
    if (i >= n) return;
    const D3 o = mk(rays[7 * i], rays[7 * i + 1], rays[7 * i + 2]), d = mk(rays[7 * i + 3], rays[7 * i + 4], rays[7 * i + 5]);
    uint32_t* stk = (uint32_t*)(smem + table) + threadIdx.x;
    Rng rng;
    rng.seed_stream(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]);
    Hit h;
    if (accel == 3)
        h = MEDIA ? traverse2_media<GENERAL, false, true>(A, sv.n_media, stk, 64, o, d, t_min, rng) : traverse2<GENERAL, false, false, true>(A, stk, 64, o, d, t_min, INFINITY);
    else if (accel == 2)
        h = MEDIA ? traverse2_media<GENERAL, true, false>(A, sv.n_media, stk, 64, o, d, t_min, rng) : traverse2<GENERAL, false, true, false>(A, stk, 64, o, d, t_min, INFINITY);
    else
        h = traverse<GENERAL, MEDIA>(A, o, d, t_min, INFINITY, &rng);
    double* q = out + 14 * i;
    for (int k = 0; k < 12; k++) q[k] = 0.;
    next_draw(rng, q + 12);
    if (h.node < 0) return;
    const Rec rec = materialize<GENERAL, true>(A, h, o, d, err);  // uv for every primitive, as rt_debug_hit_device
    hit_row(q, h, rec);
}

typedef void (*walk_fn)(FlatView, int, int, size_t, const double*, const uint64_t*, double, double*, int*);
static walk_fn pick_walk_kernel(int g, bool media) {
    if (g == 3) return media ? walk_kernel<3, true> : walk_kernel<3, false>;
    if (g == 2) return media ? walk_kernel<2, true> : walk_kernel<2, false>;
    if (g == 1) return media ? walk_kernel<1, true> : walk_kernel<1, false>;  // (a ConstantMedium is a kind beyond boxes and spheres: MEDIA has g >= 1)
    return walk_kernel<0, false>;
}

// (the arguments, the scene, the accel, the times and the LDS size were checked by abi.cpp)  true: a unit() met a zero vector
bool debug_walk_device(const rt_scene& s, int kernel, size_t n, const double* rays, const uint64_t* keys, double t_min, double* out) {
    const FlatView view = device_view(s).view;
    const SceneVariant variant = scene_variant(s, false);  // render_tiles' own choice, for integrator 0 and a closed shutter
    const bool moving = variant.moving;
    const walk_fn fn = pick_walk_kernel(variant.g(), variant.media);
    const size_t smem = debug_walk_lds_bytes(view, kernel);
    DevBuf dr, dk, dout, derr;
    dr.upload(rays, n * 7 * sizeof(double));
    dk.upload(keys, n * 3 * sizeof(uint64_t));
    dout.alloc(n * 14 * sizeof(double));
    derr.zeros(sizeof(int));
    set_dynamic_lds((const void*)fn, smem);
    hipLaunchKernelGGL(fn, dim3((unsigned)((n + 63) / 64)), dim3(64), smem, 0, view, kernel, moving ? 1 : 0, n, (const double*)dr.p, (const uint64_t*)dk.p, t_min,
                       (double*)dout.p, (int*)derr.p);
    HIP_CHECK(hipGetLastError());
    dout.download(out, n * 14 * sizeof(double));
    int unit_zero = 0;  // materialize's unit() met a vector of length 0 on some row: every row is written, and the call says so
    derr.download(&unit_zero, sizeof(int));
    return (unit_zero & 1) != 0;
}

}  // namespace rtamd
