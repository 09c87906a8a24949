// Host-callable launch interface of the HIP kernels (device/kernels.hip).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../common/flat.h"
#include "../host/scene.h"

namespace rtamd {

static const int TILE_W = 8, TILE_H = 8, TILE_PIX = 64;  // one 8x8 pixel tile == one wave64 of primary rays

struct RenderPlan {
    int width, height, spp, max_depth;
    double t_min;
    uint64_t seed;
    int rank, world;
    int tiles_x, tiles_y;
    int64_t tiles_total, tiles_owned;
    int spp_chunk;  // samples per pixel per launch (default: all of them)
    int sub_spp;    // samples per pixel per work unit (a wave's pool = 64 * sub_spp paths; at most 8)
    int kernel;
    int integrator;  // 0 BSDF sampling, 1 light/cosine mixture pdf, 2 SPPM final gather (needs sppm_est)
    double time0 = 0., time1 = 0.;  // D9: the camera's shutter (time1 > time0: every sample draws a time)
    const double* sppm_est = nullptr;  // device: per pixel {caustic estimate[3], global estimate[3]}
    // resumable rendering (rt_render_accumulate_device): only the sample indices [s_first, s_last) are traced (s_last < 0: spp) and folded
    // into the CALLER's accumulator (device, [tiles_owned][64][3] f64 sums; s_first == 0 initialises it); no division by spp, d_tiles unused
    int s_first = 0, s_last = -1;
    double* ext_accum = nullptr;
    // rt_render_adaptive: null, or DEVICE int32[tiles_owned] -- the image tiles this call renders, in place of the rank's
    // partition; job tile j (and slot j of ext_accum, which must be set) is image tile tile_list[j]
    const int32_t* tile_list = nullptr;
};

// Renders plan.tiles_owned tiles into d_tiles (device, tile-major f64 RGB) on `stream`; blocks until done.
// Throws RtError.
void render_tiles(const rt_scene& s, const CameraDev& cam, const RenderPlan& plan, double* d_tiles, void* stream, rt_stats* st);
// SPPMIntegrator::new + capture_image: pre-pass statistics (optional host copy, 10 f64 per pixel) and the final render
void render_sppm(const rt_scene& s, const CameraDev& cam, RenderPlan plan, const rt_sppm_config& cfg, double* d_tiles, double* stats_host,
                 void* stream, rt_stats* st, uint64_t* totals2);
void assemble_frame(const RenderPlan& plan, const double* d_gathered, int64_t tiles_per_rank_stride, double* d_frame, void* stream);
// pixel_color /= spp (camera.rs:102) of an accumulator filled by render_tiles(plan.ext_accum): d_tiles = d_accum / plan.spp inside the image, 0 outside
void finalize_tiles(const RenderPlan& plan, const double* d_accum, double* d_tiles, void* stream);
void debug_rng_device(uint64_t seed, uint64_t pixel, uint64_t sample, int n, uint64_t* out_host);
void debug_rng_floats_device(uint64_t seed, uint64_t pixel, uint64_t sample, int n, double lo, double hi, double* out_gen, double* out_range);
void debug_math_device(int op, size_t n, const double* a, const double* b, double* out);
void debug_hit_device(const rt_scene& s, int kernel, size_t n, const double* rays, double t_min, double t_max, double* out);
// env sampling diagnostics on the current device: the table as built; mode 0: n draws (in n*4 xi -> out n*4 {d, pdf}),
// mode 1: n pdfs (in n*3 directions -> out n)
void debug_env_table_device(const rt_scene& s, int* w, int* h, uint32_t* q_host);
void debug_env_eval_device(const rt_scene& s, int mode, size_t n, const double* in, double* out);
// area light diagnostics on the current device: mode 0: n draws (in n*7 {o, xi0..xi3} -> out n*4 {dir, pdf}),
// mode 1: n pdfs (in n*6 {o, d} -> out n)
void debug_area_eval_device(const rt_scene& s, int mode, size_t n, const double* in, double* out);
// shading and object-light diagnostics on the current device (the scene, the material and light indices were checked by the caller):
// shade: in n*17, keys n*3, out n*22; light eval mode 0: n draws (in n*4 {o, light}, keys n*3 -> out n*6), mode 1: n*6 {o, d} -> out n * n_lights
void debug_shade_device(const rt_scene& s, size_t n, const double* in, const uint64_t* keys, double* out);
void debug_light_eval_device(const rt_scene& s, int mode, size_t n, const double* in, const uint64_t* keys, double* out);
// SPPM gather diagnostics on the current device (device/sppm_debug.inc; the arguments were checked by the caller): one iteration of
// render_sppm's grid build, sort, gather and estimate on the caller's photon maps and gather points.  true: a unit() met a zero vector
bool debug_sppm_gather_device(rt_debug_sppm_gather& io);
// what the SPPM passes do not render, decided from the committed scene alone (no device): render_sppm and rt_debug_sppm_trace_device
// refuse with these codes and messages, in this order
inline void sppm_refuse(const rt_scene& s, bool open_shutter) {
    if (!s.committed) throw RtError(RT_ERR_NOT_COMMITTED, "scene not committed");
    if (s.flat.view.off_bg != 0u)
        throw RtError(RT_ERR_UNSUPPORTED, "SPPM does not render a scene with a background: the photon pass has no environment emitter (DESIGN.md s4g)");
    if (s.flat.view.off_area != 0u)
        throw RtError(RT_ERR_UNSUPPORTED, "SPPM does not render a scene with area lights: the photon pass has no emitter for them (DESIGN.md s4i)");
    if (s.lights.empty()) throw RtError(RT_ERR_ARG, "SPPM needs lights (rt_scene_set_lights)");
    if (s.flat.view.n_msph != 0u || s.flat.view.has_noise != 0u || open_shutter)
        throw RtError(RT_ERR_UNSUPPORTED, "the photon passes have no notion of time: the book-2 extensions (moving spheres, noise textures, an open shutter) render with integrator 0");
    if ((s.flat.view.kinds_mask & (1u << NK_MEDIUM_BEGIN)) != 0 && s.flat.light_in_medium)
        throw RtError(RT_ERR_UNSUPPORTED, "a light that lies inside the boundary of a ConstantMedium is not supported by the photon pass");
}
// SPPM trace diagnostics on the current device (device/sppm_trace_debug.inc; the arguments and sppm_refuse were checked by the caller): the
// photon pass and the eye pass of ONE iteration, through render_sppm's own light table, variant choice, launches and grow-and-retry.
// true: a unit() met a zero vector
bool debug_sppm_trace_device(const rt_scene& s, const CameraDev& cam, rt_debug_sppm_trace& io);
// closest-hit diagnostic with a ray time and a random stream per row, on the current device (device/walk_debug.inc; the arguments, the
// scene, the times and debug_walk_lds_bytes were checked by the caller): rays n*7, keys n*3, out n*14.  true: a unit() met a zero vector
bool debug_walk_device(const rt_scene& s, int kernel, size_t n, const double* rays, const uint64_t* keys, double t_min, double* out);
// ---- what the launch drivers and abi.cpp size and decide alike ----
// the stack columns of a workgroup's walks: the one place the launches, the kernels and abi.cpp size them from (kernels.hip "the stack
// discipline" has the capacity proof; host and device for the HIP compiler, plain C++ elsewhere)
#ifdef __HIPCC__
__host__ __device__
#endif
inline size_t walk_stack_bytes(uint32_t rows, uint32_t threads) { return (size_t)rows * threads * sizeof(uint32_t); }
// kernel 2's LDS node table: chunks of NODEW_CHUNK = 129 nodes, three planes of NODEW_FAR = 4128 bytes each (kernels.hip "NodeW";
// walk_debug.inc asserts the two numbers)
inline size_t nodew_bytes(const FlatView& v) { return ((size_t)v.n_nodes2 + 128) / 129 * 3 * 4128; }

// The one rule for "kernel 2's walk is usable" (DESIGN.md s4 "Kernel selection"): a usable accel, every ray origin inside the region the
// f32 boxes were padded for (flatten.cpp: origin_limit2; o_abs is the largest |coordinate| of an origin), t_min >= 0 (box32's proof), and
// the per-lane stacks of a workgroup of `lanes` threads within lds_max bytes.  abi.cpp decides with it before it touches a device, the
// launches again with the LDS of the device at hand.
inline bool accel2_usable(const FlatView& v, double o_abs, double t_min, uint32_t lanes, size_t lds_max) {
    const bool origin_ok = o_abs <= v.origin_limit2 && std::isfinite(o_abs) && t_min >= 0.;
    return v.accel_ok && origin_ok && walk_stack_bytes(v.stack2, lanes) <= lds_max;
}
// o_abs of a camera: the largest |coordinate| of a point on the lens (|lens offset| <= lens_radius on every axis)
inline double camera_reach(const CameraDev& cam) {
    return std::fmax(std::fmax(std::fabs(cam.origin[0]), std::fabs(cam.origin[1])), std::fabs(cam.origin[2])) + std::fabs(cam.lens_radius);
}
[[noreturn]] inline void refuse_kernel2() {
    throw RtError(RT_ERR_UNSUPPORTED, "kernel 2 requested but no usable accel for this scene/camera (unbounded item, depth overflow, stacks "
                                      "larger than LDS, negative t_min, or camera farther than 64x the scene extent); use kernel 0/1");
}

// dynamic LDS of debug_walk_device's launch (blocks of 64): kernel 3's NodeW table, the stack columns of kernels 2 / 3, and 64 ray times
// where the scene has moving spheres (walk_debug.inc has the map)
static const size_t DEBUG_WALK_LDS_MAX = 160 * 1024;
inline size_t debug_walk_lds_bytes(const FlatView& v, int kernel) {
    size_t b = 0;
    if (kernel == 3) b += nodew_bytes(v);
    if (kernel == 2 || kernel == 3) b += walk_stack_bytes(v.stack2, 64);
    if (v.kinds_mask & (1u << NK_MSPHERE)) b += 64 * sizeof(double) + (kernel == 1 ? 8 : 0);  // (kernel 1: the slots must not start at LDS address 0)
    return b;
}
int device_count();
// thin HIP wrappers so abi.cpp stays free of HIP headers
void* dev_alloc(size_t n);
void dev_free(void* p);
void dev_copy_to_host(void* dst, const void* src, size_t n);
void dev_copy_to_device(void* dst, const void* src, size_t n);
void dev_set_device(int d);
void free_device_copies(rt_scene& s);
size_t release_workspaces();
int dev_get_device();
void dev_synchronize();  // the current device

// ---- the exchange of the multi-device frame (device/exchange.hip: RCCL; rt_render_multi in abi.cpp drives it) ----
struct Exchange;  // communicators + one stream per device of a device list (cached per process, leased)
struct RowMove {  // `count` f64 from `src` on comm rank src_rank's device to `dst` on comm rank dst_rank's device
    int src_rank;
    const double* src;
    int dst_rank;
    double* dst;
    size_t count;
};
Exchange* exchange_open(const std::vector<int>& devices, bool* created = nullptr);  // comm rank r = devices[r] (distinct ordinals); ncclCommInitAll on first use (*created)
void exchange_close(Exchange* e, bool failed = false);     // returns the lease; the communicators stay cached -- unless an exchange on them failed: then they are destroyed
// One row: ncclSend on the source rank's communicator + the matching ncclRecv on the destination's, as one group, enqueued on the two ranks'
// exchange streams; returns without waiting.  Calls on one Exchange must not overlap (rt_render_multi's rank threads take a mutex).
void exchange_post(Exchange* e, const RowMove& move);
void exchange_wait(Exchange* e);                           // returns when every posted row has arrived
size_t exchange_release_idle();                            // destroys the idle cached communicators; returns how many sets
int exchange_library_version();                            // ncclGetVersion

}  // namespace rtamd
