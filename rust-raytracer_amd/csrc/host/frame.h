// The frame-level host driver: what a render call does around the kernels -- the plan of a launch, the tile arithmetic of a partition,
// the device buffers of a frame and the stitch into the caller's memory, and the drivers themselves (one frame on one GPU, resumable
// rendering with host-held state, the pass loop of tile-adaptive sampling, pixel regions, the fan-out over the GPUs of a node, the SPPM
// frame).  Plain C++17: the device is reached through device/device.h, device/adaptive.h, device/region.h, device/denoise.h and device/temporal.h only.  Everything throws RtError;
// the extern "C" boundary (abi.cpp) checks its arguments, calls in here and turns exceptions into status codes.
#pragma once
#include <chrono>
#include <cstdint>

#include "device/device.h"
#include "host/scene.h"
#include "rtamd.h"

#define REQUIRE(c, msg) \
    if (!(c)) throw rtamd::RtError(RT_ERR_ARG, msg)

// rt_sequence (rtamd.h): the state a sequence of frames keeps on its device.  Nothing is allocated before the first frame.
struct rt_sequence {
    int width = 0, height = 0;
    int device = -1;  // -1 until the first frame has resolved it to the device that was current then
    rt_temporal_config cfg{};
    int frames = 0;            // since the last reset: 0 = the next frame has no previous one
    uint64_t fingerprint = 0;  // rt_scene_fingerprint of the scene of the last frame
    rt_camera_frame cam_prev{};
    int cur = 0;  // the slot of history / aov the NEXT frame writes; the other one holds the previous frame's
    // [npix][6] x 2, [npix][8] x 2 (ping-pong), then stage A's noisy [npix][3] and variance [npix], stage B's variance [npix], the
    // accumulated colour and the filtered frame [npix][3]
    double *history[2] = {nullptr, nullptr}, *aov[2] = {nullptr, nullptr}, *noisy = nullptr, *variance = nullptr, *acc_variance = nullptr,
           *accum = nullptr, *filtered = nullptr;
    rt_sequence() = default;
    rt_sequence(const rt_sequence&) = delete;
    rt_sequence& operator=(const rt_sequence&) = delete;
    ~rt_sequence();  // (host/frame.cpp: frees the buffers on their device)
};

namespace rtamd {

// ---- the tiles of a frame and of a rank's partition (rank r of `world` owns the tiles t with t % world == r) ----
int64_t tiles_total(int width, int height);
int64_t tiles_owned(int64_t total, int rank, int world);
size_t row_doubles(int64_t tiles_owned);        // f64 in a rank's tile-major rows (an accumulator state, a row of the gather): never 0
size_t frame_bytes(int width, int height);      // the stitched f64 RGB frame
uint64_t tile_pixels(const RenderPlan& pl, int64_t t);  // pixels of image tile t that lie inside the image
uint64_t pixels_in_image(const RenderPlan& pl);         // the same over the tiles of pl's rank: rt_stats.samples = this x samples per pixel

// owned >= 0: a plan for that many tiles in place of the rank's partition (render_adaptive's passes over a tile list)
RenderPlan make_plan(const rt_params* p, int64_t owned = -1);
// the plan of an SPPM call is that of its final pass under integrator 0 (render_sppm switches the integrator); spp == 0 -- the pre-pass
// alone, which never launches the render -- is planned as 1 and put back
RenderPlan make_sppm_plan(const rt_params& p);

void require_committed(const rt_scene& s);
void require_device(bool linked = true);  // linked: the weakly referenced device function of the call is there (device/adaptive.h, denoise.h)

// the clock of a call and what every render call reports at its end: rt_stats.seconds = the wall time since the clock was made
struct CallClock {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    void stamp(rt_stats* stats, uint64_t samples) const {  // the render wrote *stats itself
        if (!stats) return;
        stats->seconds = seconds();
        stats->samples = samples;
    }
    void finish(rt_stats* stats, const rt_stats& st) const {  // *stats is written on success only
        if (!stats) return;
        *stats = st;
        stats->seconds = seconds();
    }
    void finish(rt_stats* stats, const rt_stats& st, uint64_t samples) const {
        finish(stats, st);
        if (stats) stats->samples = samples;
    }
};

// rt_params.device >= 0 makes that device current for the call only: the caller's current device comes back
struct DeviceScope {
    int prev = -1;  // what the end of the scope makes current again; -1: nothing
    explicit DeviceScope(int want) {
        if (want < 0) return;
        prev = dev_get_device();
        if (prev != want) dev_set_device(want);
        else prev = -1;
    }
    ~DeviceScope() {
        if (prev < 0) return;
        try {
            dev_set_device(prev);
        } catch (...) {
        }
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// device memory of the current device, allocated and freed per call (the idle-frame pool below is render_fanout's alone)
struct DevBuf {
    void* const p;
    explicit DevBuf(size_t bytes) : p(dev_alloc(bytes)) {}
    ~DevBuf() { dev_free(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    double* f64() const { return (double*)p; }
    int32_t* i32() const { return (int32_t*)p; }
};

size_t frame_pool_release();  // frees the idle frame-sized buffers render_fanout keeps between calls; returns the bytes (rt_release_workspaces)

// rows on the device (rank-major, `stride` tiles per rank) -> the stitched frame in d_frame -> the caller's out_rgb (HOST)
void stitch_to_host(const RenderPlan& pl, const double* d_rows, int64_t stride, double* d_frame, double* out_rgb);

// ---- the drivers: each begins where its entry point's null / range checks end ----
// rt_render, rt_render_camera_frame: one frame on one GPU; world > 1 scatters only this rank's tiles into a zeroed frame
void render_frame(const rt_scene& s, const CameraDev& cd, const rt_params& p, double* out_rgb, rt_stats* stats);
// resumable rendering: the samples [begin, end) into the caller's accumulator on the device; the same with the state held by the host;
// a complete host-held state -> the frame
void accumulate_device(const rt_scene& s, const rt_camera& cam, const rt_params& p, int32_t begin, int32_t end, double* d_accum, void* stream,
                       rt_stats* stats);
void accumulate_host(const rt_scene& s, const rt_camera& cam, const rt_params& p, int32_t begin, int32_t end, double* accum_state, rt_stats* stats);
void finalize_host(const rt_params& p, const double* accum_state, double* out_rgb);
// rt_render_adaptive: the passes over the active tiles and the stopping tests between them
void render_adaptive(const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_adaptive_config& cfg, double* out_rgb,
                     int32_t* out_tile_spp, rt_stats* stats);
// rt_denoised_render(_device): the frame in two sample ranges into one accumulator with a snapshot between them, the split into the noisy
// frame and the variance, the guides (aov_spp > 0) and the filter (luma_mode 0: rt_denoise's, 1: rt_denoise_sym's), all in device memory
// (DESIGN.md s4e).  The outputs are HOST memory, or DEVICE memory of the call's device when on_device; all but out_rgb may be null.  Its
// checks begin at RT_ERR_NOT_COMMITTED / RT_ERR_UNSUPPORTED: the entry point has checked the arguments and the config.
void render_denoised(const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_denoise_config& cfg, int luma_mode, int aov_spp,
                     double* out_rgb, double* out_noisy, double* out_variance, double* out_aov, bool on_device, void* stream, rt_stats* stats);
// what rt_denoised_render refuses after its argument checks and before the device, with its codes and messages (rt_sequence_frame
// refuses the same)
void denoised_refuse(const rt_scene& s, const rt_params& p, int aov_spp);
// rt_sequence_frame: stage A = render_denoised's first three stages, stage B = the temporal step against the sequence's
// device-resident history, stage C = the filter over the accumulated colour (luma_mode -1: none).  The outputs are HOST memory; all but
// out_rgb may be null.  Its checks begin where render_denoised's do; cfg has been validated.
void sequence_frame(rt_sequence& q, const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_denoise_config& cfg, int luma_mode,
                    int aov_spp, double* out_rgb, double* out_accum, double* out_history, double* out_variance, rt_stats* stats);
// rt_region_*: pixel regions of a frame.  check_regions is the argument check all four entry points share (RT_ERR_ARG for
// a null pointer, whatever make_plan refuses, a partition, n_regions outside 1..65536, a region that is empty or leaves the frame) and
// returns the whole frame's plan; region_pixels = the pixels of the packed output (regions counted one by one); region_tile_list = the
// image tiles any region touches, ascending and unique; render_regions = one render_tiles over that list, then the crop, into
// out (HOST, or DEVICE memory of the call's device when out_on_device) -- its checks begin at RT_ERR_UNSUPPORTED
RenderPlan check_regions(const rt_params* p, int n_regions, const rt_region* regions);
int64_t region_pixels(int n_regions, const rt_region* regions);
std::vector<int32_t> region_tile_list(const RenderPlan& full, int n_regions, const rt_region* regions);
void render_regions(const rt_scene& s, const rt_camera& cam, const rt_params& p, int n_regions, const rt_region* regions, double* out,
                    bool out_on_device, void* stream, rt_stats* stats);
// rt_render_multi*, rt_render_sppm_multi (cfg: its configuration, null for the path tracer): one host thread per rank, the gather on
// device_ids[0], the stitch
void render_fanout(const rt_scene& s, const CameraDev& cd, const rt_sppm_config* cfg, const rt_params* p, int n_devices, const int* device_ids,
                   double* out_rgb, rt_stats* stats);
// rt_render_sppm: pre-pass and final render of a whole frame on one GPU
void render_sppm_frame(const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_sppm_config& cfg, double* out_rgb, double* stats_out,
                       uint64_t photons_stored[2], rt_stats* stats);

}  // namespace rtamd
