// The frame-level host driver (host/frame.h).
#include "host/frame.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "device/adaptive.h"
#include "device/denoise.h"
#include "device/region.h"
#include "device/temporal.h"

namespace rtamd {

static int tiles_along(int pixels, int tile) { return (pixels + tile - 1) / tile; }
int64_t tiles_total(int width, int height) { return (int64_t)tiles_along(width, TILE_W) * tiles_along(height, TILE_H); }
int64_t tiles_owned(int64_t total, int rank, int world) { return (total - rank + world - 1) / world; }
size_t row_doubles(int64_t tiles_owned) { return (size_t)std::max<int64_t>(1, tiles_owned) * TILE_PIX * 3; }
size_t frame_bytes(int width, int height) { return (size_t)width * height * 3 * sizeof(double); }
uint64_t tile_pixels(const RenderPlan& pl, int64_t t) {
    const int tx = (int)(t % pl.tiles_x), ty = (int)(t / pl.tiles_x);
    return (uint64_t)std::min(TILE_W, pl.width - tx * TILE_W) * (uint64_t)std::min(TILE_H, pl.height - ty * TILE_H);
}
uint64_t pixels_in_image(const RenderPlan& pl) {
    uint64_t px = 0;
    for (int64_t lt = 0; lt < pl.tiles_owned; lt++) px += tile_pixels(pl, lt * pl.world + pl.rank);
    return px;
}

RenderPlan make_plan(const rt_params* p, int64_t owned) {
    REQUIRE(p, "null params");
    REQUIRE(p->width > 0 && p->height > 0, "width/height must be positive");
    REQUIRE(p->spp > 0, "spp must be positive");
    REQUIRE(p->max_depth >= 0, "max_depth must be >= 0");
    REQUIRE(p->world >= 1 && p->rank >= 0 && p->rank < p->world, "bad rank/world");
    REQUIRE((p->kernel >= 0 && p->kernel <= 2) || p->kernel == 5 || p->kernel == 6, "unknown kernel id (0 auto, 1, 2, 5, 6)");
    REQUIRE(p->integrator >= 0 && p->integrator <= 2, "unknown integrator id");
    REQUIRE(std::isfinite(p->time0) && std::isfinite(p->time1) && p->time1 >= p->time0, "shutter: time1 must be >= time0 and both finite");
    RenderPlan pl;
    pl.width = p->width; pl.height = p->height; pl.spp = p->spp; pl.max_depth = p->max_depth;
    pl.t_min = p->t_min; pl.seed = p->seed; pl.rank = p->rank; pl.world = p->world;
    pl.tiles_x = tiles_along(p->width, TILE_W);
    pl.tiles_y = tiles_along(p->height, TILE_H);
    pl.tiles_total = tiles_total(p->width, p->height);
    pl.tiles_owned = std::max<int64_t>(0, tiles_owned(pl.tiles_total, p->rank, p->world));
    if (owned >= 0) pl.tiles_owned = owned;
    pl.kernel = p->kernel;
    pl.integrator = p->integrator;
    pl.time0 = p->time0;
    pl.time1 = p->time1;
    // One launch renders all sample indices unless the caller splits them (rt_params.spp_chunk): samples are folded into the
    // accumulator inside the kernel, unit by unit, so no per-launch sample buffer bounds the launch size.
    int chunk = p->spp_chunk > 0 ? p->spp_chunk : p->spp;
    if (chunk > p->spp) chunk = p->spp;
    // one work unit = 64 pixels x sub_spp samples (a wave works through it with in-wave regeneration and fetches the next
    // one as soon as its pool is empty).  Many units balance the 4096 resident waves at the end of a launch: aim at
    // >= ~12 units per wave, 4 <= sub_spp <= 8 (measured on the headline workload: 4: 2144, 8: 2166, 16: 2104 Msamples/s).
    int64_t want_units = 12 * 4096;
    int64_t subs = std::max<int64_t>(1, want_units / std::max<int64_t>(1, pl.tiles_owned));
    int sub = (int)((chunk + subs - 1) / subs);
    pl.sub_spp = std::max(std::min(chunk, 4), std::min(sub, 8));
    const int tun_sub_spp = tuning().sub_spp;
    if (tun_sub_spp > 0) pl.sub_spp = std::max(1, std::min(std::min(chunk, 8), tun_sub_spp));  // rt_tuning (A/B runs)
    {   // at most 2^31 jobs per launch; 2^30 uniform units leave room for the tapered end of the schedule (host/schedule.cpp: up to
        // 1.2x as many units as a uniform cut, single-unit jobs)
        const int64_t max_chunk = (int64_t(1) << 30) / std::max<int64_t>(1, pl.tiles_owned) * pl.sub_spp;
        if (max_chunk < 1) throw RtError(RT_ERR_UNSUPPORTED, "image too large for one rank");
        if (chunk > max_chunk) chunk = (int)max_chunk;
    }
    pl.spp_chunk = chunk;
    return pl;
}
RenderPlan make_sppm_plan(const rt_params& p) {
    rt_params q = p;
    if (q.spp == 0) q.spp = 1;
    q.integrator = 0;
    RenderPlan pl = make_plan(&q);
    pl.spp = p.spp;
    return pl;
}

void require_committed(const rt_scene& s) {
    if (!s.committed) throw RtError(RT_ERR_NOT_COMMITTED, "rt_scene_commit has not been called");
}
void require_device(bool linked) {
    if (!linked || device_count() < 1) throw RtError(RT_ERR_NO_DEVICE, "no HIP device: librtamd has no CPU fallback");
}

// Frame-sized device buffers of rt_render_multi (the gathered rows, the stitched frame, the ranks' own rows) are kept between calls:
// allocating and freeing them cost every frame about a millisecond (hipFree waits for the device).  Per (device, size): at most
// FRAME_POOL_KEEP idle buffers, and FRAME_POOL_BYTES of idle buffers in all -- a host that renders many resolutions or rank counts does
// not pile up a frame per shape: beyond the cap the least recently returned buffers are freed; rt_release_workspaces frees them all.
namespace {
const size_t FRAME_POOL_KEEP = 4;
const size_t FRAME_POOL_BYTES = size_t(1) << 30;
struct IdleFrame {
    int dev;
    size_t bytes;
    void* p;
};
std::mutex g_frame_pool_mu;
std::vector<IdleFrame> g_frame_pool;  // in the order they were returned: the front is the least recently used
void* frame_pool_take(int dev, size_t bytes) {
    {
        std::lock_guard<std::mutex> g(g_frame_pool_mu);
        for (size_t i = g_frame_pool.size(); i-- > 0;)
            if (g_frame_pool[i].dev == dev && g_frame_pool[i].bytes == bytes) {
                void* p = g_frame_pool[i].p;
                g_frame_pool.erase(g_frame_pool.begin() + (ptrdiff_t)i);
                return p;
            }
    }
    return dev_alloc(bytes);  // (the caller has made `dev` current)
}
void frame_pool_give(int dev, size_t bytes, void* p) {  // the caller has made `dev` current
    std::vector<IdleFrame> drop;
    {
        std::lock_guard<std::mutex> g(g_frame_pool_mu);
        size_t same = 0, total = bytes;
        for (const IdleFrame& f : g_frame_pool) {
            same += (f.dev == dev && f.bytes == bytes) ? 1 : 0;
            total += f.bytes;
        }
        if (same >= FRAME_POOL_KEEP || bytes > FRAME_POOL_BYTES) {
            drop.push_back(IdleFrame{dev, bytes, p});
        } else {
            g_frame_pool.push_back(IdleFrame{dev, bytes, p});
            while (total > FRAME_POOL_BYTES && g_frame_pool.size() > 1) {  // evict the least recently returned
                total -= g_frame_pool.front().bytes;
                drop.push_back(g_frame_pool.front());
                g_frame_pool.erase(g_frame_pool.begin());
            }
        }
    }
    for (const IdleFrame& f : drop) {
        try {
            if (f.dev != dev) dev_set_device(f.dev);
            dev_free(f.p);
        } catch (...) {
        }
    }
    if (!drop.empty()) {
        try {
            dev_set_device(dev);
        } catch (...) {
        }
    }
}
}  // namespace
size_t frame_pool_release() {
    std::vector<IdleFrame> all;
    {
        std::lock_guard<std::mutex> g(g_frame_pool_mu);
        all.swap(g_frame_pool);
    }
    size_t freed = 0;
    for (const IdleFrame& f : all) {
        try {
            dev_set_device(f.dev);
            dev_free(f.p);
            freed += f.bytes;
        } catch (...) {
        }
    }
    return freed;
}

void stitch_to_host(const RenderPlan& pl, const double* d_rows, int64_t stride, double* d_frame, double* out_rgb) {
    assemble_frame(pl, d_rows, stride, d_frame, nullptr);
    dev_copy_to_host(out_rgb, d_frame, frame_bytes(pl.width, pl.height));
}

void render_frame(const rt_scene& s, const CameraDev& cd, const rt_params& p, double* out_rgb, rt_stats* stats) {
    require_committed(s);
    require_device();
    const CallClock clock;
    DeviceScope dev_scope(p.device);
    const RenderPlan pl = make_plan(&p);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    DevBuf tiles(row_doubles(pl.tiles_owned) * sizeof(double)), frame(frame_bytes(pl.width, pl.height));
    rt_stats st{};
    render_tiles(s, cd, pl, tiles.f64(), nullptr, &st);
    if (pl.world == 1) {
        stitch_to_host(pl, tiles.f64(), pl.tiles_owned, frame.f64(), out_rgb);
    } else {
        // only this rank's tiles: others stay 0 in the caller's frame
        std::vector<double> h((size_t)pl.tiles_owned * TILE_PIX * 3);
        dev_copy_to_host(h.data(), tiles.p, h.size() * sizeof(double));
        std::memset(out_rgb, 0, frame_bytes(pl.width, pl.height));
        for (int64_t lt = 0; lt < pl.tiles_owned; lt++) {
            int64_t t = lt * pl.world + pl.rank;
            int tx = (int)(t % pl.tiles_x), ty = (int)(t / pl.tiles_x);
            for (int pix = 0; pix < TILE_PIX; pix++) {
                int x = tx * TILE_W + (pix & 7), y = ty * TILE_H + (pix >> 3);
                if (x >= pl.width || y >= pl.height) continue;
                for (int c = 0; c < 3; c++) out_rgb[((size_t)y * pl.width + x) * 3 + c] = h[((size_t)lt * TILE_PIX + pix) * 3 + c];
            }
        }
    }
    clock.finish(stats, st, pixels_in_image(pl) * (uint64_t)pl.spp);
}

void accumulate_device(const rt_scene& s, const rt_camera& cam, const rt_params& p, int32_t begin, int32_t end, double* d_accum, void* stream,
                       rt_stats* stats) {
    require_committed(s);
    require_device();
    const CallClock clock;
    RenderPlan pl = make_plan(&p);
    REQUIRE(begin >= 0 && begin < end && end <= pl.spp, "sample range: 0 <= begin < end <= spp");
    REQUIRE(pl.integrator == 0 || pl.integrator == 1, "resumable rendering: integrators 0 and 1");
    pl.s_first = begin;
    pl.s_last = end;
    pl.ext_accum = d_accum;
    DeviceScope dev_scope(p.device);  // (d_accum and stream must belong to it)
    const CameraDev cd = make_camera(cam);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    render_tiles(s, cd, pl, nullptr, stream, stats);
    clock.stamp(stats, pixels_in_image(pl) * (uint64_t)(end - begin));
}
void accumulate_host(const rt_scene& s, const rt_camera& cam, const rt_params& p, int32_t begin, int32_t end, double* accum_state, rt_stats* stats) {
    require_device();
    const int64_t n = rt_accum_state_doubles(&p);
    REQUIRE(n > 0, "bad image size or partition");
    const size_t bytes = (size_t)n * sizeof(double);
    DeviceScope dev_scope(p.device);
    DevBuf acc(bytes);
    // the state always goes to the device: a rank that owns no tile (more ranks than tiles) launches nothing, and what comes back must
    // be what went in -- zeros at sample_begin == 0 -- not uninitialised device memory
    if (begin == 0) std::memset(accum_state, 0, bytes);
    dev_copy_to_device(acc.p, accum_state, bytes);
    accumulate_device(s, cam, p, begin, end, acc.f64(), nullptr, stats);
    dev_copy_to_host(accum_state, acc.p, bytes);
}
void finalize_host(const rt_params& p, const double* accum_state, double* out_rgb) {
    require_device();
    const RenderPlan pl = make_plan(&p);
    const size_t bytes = row_doubles(pl.tiles_owned) * sizeof(double);
    DeviceScope dev_scope(p.device);
    DevBuf acc(bytes), tiles(bytes), frame(frame_bytes(pl.width, pl.height));
    dev_copy_to_device(acc.p, accum_state, bytes);
    finalize_tiles(pl, acc.f64(), tiles.f64(), nullptr);
    stitch_to_host(pl, tiles.f64(), pl.tiles_owned, frame.f64(), out_rgb);
}

void render_adaptive(const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_adaptive_config& cfg, double* out_rgb,
                     int32_t* out_tile_spp, rt_stats* stats) {
    const RenderPlan full = make_plan(&p);
    require_committed(s);
    require_device(adaptive_test != nullptr);
    const CallClock clock;
    DeviceScope dev_scope(p.device);
    const CameraDev cd = make_camera(cam);
    const int64_t T = full.tiles_total;
    const size_t acc_bytes = (size_t)T * TILE_PIX * 3 * sizeof(double);
    // the frame's running sums S, the half snapshot S_m, a pass's compact accumulator (also the finalized tiles at the end), the active
    // list, the stop flags and errors of a test, the tiles' final spp, the frame
    DevBuf acc(acc_bytes), half(acc_bytes), compact(acc_bytes), list((size_t)T * sizeof(int32_t)), stop((size_t)T * sizeof(int32_t)),
        err((size_t)T * sizeof(double)), tile_spp((size_t)T * sizeof(int32_t)), frame(frame_bytes(full.width, full.height));
    std::vector<int32_t> active((size_t)T), n_t((size_t)T, full.spp), h_stop;
    for (int64_t t = 0; t < T; t++) active[(size_t)t] = (int32_t)t;
    rt_stats sum{};
    uint64_t samples = 0;
    bool first_pass = true;
    const int h = cfg.min_spp / 2;
    // passes [0, h), [h, 2h), [2h, 4h), ... capped at spp; a test after every pass that ends at n = 2m < spp
    for (int begin = 0, end = h; begin < full.spp && !active.empty(); begin = end, end = (int)std::min<int64_t>((int64_t)end * 2, full.spp)) {
        const int64_t na = (int64_t)active.size();
        dev_copy_to_device(list.p, active.data(), (size_t)na * sizeof(int32_t));
        if (begin > 0) adaptive_copy_tiles(compact.f64(), nullptr, acc.f64(), list.i32(), na, nullptr);
        RenderPlan pl = make_plan(&p, na);
        pl.s_first = begin;
        pl.s_last = end;
        pl.ext_accum = compact.f64();
        pl.tile_list = list.i32();
        rt_stats st{};
        render_tiles(s, cd, pl, nullptr, nullptr, &st);
        adaptive_copy_tiles(acc.f64(), list.i32(), compact.f64(), nullptr, na, nullptr);
        for (int32_t t : active) samples += tile_pixels(full, t) * (uint64_t)(end - begin);
        if (first_pass) {
            sum = st;
            first_pass = false;
        } else {
            sum.kernel_ms += st.kernel_ms;
            sum.launches += st.launches;
        }
        if (begin == 0) {  // S_h: the first half snapshot, every tile
            adaptive_copy_tiles(half.f64(), nullptr, acc.f64(), nullptr, T, nullptr);
        } else if (end < full.spp) {
            adaptive_test(full, acc.f64(), half.f64(), list.i32(), na, end, end / 2, cfg.threshold, stop.i32(), err.f64(), nullptr);
            h_stop.resize((size_t)na);
            dev_copy_to_host(h_stop.data(), stop.p, (size_t)na * sizeof(int32_t));
            std::vector<int32_t> next;
            for (int64_t i = 0; i < na; i++) {
                if (h_stop[(size_t)i]) n_t[(size_t)active[(size_t)i]] = end;
                else next.push_back(active[(size_t)i]);
            }
            active.swap(next);
        }
    }
    dev_copy_to_device(tile_spp.p, n_t.data(), (size_t)T * sizeof(int32_t));
    adaptive_finalize(full, acc.f64(), tile_spp.i32(), compact.f64(), nullptr);
    stitch_to_host(full, compact.f64(), T, frame.f64(), out_rgb);
    if (out_tile_spp) std::memcpy(out_tile_spp, n_t.data(), (size_t)T * sizeof(int32_t));
    clock.finish(stats, sum, samples);
}

// ---- one call from scene to clean frame ----
void denoised_refuse(const rt_scene& s, const rt_params& p, int aov_spp) {
    require_committed(s);
    if (p.kernel == 6 || p.integrator == 2)
        throw RtError(RT_ERR_UNSUPPORTED, "rt_denoised_render runs with kernels 0 / 1 / 2 / 5 and integrators 0 / 1 (those of rt_render_accumulate_device)");
    if (aov_spp > 0) aov_refuse(s);  // (before the frame is rendered; such scenes pass aov_spp = 0)
}
static bool denoised_linked() {
    return adaptive_copy_tiles != nullptr && denoise_split_halves != nullptr && render_aov_device != nullptr && denoise_device != nullptr &&
           denoise_sym_device != nullptr;
}
// The first three stages of rt_denoised_render on the current device: the frame in two sample ranges into one accumulator with a snapshot
// between them, the split into d_noisy and d_var, and the guides into d_aov (aov_spp > 0).  Returns the stats of the two ranges.
static rt_stats render_noisy_stage(const rt_scene& s, const CameraDev& cd, const rt_params& p, RenderPlan pl, int aov_spp, double* d_noisy,
                                   double* d_var, double* d_aov, void* stream) {
    const size_t acc_bytes = row_doubles(pl.tiles_total) * sizeof(double);
    DevBuf acc(acc_bytes), half(acc_bytes);  // the running sums S and their snapshot S_h after the first half
    const int h = pl.spp / 2;
    rt_stats sum{};
    for (int range = 0; range < 2; range++) {
        pl.s_first = range == 0 ? 0 : h;
        pl.s_last = range == 0 ? h : pl.spp;
        pl.ext_accum = acc.f64();
        rt_stats st{};
        render_tiles(s, cd, pl, nullptr, stream, &st);
        if (range == 0) {
            sum = st;
            adaptive_copy_tiles(half.f64(), nullptr, acc.f64(), nullptr, pl.tiles_total, stream);  // S_h
        } else {
            sum.kernel_ms += st.kernel_ms;
            sum.launches += st.launches;
        }
    }
    denoise_split_halves(pl, acc.f64(), half.f64(), d_noisy, d_var, stream);
    if (aov_spp > 0)
        render_aov_device(s, cd, pl.width, pl.height, pl.seed, pl.t_min, (p.kernel == 1 || p.kernel == 2) ? p.kernel : 0, aov_spp, d_aov, stream, nullptr);
    return sum;
}

void render_denoised(const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_denoise_config& cfg, int luma_mode, int aov_spp,
                     double* out_rgb, double* out_noisy, double* out_variance, double* out_aov, bool on_device, void* stream, rt_stats* stats) {
    const RenderPlan pl = make_plan(&p);
    denoised_refuse(s, p, aov_spp);
    require_device(denoised_linked());
    const CallClock clock;
    DeviceScope dev_scope(p.device);  // (device outputs and the stream must belong to it)
    const CameraDev cd = make_camera(cam);
    const size_t npix = (size_t)pl.width * (size_t)pl.height;
    // whatever the caller did not give device memory for
    DevBuf own_rgb(on_device ? 16 : npix * 3 * sizeof(double)), own_noisy((on_device && out_noisy) ? 16 : npix * 3 * sizeof(double)),
        own_var((on_device && out_variance) ? 16 : npix * sizeof(double)),
        own_aov((aov_spp == 0 || (on_device && out_aov)) ? 16 : npix * 8 * sizeof(double));
    double* d_rgb = on_device ? out_rgb : own_rgb.f64();
    double* d_noisy = (on_device && out_noisy) ? out_noisy : own_noisy.f64();
    double* d_var = (on_device && out_variance) ? out_variance : own_var.f64();
    double* d_aov = aov_spp == 0 ? nullptr : (on_device && out_aov) ? out_aov : own_aov.f64();
    const rt_stats sum = render_noisy_stage(s, cd, p, pl, aov_spp, d_noisy, d_var, d_aov, stream);
    (luma_mode == 1 ? denoise_sym_device : denoise_device)(cfg, pl.width, pl.height, d_noisy, d_var, d_aov, d_rgb, nullptr, stream);
    if (!on_device) {
        dev_copy_to_host(out_rgb, d_rgb, npix * 3 * sizeof(double));
        if (out_noisy) dev_copy_to_host(out_noisy, d_noisy, npix * 3 * sizeof(double));
        if (out_variance) dev_copy_to_host(out_variance, d_var, npix * sizeof(double));
        if (out_aov) dev_copy_to_host(out_aov, d_aov, npix * 8 * sizeof(double));
    }
    clock.finish(stats, sum, pixels_in_image(pl) * (uint64_t)pl.spp);
}

// ---- a device-resident sequence of frames with temporal accumulation ----
}  // namespace rtamd
rt_sequence::~rt_sequence() {
    if (!history[0]) return;  // (nothing was allocated: no frame ran)
    try {
        rtamd::DeviceScope dev_scope(device);
        for (double* b : {history[0], history[1], aov[0], aov[1], noisy, variance, acc_variance, accum, filtered})
            if (b) rtamd::dev_free(b);
    } catch (...) {
    }
}
namespace rtamd {
static rt_camera_frame camera_frame_of(const CameraDev& d) {
    rt_camera_frame f;
    for (int i = 0; i < 3; i++) {
        f.origin[i] = d.origin[i]; f.lower_left_corner[i] = d.llc[i]; f.horizontal[i] = d.horizontal[i];
        f.vertical[i] = d.vertical[i]; f.u[i] = d.u[i]; f.v[i] = d.v[i]; f.w[i] = d.w[i];
    }
    f.lens_radius = d.lens_radius;
    return f;
}
void sequence_frame(rt_sequence& q, const rt_scene& s, const rt_camera& cam, const rt_params& p_in, const rt_denoise_config& cfg, int luma_mode,
                    int aov_spp, double* out_rgb, double* out_accum, double* out_history, double* out_variance, rt_stats* stats) {
    const RenderPlan pl = make_plan(&p_in);
    denoised_refuse(s, p_in, aov_spp);
    require_device(denoised_linked() && temporal_device != nullptr && temporal_history_colour != nullptr);
    const CallClock clock;
    if (q.device < 0) q.device = dev_get_device();
    rt_params p = p_in;
    p.device = q.device;
    DeviceScope dev_scope(q.device);
    const size_t npix = (size_t)q.width * (size_t)q.height;
    if (!q.history[0]) {  // the first frame of the sequence: its buffers, all or none
        double* b[9] = {};
        const size_t doubles[9] = {6, 6, 8, 8, 3, 1, 1, 3, 3};
        try {
            for (int i = 0; i < 9; i++) b[i] = (double*)dev_alloc(npix * doubles[i] * sizeof(double));
        } catch (...) {
            for (double* x : b)
                if (x) dev_free(x);
            throw;
        }
        q.history[0] = b[0]; q.history[1] = b[1]; q.aov[0] = b[2]; q.aov[1] = b[3];
        q.noisy = b[4]; q.variance = b[5]; q.acc_variance = b[6]; q.accum = b[7]; q.filtered = b[8];
    }
    const uint64_t fp = rt_scene_fingerprint(&s);
    if (fp != q.fingerprint) q.frames = 0;  // another scene: its surfaces are not those the history saw
    const CameraDev cd = make_camera(cam);
    const rt_camera_frame cam_cur = camera_frame_of(cd);
    const int cur = q.cur, prev = cur ^ 1;
    const bool first = q.frames == 0;
    const rt_stats sum = render_noisy_stage(s, cd, p, pl, aov_spp, q.noisy, q.variance, q.aov[cur], nullptr);
    temporal_device(q.cfg, q.width, q.height, first ? nullptr : &q.cam_prev, cam_cur, q.noisy, q.aov[cur], q.variance, first ? nullptr : q.history[prev],
                    first ? nullptr : q.aov[prev], q.history[cur], q.acc_variance, nullptr);
    temporal_history_colour((int64_t)npix, q.history[cur], q.accum, nullptr);
    const double* d_rgb = q.accum;
    if (luma_mode >= 0) {
        (luma_mode == 1 ? denoise_sym_device : denoise_device)(cfg, q.width, q.height, q.accum, q.acc_variance, q.aov[cur], q.filtered, nullptr, nullptr);
        d_rgb = q.filtered;
    }
    dev_copy_to_host(out_rgb, d_rgb, npix * 3 * sizeof(double));
    if (out_accum) dev_copy_to_host(out_accum, q.accum, npix * 3 * sizeof(double));
    if (out_history) dev_copy_to_host(out_history, q.history[cur], npix * 6 * sizeof(double));
    if (out_variance) dev_copy_to_host(out_variance, q.acc_variance, npix * sizeof(double));
    // the frame is complete: only now does it become the sequence's previous one (a throw above leaves the last good state)
    q.cam_prev = cam_cur;
    q.fingerprint = fp;
    q.cur = prev;
    if (q.frames < INT32_MAX) q.frames++;
    clock.finish(stats, sum, pixels_in_image(pl) * (uint64_t)pl.spp);
}

// ---- pixel regions of a frame ----
RenderPlan check_regions(const rt_params* p, int n_regions, const rt_region* regions) {
    REQUIRE(p && regions, "null argument");
    const RenderPlan full = make_plan(p);
    REQUIRE(p->world == 1 && p->rank == 0, "rt_region_* cuts regions out of a whole frame: world must be 1 and rank 0");
    REQUIRE(full.tiles_total <= 0x7FFFFFFF, "frame too large: more than 2^31 - 1 tiles");
    REQUIRE(n_regions >= 1 && n_regions <= 65536, "n_regions must be 1..65536");
    for (int i = 0; i < n_regions; i++) {
        const rt_region& r = regions[i];
        if (!(0 <= r.x0 && r.x0 < r.x1 && r.x1 <= p->width && 0 <= r.y0 && r.y0 < r.y1 && r.y1 <= p->height))
            throw RtError(RT_ERR_ARG, "region " + std::to_string(i) + " = (" + std::to_string(r.x0) + ", " + std::to_string(r.y0) + ", " + std::to_string(r.x1) +
                                          ", " + std::to_string(r.y1) + ") must satisfy 0 <= x0 < x1 <= width = " + std::to_string(p->width) +
                                          " and 0 <= y0 < y1 <= height = " + std::to_string(p->height));
    }
    return full;
}
int64_t region_pixels(int n_regions, const rt_region* regions) {
    const int64_t limit = INT64_MAX / (3 * (int64_t)sizeof(double));  // the packed output's size in bytes stays an int64
    int64_t px = 0;
    for (int i = 0; i < n_regions; i++) {
        const int64_t area = (int64_t)(regions[i].x1 - regions[i].x0) * (regions[i].y1 - regions[i].y0);
        if (area > limit - px) throw RtError(RT_ERR_UNSUPPORTED, "regions too large: the packed output exceeds 2^63 bytes");
        px += area;
    }
    return px;
}
std::vector<int32_t> region_tile_list(const RenderPlan& full, int n_regions, const rt_region* regions) {
    std::vector<bool> touched((size_t)full.tiles_total, false);
    for (int i = 0; i < n_regions; i++) {
        const rt_region& r = regions[i];
        for (int ty = r.y0 / TILE_H; ty <= (r.y1 - 1) / TILE_H; ty++)
            for (int tx = r.x0 / TILE_W; tx <= (r.x1 - 1) / TILE_W; tx++) touched[(size_t)ty * full.tiles_x + tx] = true;
    }
    std::vector<int32_t> list;
    for (int64_t t = 0; t < full.tiles_total; t++)
        if (touched[(size_t)t]) list.push_back((int32_t)t);
    return list;
}
void render_regions(const rt_scene& s, const rt_camera& cam, const rt_params& p, int n_regions, const rt_region* regions, double* out,
                    bool out_on_device, void* stream, rt_stats* stats) {
    if (p.kernel == 6 || p.integrator == 2) throw RtError(RT_ERR_UNSUPPORTED, "rt_region_render runs with kernels 0 / 1 / 2 / 5 and integrators 0 / 1");
    require_committed(s);
    require_device(region_crop != nullptr);
    const CallClock clock;
    DeviceScope dev_scope(p.device);  // (a device output and the stream must belong to it)
    const RenderPlan full = make_plan(&p);
    const CameraDev cd = make_camera(cam);
    const std::vector<int32_t> tiles = region_tile_list(full, n_regions, regions);
    const int64_t n_tiles = (int64_t)tiles.size();
    std::vector<RegionDev> table((size_t)n_regions);
    int64_t first = 0;
    for (int i = 0; i < n_regions; i++) {
        const rt_region& r = regions[i];
        table[(size_t)i] = RegionDev{r.x0, r.y0, r.x1 - r.x0, r.y1 - r.y0, first};
        first += (int64_t)(r.x1 - r.x0) * (r.y1 - r.y0);
    }
    const int64_t n_values = 3 * region_pixels(n_regions, regions);
    uint64_t traced = 0;
    for (int32_t t : tiles) traced += tile_pixels(full, t);
    // the tile list, the regions, the compact accumulator [n_tiles][64][3] of the one launch and, for a host caller, the packed output
    DevBuf list((size_t)n_tiles * sizeof(int32_t)), regs(table.size() * sizeof(RegionDev)), compact((size_t)n_tiles * TILE_PIX * 3 * sizeof(double)),
        packed(out_on_device ? 16 : (size_t)n_values * sizeof(double));
    dev_copy_to_device(list.p, tiles.data(), (size_t)n_tiles * sizeof(int32_t));
    dev_copy_to_device(regs.p, table.data(), table.size() * sizeof(RegionDev));
    RenderPlan pl = make_plan(&p, n_tiles);
    pl.s_first = 0;
    pl.s_last = full.spp;
    pl.ext_accum = compact.f64();
    pl.tile_list = list.i32();
    rt_stats st{};
    render_tiles(s, cd, pl, nullptr, stream, &st);
    double* d_out = out_on_device ? out : packed.f64();
    region_crop(compact.f64(), list.i32(), n_tiles, (const RegionDev*)regs.p, n_regions, n_values, full.tiles_x, full.spp, d_out, stream);
    if (!out_on_device) dev_copy_to_host(out, packed.p, (size_t)n_values * sizeof(double));
    clock.finish(stats, st, traced * (uint64_t)full.spp);
}

// ---- the frame across the GPUs of one node (camera.rs:74-126 has the fan-out and the stitch inside capture_image) ----
namespace {
struct DevMem {  // device memory that remembers which device it lives on
    void* p = nullptr;
    int device = -1;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    size_t size = 0;
    void alloc(int dev, size_t bytes) {
        dev_set_device(dev);
        p = frame_pool_take(dev, bytes);
        device = dev;
        size = bytes;
    }
    ~DevMem() {
        if (!p) return;
        try {
            dev_set_device(device);
            frame_pool_give(device, size, p);
        } catch (...) {
        }
    }
};
struct ExchangeLease {
    Exchange* e = nullptr;
    bool failed = false;  // an exchange call threw: the communicators are destroyed instead of going back into the cache
    ~ExchangeLease() { exchange_close(e, failed); }
};
}  // namespace

// Every rank renders its tiles (render_tiles, or render_sppm where cfg is given) on its own host thread with the rank's device current,
// into rows on that device.
void render_fanout(const rt_scene& s, const CameraDev& cd, const rt_sppm_config* cfg, const rt_params* p, int n_devices, const int* device_ids,
                   double* out_rgb, rt_stats* stats) {
    REQUIRE(p && out_rgb, "null argument");
    REQUIRE(p->world == 1 && p->rank == 0, "rt_render_multi partitions the frame itself: rank / world must be 0 / 1");
    const int visible = device_count();
    if (visible < 1) throw RtError(RT_ERR_NO_DEVICE, "no HIP device: librtamd has no CPU fallback");
    REQUIRE(n_devices >= 0 && n_devices <= 4096, "n_devices out of range");
    const int n = n_devices == 0 ? visible : n_devices;
    std::vector<int> ids((size_t)n);
    for (int i = 0; i < n; i++) {
        ids[(size_t)i] = device_ids ? device_ids[i] : i;
        if (ids[(size_t)i] < 0 || ids[(size_t)i] >= visible)
            throw RtError(RT_ERR_NO_DEVICE, "device ordinal " + std::to_string(ids[(size_t)i]) + " of rank " + std::to_string(i) + " is not visible (" +
                                                std::to_string(visible) + " device(s))");
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(t - t0).count(); };
    DeviceScope restore(-1);  // nothing is made current here (the rank threads and the buffers pick their devices) ...
    restore.prev = dev_get_device();  // ... and whatever they leave, the caller's device comes back
    const bool force = tuning().multi_force_rccl != 0;
    const int root = ids[0];
    std::vector<RenderPlan> plans((size_t)n);
    for (int i = 0; i < n; i++) {
        rt_params q = *p;
        q.rank = i;
        q.world = n;
        q.device = -1;
        plans[(size_t)i] = cfg ? make_sppm_plan(q) : make_plan(&q);  // (as rt_render_sppm_tiles_device plans it)
    }
    const int64_t stride = plans[0].tiles_owned;  // rank 0 owns the most tiles: every rank's rows are padded to it
    const size_t row = row_doubles(stride);
    DevMem gathered, frame;
    gathered.alloc(root, (size_t)n * row * sizeof(double));
    frame.alloc(root, frame_bytes(p->width, p->height));
    // a rank on the root's device renders straight into its slot of the gathered buffer; the others (every rank when the
    // exchange is forced) into a row of their own on their device, which then travels
    std::vector<DevMem> rows((size_t)n);
    std::vector<double*> dst((size_t)n);
    std::vector<int> uniq;  // comm rank r = uniq[r]; the root's device first
    auto comm_rank = [&](int dev) {
        for (size_t r = 0; r < uniq.size(); r++)
            if (uniq[r] == dev) return (int)r;
        uniq.push_back(dev);
        return (int)uniq.size() - 1;
    };
    comm_rank(root);
    std::vector<RowMove> moves((size_t)n, RowMove{0, nullptr, 0, nullptr, 0});  // moves[i].count == 0: rank i's rows stay where they are rendered
    size_t n_moves = 0;
    for (int i = 0; i < n; i++) {
        double* slot = (double*)gathered.p + (size_t)i * row;
        if (ids[(size_t)i] == root && !force) {
            dst[(size_t)i] = slot;
        } else {
            rows[(size_t)i].alloc(ids[(size_t)i], row * sizeof(double));
            dst[(size_t)i] = (double*)rows[(size_t)i].p;
            const size_t count = (size_t)plans[(size_t)i].tiles_owned * TILE_PIX * 3;
            if (count) {
                moves[(size_t)i] = RowMove{comm_rank(ids[(size_t)i]), (const double*)rows[(size_t)i].p, 0, slot, count};
                n_moves++;
            }
        }
    }
    // the communicators BEFORE the renders start (creating them is the expensive part of a first call and no part of the exchange)
    ExchangeLease lease;
    double comm_init_ms = 0.;
    if (n_moves) {
        const auto tc = std::chrono::steady_clock::now();
        bool created = false;
        lease.e = exchange_open(uniq, &created);
        if (created) comm_init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
    }
    std::mutex post_mu;  // one rank at a time drives the communicators (exchange_post)
    std::vector<rt_stats> st((size_t)n);
    std::vector<int> rc((size_t)n, (int)RT_OK);
    std::vector<std::string> msg((size_t)n);
    std::vector<double> posted_ms((size_t)n, 0.);
    auto work = [&](int i) {
        try {
            dev_set_device(ids[(size_t)i]);
            std::memset(&st[(size_t)i], 0, sizeof(rt_stats));
            if (cfg) render_sppm(s, cd, plans[(size_t)i], *cfg, dst[(size_t)i], nullptr, nullptr, &st[(size_t)i], nullptr);
            else render_tiles(s, cd, plans[(size_t)i], dst[(size_t)i], nullptr, &st[(size_t)i]);
            if (moves[(size_t)i].count) {  // this rank's rows leave NOW: the ranks still rendering do not hold them up
                std::lock_guard<std::mutex> g(post_mu);
                try {
                    exchange_post(lease.e, moves[(size_t)i]);
                } catch (...) {
                    lease.failed = true;
                    throw;
                }
                posted_ms[(size_t)i] = ms_since(std::chrono::steady_clock::now());
            }
        } catch (const RtError& e) {
            rc[(size_t)i] = e.code;
            msg[(size_t)i] = e.msg;
        } catch (const std::exception& e) {
            rc[(size_t)i] = RT_ERR_INTERNAL;
            msg[(size_t)i] = e.what();
        } catch (...) {
            rc[(size_t)i] = RT_ERR_INTERNAL;
            msg[(size_t)i] = "unknown error";
        }
    };
    {
        std::vector<std::thread> th;
        for (int i = 1; i < n; i++) th.emplace_back(work, i);
        work(0);  // rank 0 on the calling thread, as the reference's caller blocks in capture_image
        for (auto& t : th) t.join();
    }
    const auto t1 = std::chrono::steady_clock::now();
    // ---- the exchange: every posted row has to arrive in its slot on the root device (also after a failed rank: nothing may still be in
    //      flight when the buffers go back to the pool)
    if (lease.e) {
        try {
            exchange_wait(lease.e);
        } catch (...) {
            lease.failed = true;
            throw;
        }
    }
    for (int i = 0; i < n; i++)
        if (rc[(size_t)i] != RT_OK) throw RtError(rc[(size_t)i], "rank " + std::to_string(i) + " (device " + std::to_string(ids[(size_t)i]) + "): " + msg[(size_t)i]);
    const auto t2 = std::chrono::steady_clock::now();
    dev_set_device(root);
    stitch_to_host(plans[0], (const double*)gathered.p, stride, (double*)frame.p, out_rgb);
    const auto t3 = std::chrono::steady_clock::now();
    if (stats) {
        for (int i = 0; i < n; i++) {
            stats[i] = st[(size_t)i];
            stats[i].samples = pixels_in_image(plans[(size_t)i]) * (uint64_t)plans[(size_t)i].spp;
            stats[i].posted_ms = posted_ms[(size_t)i];
        }
        stats[0].seconds = std::chrono::duration<double>(t3 - t0).count();
        stats[0].exchange_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();  // the last rank's finish (the join) -> all rows on the root
        stats[0].reserved[2] = (uint64_t)(stats[0].exchange_ms * 1e3);
        stats[0].reserved[3] = (uint64_t)n_moves;
        stats[0].stitch_copy_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
        stats[0].comm_init_ms = comm_init_ms;
    }
}

void render_sppm_frame(const rt_scene& s, const rt_camera& cam, const rt_params& p, const rt_sppm_config& cfg, double* out_rgb, double* stats_out,
                       uint64_t photons_stored[2], rt_stats* stats) {
    require_committed(s);
    require_device();
    const CallClock clock;
    DeviceScope dev_scope(p.device);
    const RenderPlan pl = make_sppm_plan(p);
    const CameraDev cd = make_camera(cam);
    DevBuf tiles(row_doubles(pl.tiles_owned) * sizeof(double)), frame(frame_bytes(pl.width, pl.height));
    rt_stats st{};
    render_sppm(s, cd, pl, cfg, tiles.f64(), stats_out, nullptr, &st, photons_stored);
    if (p.spp > 0) stitch_to_host(pl, tiles.f64(), pl.tiles_owned, frame.f64(), out_rgb);
    clock.finish(stats, st, (uint64_t)pl.width * pl.height * (uint64_t)p.spp);
}

}  // namespace rtamd
