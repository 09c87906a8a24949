// rtamd_render -- the reference's main.rs (main.rs:49-72) on top of the C ABI:
//   let world = select_scene(0); let result = world.cam.capture_image(integrator); result.save("output/test.png")
// and the same "Total / RT" timing print.  Also renders the reference's scene files.
//   rtamd_render [--scene cornell|FILE.json|FILE.yaml] [--cube data/mesh/cube.obj] [-w W] [-h H] [--spp N]
//                [--depth D] [--seed S] [--aspect A] [--integrator 0|1] [--sppm ITERATIONS PHOTONS_PER_ITER]
//                [--gpus N | --devices 0,1,...] [--background r,g,b | --sky] [--env-sampling] [--region x0,y0,x1,y1] [-o out.png]
//                [--denoise [--aov-spp N] [--luma-mode M]] [--sequence N [--orbit-step DEG]] [--ao FILE.png [--ao-rays K] [--ao-distance D]] [--describe] [--vec3-selftest]
// --gpus N spreads the frame over N GPUs of this node inside ONE capture_image call (rt_render_multi: tiles dealt round-robin, RCCL
// gather; 0 = all visible); --devices names the HIP ordinal of every rank (an ordinal may repeat).
// `rtamd_render --cube data/mesh/cube.obj --sppm 50 500000` is the reference binary: SPPM pre-pass + 256 spp, output/test.png
// --background r,g,b gives rays that leave the scene a constant colour, --sky book 1's sky gradient (rt_scene_set_background; the
// reference has neither: its misses are black); --env-sampling makes that background one more light of --integrator 1
// (rt_scene_set_env_sampling, automatic table size)
// --region x0,y0,x1,y1 renders only the pixels [x0, x1) x [y0, y1) of the W x H frame (rt_region_render: the frame's own pixels, at the
// cost of the 8x8 tiles they touch) and writes the cropped PNG
// --denoise renders the frame and filters it in one call (rt_denoised_render: --spp must be even) and writes the denoised PNG; --aov-spp N
// guide rays per pixel (default 4; 0: none, for scenes with media or moving spheres), --luma-mode 1 (default) the energy-preserving
// symmetric luminance stop, 0 rt_denoise's
// --sequence N renders N frames with temporal accumulation (rt_sequence_frame: --spp samples per frame, even; --aov-spp guide rays, at
// least 1; --luma-mode 1 / 0 filters the accumulation, -1 writes it unfiltered; frame f runs with seed --seed + f).  Between frames the
// camera turns about its look_at point around the y axis by --orbit-step DEG (default 0), and frame f goes to NAME_%03d.png for -o NAME.png
// --ao FILE.png writes the ambient-occlusion pass of the frame (rt_ao_render: 4 camera rays per pixel, --ao-rays K occlusion rays per hit,
// default 4, that reach no farther than --ao-distance D, default unlimited) as the grey image visibility * coverage, and nothing else
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rtamd.hpp"

using namespace rtamd_host;

// the reference's Vec3 unit tests (vec3.rs:425-564) against the mirrored Vec3
static int vec3_selftest() {
    int fails = 0;
#define EXPECT(c) if (!(c)) { std::printf("FAIL: %s\n", #c); fails++; }
    EXPECT(Vec3(1.0, 0.0, -1.0) + Vec3(2.0, 4.0, 6.0) == Vec3(3.0, 4.0, 5.0));
    EXPECT(Vec3(1.0, 0.0, -1.0) + 233.0 == Vec3(234.0, 233.0, 232.0));
    EXPECT(Vec3(1.0, 0.0, -1.0) - Vec3(2.0, 4.0, 6.0) == Vec3(-1.0, -4.0, -7.0));
    EXPECT(Vec3(1.0, 0.0, -1.0) - 1.0 == Vec3(0.0, -1.0, -2.0));
    EXPECT(Vec3(1.0, 0.0, -1.0) * Vec3::ones() == 0.0);
    EXPECT(Vec3(1.0, 0.0, -1.0) * 2.0 == Vec3(2.0, 0.0, -2.0));
    EXPECT(Vec3(1.0, -2.0, 0.0) / 2.0 == Vec3(0.5, -1.0, 0.0));
    EXPECT(Vec3::elemul(Vec3(1.0, 2.0, 3.0), Vec3(1.0, 2.0, 3.0)) == Vec3(1.0, 4.0, 9.0));
    EXPECT(Vec3::cross(Vec3(1.0, 2.0, 3.0), Vec3(2.0, 3.0, 4.0)) == Vec3(8.0 - 9.0, 6.0 - 4.0, 3.0 - 4.0));
    EXPECT(-Vec3(1.0, -2.0, 3.0) == Vec3(-1.0, 2.0, -3.0));
    EXPECT(Vec3(1.0, 2.0, 3.0).squared_length() == 14.0);
    EXPECT(Vec3(3.0, 4.0, 5.0).length() == std::sqrt(3.0 * 3.0 + 4.0 * 4.0 + 5.0 * 5.0));
    EXPECT(Vec3(233.0, 0.0, 0.0).unit() == Vec3(1.0, 0.0, 0.0));
    EXPECT(Vec3(-233.0, 0.0, 0.0).unit() == Vec3(-1.0, 0.0, 0.0));
    bool panicked = false;
    try { Vec3(0.0, 0.0, 0.0).unit(); } catch (const Error& e) { panicked = e.code == RT_ERR_UNIT_ZERO; }
    EXPECT(panicked);
    std::printf("vec3 selftest: %s\n", fails ? "FAILED" : "ok");
    return fails;
}

int main(int argc, char** argv) {
    std::string scene = "cornell", cube = "data/mesh/cube.obj", out = "output/test.png";
    Config cfg;
    double aspect = -1;
    bool describe = false;
    std::string checkpoint;  // --checkpoint FILE [--run-samples K]: trace the next K samples per pixel into the state in FILE; the image is written once all are in
    int run_samples = 64;
    rt_background bg{};  // kind 0: none
    bool env_sampling = false;
    rt_region region{0, 0, 0, 0};
    bool crop = false;
    bool denoise_frame = false;
    int aov_spp = 4, luma_mode = 1;
    int sequence_frames = 0;
    double orbit_step = 0.;
    std::string ao_out;
    int ao_rays = 4;
    double ao_distance = INFINITY;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--scene") scene = next();
        else if (a == "--cube") cube = next();
        else if (a == "-w") cfg.width = std::atoi(next());
        else if (a == "-h") cfg.height = std::atoi(next());
        else if (a == "--spp") cfg.sample_per_pixel = std::atoi(next());
        else if (a == "--depth") cfg.max_depth = std::atoi(next());
        else if (a == "--seed") cfg.seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--aspect") aspect = std::atof(next());
        else if (a == "--integrator") cfg.integrator = std::atoi(next());
        else if (a == "--sppm") { cfg.sppm_iterations = std::atoi(next()); cfg.sppm_photons_per_iter = std::atoi(next()); }
        else if (a == "--gpus") cfg.gpus = std::atoi(next());
        else if (a == "--devices") {
            for (const char* q = next(); *q;) {
                cfg.devices.push_back((int)std::strtol(q, const_cast<char**>(&q), 10));
                if (*q == ',') q++;
                else if (*q) { std::fprintf(stderr, "--devices wants a comma-separated list of ordinals\n"); return 2; }
            }
        }
        else if (a == "--sky") bg = World::background_sky();
        else if (a == "--env-sampling") env_sampling = true;
        else if (a == "--background") {
            double c[3];
            if (std::sscanf(next(), "%lf,%lf,%lf", &c[0], &c[1], &c[2]) != 3) { std::fprintf(stderr, "--background wants r,g,b\n"); return 2; }
            bg = World::background_color(c[0], c[1], c[2]);
        }
        else if (a == "--region") {
            if (std::sscanf(next(), "%d,%d,%d,%d", &region.x0, &region.y0, &region.x1, &region.y1) != 4) { std::fprintf(stderr, "--region wants x0,y0,x1,y1\n"); return 2; }
            crop = true;
        }
        else if (a == "--denoise") denoise_frame = true;
        else if (a == "--aov-spp") aov_spp = std::atoi(next());
        else if (a == "--luma-mode") luma_mode = std::atoi(next());
        else if (a == "--sequence") sequence_frames = std::atoi(next());
        else if (a == "--orbit-step") orbit_step = std::atof(next());
        else if (a == "--ao") ao_out = next();
        else if (a == "--ao-rays") ao_rays = std::atoi(next());
        else if (a == "--ao-distance") ao_distance = std::atof(next());
        else if (a == "-o") out = next();
        else if (a == "--checkpoint") { checkpoint = next(); }
        else if (a == "--run-samples") run_samples = std::atoi(next());
        else if (a == "--describe") describe = true;
        else if (a == "--vec3-selftest") return vec3_selftest();
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    try {
        auto start_time = std::chrono::steady_clock::now();
        std::unique_ptr<World> world;
        const rt_env_sampling env = World::env_sampling_on();
        const rt_env_sampling* envp = env_sampling ? &env : nullptr;
        if (scene == "cornell") {
            world = cornell_box_scene(cube, aspect > 0 ? aspect : (double)cfg.width / cfg.height, 1, bg.kind ? &bg : nullptr, envp);
        } else {
            world = std::make_unique<World>(scene, bg.kind ? &bg : nullptr, envp);
            if (aspect > 0) world->cam.c.aspect = aspect;
        }
        rt_scene_info info;
        check(rt_scene_info_get(world->handle(), &info));
        std::printf("scene: %d nodes (%d boxes, %d spheres, %d rects, %d tris, %d xforms), %llu bytes flattened\n", info.n_nodes, info.n_boxes,
                    info.n_spheres, info.n_rects, info.n_tris, info.n_xforms, (unsigned long long)info.bytes);
        if (describe) return 0;
        if (!checkpoint.empty()) {
            RgbImage img;
            int done = 0;
            const bool complete = world->capture_image_resumable(cfg, checkpoint, run_samples, &img, &done);
            std::printf("checkpoint %s: %d of %d samples per pixel done%s\n", checkpoint.c_str(), done, cfg.sample_per_pixel, complete ? "" : " (run again to continue)");
            if (complete) img.save(out);
            return 0;
        }
        auto rt_start = std::chrono::steady_clock::now();
        rt_stats st{};
        if (crop) {
            const std::vector<double> rad = world->render_regions(cfg, {region}, 0, &st)[0];
            RgbImage img;
            img.width = region.x1 - region.x0;
            img.height = region.y1 - region.y0;
            img.data.resize(rad.size());
            check(rt_tonemap_u8(rad.data(), rad.size(), img.data.data()));
            img.save(out);
            std::printf("region (%d, %d, %d, %d): %llu samples traced, kernel %.1f ms, %.3fs\n", region.x0, region.y0, region.x1, region.y1,
                        (unsigned long long)st.samples, st.kernel_ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - rt_start).count());
            return 0;
        }
        if (!ao_out.empty()) {
            const std::vector<double> ao = world->render_ao(cfg, 4, ao_rays, ao_distance, 0, &st);
            const size_t npix = (size_t)cfg.width * cfg.height;
            std::vector<double> grey(npix * 3);
            for (size_t i = 0; i < npix; i++) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = ao[8 * i] * ao[8 * i + 7];
            RgbImage img;
            img.width = cfg.width;
            img.height = cfg.height;
            img.data.resize(grey.size());
            check(rt_tonemap_u8(grey.data(), grey.size(), img.data.data()));
            img.save(ao_out);
            std::printf("ambient occlusion (%d rays per hit): %llu camera rays, kernel %d, %.1f ms, %.3fs\n", ao_rays, (unsigned long long)st.samples,
                        st.kernel_used, st.kernel_ms, st.seconds);
            return 0;
        }
        if (sequence_frames > 0) {
            Sequence seq(cfg.width, cfg.height);
            const Camera cam0 = world->cam;
            const size_t dot = out.rfind('.');
            const std::string stem = dot == std::string::npos ? out : out.substr(0, dot), ext = dot == std::string::npos ? ".png" : out.substr(dot);
            for (int f = 0; f < sequence_frames; f++) {
                // look_from turned about look_at around the y axis by f * orbit_step degrees
                Camera cam = cam0;
                const double a = orbit_step * (double)f * 3.14159265358979323846 / 180.0, c = std::cos(a), s = std::sin(a);
                const double dx = cam0.c.look_from[0] - cam0.c.look_at[0], dz = cam0.c.look_from[2] - cam0.c.look_at[2];
                cam.c.look_from[0] = cam0.c.look_at[0] + (c * dx + s * dz);
                cam.c.look_from[2] = cam0.c.look_at[2] + (-s * dx + c * dz);
                Config fc = cfg;
                fc.seed = cfg.seed + (uint64_t)f;
                const std::vector<double> rad = seq.frame(*world, cam, fc, aov_spp, luma_mode, nullptr, nullptr, nullptr, nullptr, 0, &st);
                RgbImage img;
                img.width = cfg.width;
                img.height = cfg.height;
                img.data.resize(rad.size());
                check(rt_tonemap_u8(rad.data(), rad.size(), img.data.data()));
                char num[16];
                std::snprintf(num, sizeof(num), "_%03d", f);
                img.save(stem + num + ext);
                std::printf("frame %d of %d (%.2f degrees, seed %llu): %llu samples, kernel %.1f ms, %.3fs\n", f, sequence_frames, orbit_step * f,
                            (unsigned long long)fc.seed, (unsigned long long)st.samples, st.kernel_ms, st.seconds);
            }
            return 0;
        }
        if (denoise_frame) {
            const std::vector<double> rad = world->render_denoised(cfg, aov_spp, luma_mode, nullptr, nullptr, nullptr, nullptr, 0, &st);
            RgbImage img;
            img.width = cfg.width;
            img.height = cfg.height;
            img.data.resize(rad.size());
            check(rt_tonemap_u8(rad.data(), rad.size(), img.data.data()));
            img.save(out);
            std::printf("denoised (luma mode %d, %d guide rays per pixel): %llu samples, kernel %.1f ms in %d launches, %.3fs\n", luma_mode, aov_spp,
                        (unsigned long long)st.samples, st.kernel_ms, st.launches, st.seconds);
            return 0;
        }
        std::vector<rt_stats> ranks;
        RgbImage result = world->capture_image(cfg, &st, nullptr, &ranks);
        result.save(out);
        auto end = std::chrono::steady_clock::now();
        double total = std::chrono::duration<double>(end - start_time).count(), rt = std::chrono::duration<double>(end - rt_start).count();
        double sppm = st.reserved[0] * 1e-6;
        std::printf("Total: %.3fs\n\tSPPM: %.3fs\n\tRT: %.3fs\n", total, sppm, rt - sppm);  // main.rs:57-71
        std::printf("%.2f Msamples/s (%llu samples, kernel %.1f ms in %d launches, scene %s)\n", st.samples / st.seconds / 1e6,
                    (unsigned long long)st.samples, st.kernel_ms, st.launches, st.scene_in_lds ? "in LDS" : "in L2/HBM");
        for (size_t i = 0; i < ranks.size(); i++)
            std::printf("\trank %zu: kernel %d, %.1f ms, %llu samples%s\n", i, ranks[i].kernel_used, ranks[i].kernel_ms, (unsigned long long)ranks[i].samples,
                        i == 0 ? (", exchange + stitch " + std::to_string(ranks[0].reserved[2] * 1e-3) + " ms, " + std::to_string(ranks[0].reserved[3]) + " rows through RCCL " +
                                  std::to_string(rt_rccl_version())).c_str() : "");
    } catch (const Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
