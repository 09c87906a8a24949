// rt_debug_sppm_trace_device (rtamd.h "diagnostics"): the photon pass and the eye pass of one iteration of render_sppm on a committed scene.
// Included at the end of kernels.hip.  The driver below has no kernel and no choice of its own: the light table, the kernel variant and
// its launch shape, the launches and the grow-and-retry of the stores are the functions render_sppm calls (SppmLights, sppm_choose,
// sppm_capacities, sppm_launch_photons, sppm_collect_photons, sppm_launch_eye).  It runs one iteration on one stream and copies out what
// the kernels wrote.

namespace rtamd {

namespace {
// the three arrays of a PhotonStore -> n x 9 {position, power, norm} of the caller
void download_photons(const PhotonStore& ps, unsigned int n, double* rows) {
    if (n == 0) return;
    std::vector<double> pos(3 * (size_t)n), power(3 * (size_t)n), norm(3 * (size_t)n);
    ps.pos.download(pos.data(), pos.size() * 8);
    ps.power.download(power.data(), power.size() * 8);
    ps.norm.download(norm.data(), norm.size() * 8);
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            rows[9 * i + a] = pos[3 * i + a];
            rows[9 * i + 3 + a] = power[3 * i + a];
            rows[9 * i + 6 + a] = norm[3 * i + a];
        }
}
}  // namespace

// (the arguments and sppm_refuse were checked by abi.cpp)  Returns true where a unit() of one of the passes met a zero vector.
bool debug_sppm_trace_device(const rt_scene& s, const CameraDev& cam, rt_debug_sppm_trace& io) {
    const Tuning tun = tuning();  // one snapshot per call
    hipStream_t stream = nullptr;
    const size_t npix = (size_t)io.width * io.height;
    const SppmLaunch L = sppm_choose(s, cam, tun, io.photons_per_iter, npix);
    SppmLights lights;
    lights.prepare(s);
    io.shift = lights.S;
    io.variant = L.word();
    io.photon_launches = 0;
    io.n_global = io.n_caustic = 0;
    SppmK sk{};
    sk.width = io.width; sk.height = io.height; sk.photons_per_iter = io.photons_per_iter;
    sk.k_global = 1; sk.k_caustic = 1; sk.max_bounces = io.max_bounces; sk.alpha = 1.;  // (k and alpha belong to the gather: neither pass reads them)
    sk.seed = io.seed; sk.S = lights.S; sk.iteration = io.iteration;
    sk.knn_cand = KNN_CAND;
    bool unit_zero = false;
    bool too_small = false;
    if (io.global || io.caustic) {
        DevBuf d_cursor, d_err_p;
        d_cursor.alloc(4);
        d_err_p.zeros(4);
        PhotonStore sg, sc;
        unsigned int cap_g = io.capacity_global, cap_c = io.capacity_caustic;
        sppm_capacities(io.photons_per_iter, tun, cap_g, cap_c);
        sg.alloc(cap_g);
        sc.alloc(cap_c);
        auto launch = [&] {
            sppm_launch_photons(L, sk, lights.lk, sg, sc, (unsigned int*)d_cursor.p, (int*)d_err_p.p, stream);
            io.photon_launches++;
        };
        launch();
        unsigned int ng = 0, nc = 0;
        try {
            sppm_collect_photons(sg, sc, (int*)d_err_p.p, stream, ng, nc, launch);
        } catch (const RtError& e) {
            if (e.code != RT_ERR_UNIT_ZERO) throw;
            unit_zero = true;  // (the stores hold what the launch wrote, up to their capacities)
            ng = std::min(ng, sg.b.cap);
            nc = std::min(nc, sc.b.cap);
        }
        io.n_global = ng;
        io.n_caustic = nc;
        too_small = (io.global && io.global_rows < ng) || (io.caustic && io.caustic_rows < nc);
        if (!too_small) {
            if (io.global) download_photons(sg, ng, io.global);
            if (io.caustic) download_photons(sc, nc, io.caustic);
        }
    }
    if (io.points) {
        DevBuf d_cam, d_gp, d_err;
        CamK ck = to_camk(cam);
        d_cam.upload(&ck, sizeof(CamK));
        d_err.zeros(4);
        d_gp.zeros(npix * 7 * 8);  // the kernel writes only `valid` of a pixel without a gather point
        sppm_launch_eye(L, (const CamK*)d_cam.p, sk, (double*)d_gp.p, (int*)d_err.p, stream);
        HIP_CHECK(hipGetLastError());
        const int h_err = wait_error_word(d_err.p, stream);
        d_gp.download(io.points, npix * 7 * 8);
        unit_zero = unit_zero || (h_err & 1) != 0;
    }
    if (too_small) throw RtError(RT_ERR_ARG, "rt_debug_sppm_trace_device: a photon buffer holds fewer rows than its map (n_global, n_caustic are set)");
    return unit_zero;
}

}  // namespace rtamd
