// rt_debug_sppm_gather_device (rtamd.h "diagnostics"): one iteration of the SPPM gather on explicit photon maps and gather points.
// Included at the end of kernels.hip: the driver below uploads the caller's arrays and then launches what render_sppm launches per
// iteration -- build_grid and PhotonStore::sort_into_grid for both maps, gather_kernel, estimate_kernel -- with render_sppm's launch
// shapes.  It has no kernel of its own, and no render kernel changes.

namespace rtamd {

namespace {
// n x 9 {position, power, norm} of the caller -> the three arrays of a PhotonStore
void upload_photons(PhotonStore& ps, const double* rows, unsigned int n) {
    ps.alloc(n);
    if (n == 0) return;
    std::vector<double> pos(3 * (size_t)n), power(3 * (size_t)n), norm(3 * (size_t)n);
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            pos[3 * i + a] = rows[9 * i + a];
            power[3 * i + a] = rows[9 * i + 3 + a];
            norm[3 * i + a] = rows[9 * i + 6 + a];
        }
    dev_copy_to_device(ps.pos.p, pos.data(), pos.size() * 8);
    dev_copy_to_device(ps.power.p, power.data(), power.size() * 8);
    dev_copy_to_device(ps.norm.p, norm.data(), norm.size() * 8);
}
// what build_grid made of a map, and the two tables where the caller gave buffers for them
void report_grid(const Grid& g, unsigned int n, rt_debug_grid& out) {
    for (int a = 0; a < 3; a++) {
        out.lo[a] = g.k.lo[a];
        out.dim[a] = g.k.dim[a];
    }
    out.cell = g.k.cell;
    if (n == 0) return;
    const size_t n_scan = (size_t)g.k.dim[0] * g.k.dim[1] * g.k.dim[2] + 1;
    if (out.cell_start) {
        if (out.cell_start_capacity < n_scan) throw RtError(RT_ERR_ARG, "rt_debug_sppm_gather_device: cell_start_capacity is below the grid's cells + 1");
        g.cell_start.download(out.cell_start, n_scan * 4);
    }
    if (out.index) {
        if (out.index_capacity < n) throw RtError(RT_ERR_ARG, "rt_debug_sppm_gather_device: index_capacity is below the map's photons");
        g.index.download(out.index, (size_t)n * 4);
    }
}
}  // namespace

// (the arguments were checked by abi.cpp)  Returns true where a unit() of the gather met a zero vector.
bool debug_sppm_gather_device(rt_debug_sppm_gather& io) {
    const Tuning tun = tuning();  // one snapshot per call
    hipStream_t stream = nullptr;
    const unsigned int ng = (unsigned int)io.n_global, nc = (unsigned int)io.n_caustic;
    const size_t m = (size_t)io.m;
    PhotonStore sg, sc;
    upload_photons(sg, io.global, ng);
    upload_photons(sc, io.caustic, nc);
    DevBuf d_gp, d_stats, d_est, d_err;
    d_gp.upload(io.points, m * 7 * 8);
    d_stats.upload(io.stats, m * 10 * 8);
    d_est.alloc(m * 6 * 8);
    d_err.zeros(4);
    SppmK sk{};
    sk.width = (int)m; sk.height = 1;  // gather_kernel's pixel count
    sk.k_global = io.k_global; sk.k_caustic = io.k_caustic; sk.alpha = io.alpha; sk.S = io.shift;
    sk.knn_cand = KNN_CAND;
    if (tun.knn_cand >= 0) sk.knn_cand = std::min(KNN_CAND, tun.knn_cand);  // as render_sppm
    // one iteration of render_sppm's loop, without its photon and eye passes
    Grid gg, gc;
    build_grid(gg, sg.b, ng, stream);
    build_grid(gc, sc.b, nc, stream);
    sg.sort_into_grid(gg, ng, stream);
    sc.sort_into_grid(gc, nc, stream);
    const size_t pix_per_block = GATHER_BLOCK / 64;  // one wave per gather point
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((m + pix_per_block - 1) / pix_per_block)), dim3(GATHER_BLOCK), 0, stream, sk,
                       (const double*)d_gp.p, gg.k, sg.s, gc.k, sc.s, (double*)d_stats.p, (int*)d_err.p);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(estimate_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const double*)d_stats.p, m, io.n_emitted,
                       (double*)d_est.p);
    HIP_CHECK(hipGetLastError());
    const int h_err = wait_error_word(d_err.p, stream);
    d_stats.download(io.stats, m * 10 * 8);
    d_est.download(io.estimates, m * 6 * 8);
    report_grid(gg, ng, io.grid_global);
    report_grid(gc, nc, io.grid_caustic);
    return (h_err & 1) != 0;
}

}  // namespace rtamd
