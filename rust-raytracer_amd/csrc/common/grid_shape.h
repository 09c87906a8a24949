// The shape of the uniform grid over a photon map (SPPM gather, device/sppm.inc): cell size and cells per axis from the map's bounding
// box and its photon count.  Plain host arithmetic, shared by build_grid (device/kernels.hip) and rt_debug_grid_shape (abi.cpp).
#pragma once
#include <cmath>
#include <cstddef>

namespace rtamd {

static const int GRID_MAX_DIM = 161;  // 160 cells per axis along the longest extent, + 1 for the photon on the upper face

// Photons lie on surfaces: aim at ~4 per occupied cell  ->  cell ~ 2 * sqrt(area / n), never less than longest / 160.
// Fallbacks: a box without area (a line, a point) takes cell = its longest extent, a point takes cell = 1.  n == 0: cell = 1, dim = 1.
// Returns false where an extent hi - lo is negative or not finite (a NaN or infinite coordinate); cell and dim are then not written.
inline bool grid_shape(const double lo[3], const double hi[3], size_t n, double* cell_out, int dim[3]) {
    if (n == 0) {
        *cell_out = 1.;
        dim[0] = dim[1] = dim[2] = 1;
        return true;
    }
    double ext[3];
    for (int a = 0; a < 3; a++) {
        ext[a] = hi[a] - lo[a];
        if (!(ext[a] >= 0.) || !std::isfinite(ext[a])) return false;
    }
    double area = 2. * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]);
    double longest = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
    double cell = 2. * std::sqrt(area / (double)n);
    if (!(cell > 0.)) cell = longest > 0. ? longest : 1.;
    const double min_cell = longest / 160.;  // at most 160 cells per axis
    if (cell < min_cell) cell = min_cell;
    if (!(cell > 0.)) cell = 1.;
    for (int a = 0; a < 3; a++) {
        int d = (int)std::floor(ext[a] / cell) + 1;
        if (d < 1) d = 1;
        if (d > GRID_MAX_DIM) d = GRID_MAX_DIM;
        dim[a] = d;
    }
    *cell_out = cell;
    return true;
}

}  // namespace rtamd
