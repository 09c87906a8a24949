// Per-render pads of the LDS node table (NodeW, csrc/device/kernels.hip "box32w").
//
// The blob's Node2 boxes are padded for every ray origin a render may be asked for: pad_w = 3 * 2^-22 * origin_limit2, with
// origin_limit2 = 64 x the scene's extent (host/accel.cpp, build_bvhs).  One render needs less: its origins are the lens and points
// on the scene's items, all within O_r = 2 * max(extent, camera bound), and the pad that box32w's proof asks for that bound is
// pad_r = 3 * 2^-22 * O_r.  The workgroup that expands Node2 into NodeW rows therefore moves every plane inward by
// shrink <= pad_w - pad_r.  Every rounding goes OUTWARD: the tightened box is never smaller than B -+ pad_r and never larger than
// the stored one.  Host and device run the code below; tests/test_tighten.py drives it from a host program.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RT_TIGHTEN_HD __host__ __device__
#else
#define RT_TIGHTEN_HD
#endif

namespace rtamd {

// the f32 neighbours of a finite f (no library call: the same code on both sides)
RT_TIGHTEN_HD inline float f32_below(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u << 1) == 0u) u = 0x80000001u;  // +-0 -> the smallest negative number
    else u = (u >> 31) ? u + 1u : u - 1u;
    memcpy(&f, &u, 4);
    return f;
}
RT_TIGHTEN_HD inline float f32_above(float f) { return -f32_below(-f); }

// One child box of a Node2, its planes moved inward by `shrink` (>= 0, finite).  The sums are taken in f64 and the f32 result is
// stepped one ulp outward whichever way the conversion rounded (that also covers the rounding of the f64 sum itself), then clamped
// to the stored plane: lo <= lo' <= lo + shrink and hi - shrink <= hi' <= hi.  The zero-size second child of a one-item BVH
// (lo == hi on every axis, accel.cpp) is a point on purpose and stays one.
RT_TIGHTEN_HD inline void tighten_box(float lo[3], float hi[3], float shrink) {
    if (lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2]) return;
    for (int k = 0; k < 3; k++) {
        const float l = f32_below((float)((double)lo[k] + (double)shrink));
        const float h = f32_above((float)((double)hi[k] - (double)shrink));
        if (l > lo[k]) lo[k] = l;
        if (h < hi[k]) hi[k] = h;
    }
}

// The origin bound of one render: ew = origin_limit2 / 64 (exact: a power of two), cam_abs = the largest |coordinate| the lens reaches.
// The factor 2 covers a hit point o + t d that lands a rounding outside its item's box; the max keeps O_r >= ew, which the
// "t |d| <= 2 |o|max" step of box32w's proof needs (|o|max bounds item coordinates as well).
inline double render_origin_bound(double origin_limit2, double cam_abs) { return 2. * std::fmax(origin_limit2 / 64., cam_abs); }

// shrink = pad_w - pad_r as an f32 rounded toward zero (and one ulp further: pad_w as accel.cpp computed it carries an f64 rounding
// of its own); exactly 0 at and beyond the limit, for a scene that is not eligible, and for anything that is not a number.
inline float box_shrink(double origin_limit2, double o_r, bool eligible) {
    if (!eligible || !(o_r < origin_limit2) || !(o_r >= 0.)) return 0.f;
    const double s = 3. * std::ldexp(origin_limit2, -22) - 3. * std::ldexp(o_r, -22);
    if (!(s > 0.) || !std::isfinite(s)) return 0.f;
    float f = (float)s;
    if ((double)f > s) f = f32_below(f);
    f = f32_below(f);
    return f > 0.f ? f : 0.f;
}

}  // namespace rtamd
