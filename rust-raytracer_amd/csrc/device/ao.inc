// rt_ao_render (DESIGN.md s4k): ambient occlusion / sky visibility, a bent normal and the ambient term lit by the scene's background,
// and the library's any-hit walks.  Included at the end of kernels.hip, whose primitive tests, box tests, materialize and
// background_radiance it uses as they are; no render kernel changes.
//
// Any-hit: "does World::hit(ray, t_min, t_max) return a hit" without finding which.  The walks below return at the first primitive whose
// own f64 test accepts a t in [t_min, t_max]; they keep no best hit, build no record, note no tie and never shrink t_max.  That is the
// closest-hit walks' answer: those accept the first such primitive too (nothing is closer yet) and a walk that holds a hit ends with one.
// Two lean functions instead of one more flag on traverse / traverse2: an any-hit walk shares the node loop's shape with them but none of
// what their flags steer (the best hit, the tie rule, deferring, tracking), and nothing compiled into the render kernels is touched.
//
// One pixel per thread.  Sample s of pixel (x, y) is pt_kernel's camera ray (stream (seed, pix, s)) and its first hit, as aov_kernel
// finds it; every hit sends K occlusion rays from its point, cosine-distributed around its front-facing normal, each with a fresh stream
// (seed ^ AO_STREAM, pix, s * K + k).  Sums in (s, k) order, f64; out[pix] = {visibility, bent[3], ambient[3], coverage}.

#include "ao.h"

namespace rtamd {

static const uint64_t AO_STREAM = 0x9E3779B97F4A7C15ull;  // keeps the direction draws apart from the jitter draws of every camera sample

// Any-hit over the reference-order program (traverse<>'s node loop: the same boxes, tested against the whole range).  GENERAL 1 or 3;
// scenes with media or moving spheres do not come here (aov_refuse).
template <int GENERAL>
DEV bool occluded(const Acc& A, D3 wo, D3 wd, double t_min, double t_max) {
    D3 o = wo, d = wd;
    D3 inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
    double a = sqlen(d);
    uint32_t n = 0u;
    const uint32_t N = A.n_nodes;
    while (n < N) {
        const uint2 m = A.meta[n];
        const uint32_t kind = m.x & NK_MASK, pl = m.x >> NK_BITS;
        double t;
        if (kind == NK_BOX) {
            n = aabb_hit(A.boxes + 3 * pl, o, inv, t_min, t_max) ? n + 1 : m.y;
            continue;
        }
        if (kind == NK_SPHERE) {
            if (sphere_hit(A.spheres + 2 * pl, o, d, a, t_min, t_max, t)) return true;
        } else if (kind == NK_RECT_YZ || kind == NK_RECT_XZ || kind == NK_RECT_XY) {
            if (rect_hit(A.rects + 3 * pl, (int)kind - (int)NK_RECT_YZ, o, d, t_min, t_max, t)) return true;
        } else if (kind == NK_CUBE) {
            uint32_t side;
            if (cube_hit(A.rects + 3 * (pl >> 3), o, d, t_min, t_max, t, side)) return true;
        } else if (kind == NK_TRI) {
            double b1, b2;
            if (tri_hit(A.tripre + 5 * pl, o, d, t_min, t_max, t, b1, b2)) return true;
        } else if (kind == NK_XFORM_BEGIN) {  // transform.rs:153-156
            if (GENERAL == 3) {  // chain pl: its innermost level applied to the parent's ray, which is the current one
                const double* Minv = A.xforms + 32 * chain_rec(A, pl)[1];
                o = xf_point(Minv, o);
                d = xf_dir(Minv, d);
            } else {
                const double* Minv = A.xforms + 32 * pl;
                o = xf_point(Minv, wo);
                d = xf_dir(Minv, wd);
            }
            inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
            a = sqlen(d);
        } else if (kind == NK_XFORM_END) {
            o = wo;
            d = wd;
            if (GENERAL == 3 && pl != 0u) chain_ray(A, pl - 1u, CHAIN_ALL, o, d);  // back to the parent chain's ray
            inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
            a = sqlen(d);
        }
        n++;
    }
    return false;
}

// The accel walk met a primitive that accepts a t at an end of the range: the reference's own walk decides.  World::hit may still miss
// there: BVHNode::hit culls a node whose box interval, clipped to [t_min, t_max], has shrunk to a point (aabb.rs:28-30) -- a cube face
// that IS its box's near face, asked with t_max = its hit distance -- and its slab arithmetic rounds apart from the primitive's own t, so
// the cull also happens a few ulps inside the range.  The accel's padded f32 boxes never cull such a hit; the reference-order walk
// tests the reference's boxes.  Out of line: rare (an explicit t_max or max_distance that equals a surface's distance), and the walk
// keeps its registers.
template <int GENERAL>
__device__ __noinline__ bool occluded_at_range_end(const Acc& A, D3 wo, D3 wd, double t_min, double t_max) {
    return occluded<GENERAL>(A, wo, wd, t_min, t_max);
}
enum { OCC_NO = 0, OCC_YES = 1, OCC_AT_END = 2 };  // occluded2's answers: OCC_AT_END = a primitive accepts at an end of the range
DEV bool at_range_end(double t, double t_min, double t_max) {  // within 2^-48 (relative) of either end; false for t_max = +inf
    return t * (1.0 + 0x1p-48) >= t_max || t * (1.0 - 0x1p-48) <= t_min;
}

// Any-hit through the accel: traverse2's plain form (Node2 array in global memory, the lane's stack a column of LDS words `stride`
// apart, first row 0, at most FlatView::stack2 - 2 entries: "The stack" above traverse2) with the range [t_min, t_max] fixed.  The f32
// boxes are conservative for every t in the range (box32's proof), so a primitive that accepts is reached; one that accepts at an end of the range
// ends the walk with OCC_AT_END and is settled by the reference-order walk (ray_occluded calls occluded_at_range_end), whose boxes may
// cull it as World::hit's do.
template <int GENERAL>
DEV int occluded2(const Acc& A, uint32_t* stk, const int stride, D3 wo, D3 wd, double t_min, double t_max) {
    D3 o = wo, d = wd;
    double a = sqlen(d);
    int cur_xf = -1;
    Ray32 r = make_ray32(o, d, t_min, t_max);
    int sp = 0;
    uint32_t cur = A.root2;
    for (;;) {
        while ((cur >> REF_TAG_SHIFT) == 0u) {  // inner node: test both children
            const f32x4* p = (const f32x4*)A.n2 + NODE2_F4 * cur;
            const f32x4 q0 = p[0], q1 = p[1], q2 = p[2];
            const f32x2 q3 = *(const f32x2*)(p + 3);
            float e0, e1;
            const bool h0 = box32(q0.x, q0.z, q1.x, q1.z, q2.x, q2.z, r, e0);
            const bool h1 = box32(q0.y, q0.w, q1.y, q1.w, q2.y, q2.w, r, e1);
            const uint32_t c0 = __float_as_uint(q3.x), c1 = __float_as_uint(q3.y);
            if (h0 && h1) {  // nearer child first: an occluder close to the origin ends the walk soonest
                const bool swap = e1 < e0;
                stk[sp] = swap ? c0 : c1;
                sp += stride;
                cur = swap ? c1 : c0;
            } else if (h0) {
                cur = c0;
            } else if (h1) {
                cur = c1;
            } else if (sp > 0) {
                sp -= stride;
                cur = stk[sp];
            } else {
                cur = REF_DONE;
            }
        }
        if (cur == REF_DONE) return OCC_NO;
        if ((cur >> REF_TAG_SHIFT) == 1u) {  // leaf: the reference's f64 tests
            const uint32_t first = cur & REF_LEAF_FIRST_MASK, cnt = ((cur >> REF_LEAF_COUNT_SHIFT) & 7u) + 1u;
            uint32_t enter = REF_DONE;
            for (uint32_t i = 0; i < cnt; i++) {
                const uint2 it = A.items2[first + i];
                const uint32_t kind = it.x & NK_MASK, pl = it.x >> NK_BITS;
                double t;
                if (kind == NK_SPHERE) {
                    if (sphere_hit(A.spheres + 2 * pl, o, d, a, t_min, t_max, t)) return at_range_end(t, t_min, t_max) ? OCC_AT_END : OCC_YES;
                } else if (kind == NK_RECT_YZ || kind == NK_RECT_XZ || kind == NK_RECT_XY) {
                    if (rect_hit(A.rects + 3 * pl, (int)kind - (int)NK_RECT_YZ, o, d, t_min, t_max, t)) return at_range_end(t, t_min, t_max) ? OCC_AT_END : OCC_YES;
                } else if (kind == NK_CUBE) {
                    uint32_t side;
                    if (cube_hit(A.rects + 3 * (pl >> 3), o, d, t_min, t_max, t, side)) return at_range_end(t, t_min, t_max) ? OCC_AT_END : OCC_YES;
                } else if (kind == NK_TRI) {
                    double b1, b2;
                    if (tri_hit(A.tripre2 + 5 * (first + i), o, d, t_min, t_max, t, b1, b2)) return at_range_end(t, t_min, t_max) ? OCC_AT_END : OCC_YES;
                } else {  // an instance: its object-space BVH after the remaining items
                    enter = pl;
                }
            }
            if (enter != REF_DONE) {  // Transform::hit, transform.rs:153-156 (the marker carries the parent chain + 1, as in traverse2)
                const uint2 in = A.inst2[enter];
                const uint32_t restore = GENERAL == 3 ? REF_RESTORE | (uint32_t)(cur_xf + 1) : REF_RESTORE;
                if (GENERAL == 3) {
                    const double* Minv = A.xforms + 32 * chain_rec(A, in.x)[1];
                    o = xf_point(Minv, o);
                    d = xf_dir(Minv, d);
                } else {
                    const double* Minv = A.xforms + 32 * in.x;
                    o = xf_point(Minv, wo);
                    d = xf_dir(Minv, wd);
                }
                a = sqlen(d);
                cur_xf = (int)in.x;
                r = make_ray32(o, d, t_min, t_max);
                stk[sp] = restore;
                sp += stride;
                cur = in.y;
                continue;
            }
        } else {  // REF_RESTORE: leave the Transform
            o = wo;
            d = wd;
            cur_xf = -1;
            if (GENERAL == 3) {
                const uint32_t pc = cur & ~(3u << REF_TAG_SHIFT);
                if (pc != 0u) chain_ray(A, pc - 1u, CHAIN_ALL, o, d);
                cur_xf = (int)pc - 1;
            }
            a = sqlen(d);
            r = make_ray32(o, d, t_min, t_max);
        }
        if (sp > 0) {
            sp -= stride;
            cur = stk[sp];
        } else {
            cur = REF_DONE;
        }
    }
}

// The one question the pass and the diagnostic ask.  RT_AO_CLOSEST_HIT (A/B build, DESIGN.md s4k): the closest-hit walks answer it.
template <bool ACCEL, int GENERAL>
DEV bool ray_occluded(const Acc& A, uint32_t* stk, const int stride, D3 o, D3 d, double t_min, double t_max) {
#ifdef RT_AO_CLOSEST_HIT
    const Hit h = ACCEL ? traverse2<GENERAL, false, false>(A, stk, stride, o, d, t_min, t_max) : traverse<GENERAL>(A, o, d, t_min, t_max);
    return h.node >= 0;
#else
    if (!ACCEL) return occluded<GENERAL>(A, o, d, t_min, t_max);
    const int r = occluded2<GENERAL>(A, stk, stride, o, d, t_min, t_max);
    return r == OCC_AT_END ? occluded_at_range_end<GENERAL>(A, o, d, t_min, t_max) : r == OCC_YES;  // (the call after the walk's loops, as tie_resolve's)
#endif
}

template <bool ACCEL, int GENERAL>
__global__ void __launch_bounds__(64) ao_kernel(FlatView sv, CamK cam, int width, int height, uint64_t seed, double t_min, int ao_spp, int rays_per_hit,
                                                double max_distance, double* out, int* err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)width * (size_t)height) return;
    Acc A = make_acc(sv.base, sv.base, sv);
    uint32_t* stk = (uint32_t*)smem + threadIdx.x;
    const int x = (int)(pix % (size_t)width), y = (int)(pix / (size_t)width);
    const BgDev* bg = sv.off_bg != 0u ? (const BgDev*)(sv.base + sv.off_bg) : nullptr;
    double open = 0., b0 = 0., b1 = 0., b2 = 0., a0 = 0., a1 = 0., a2 = 0.;
    int hits = 0;
    for (int s = 0; s < ao_spp; s++) {
        // pt_kernel's camera ray
        Rng rng;
        rng.seed_stream(seed, (uint64_t)pix, (uint64_t)s);
        double u, st;
        D3 rd, o, d;
        camera_draw(cam, width, height, x, y, rng, u, st, rd);
        camera_ray(cam, u, st, rd, o, d);
        const Hit h = ACCEL ? traverse2<GENERAL, false, false>(A, stk, (int)blockDim.x, o, d, t_min, INFINITY) : traverse<GENERAL>(A, o, d, t_min, INFINITY);
        if (h.node < 0) continue;
        const Rec rec = materialize<GENERAL, false>(A, h, o, d, err);
        hits++;
        for (int k = 0; k < rays_per_hit; k++) {
            Rng dr;
            dr.seed_stream(seed ^ AO_STREAM, (uint64_t)pix, (uint64_t)s * (uint64_t)rays_per_hit + (uint64_t)k);
            // scattered_direction of a Lambertian, material.rs:92-98 (shade's order), then the unit direction
            const D3 us = unit(random_in_unit_sphere(dr), err);
            D3 dir = add(rec.normal, us);
            if (near_zero(dir)) dir = rec.normal;
            dir = unit(dir, err);
            if (ray_occluded<ACCEL, GENERAL>(A, stk, (int)blockDim.x, rec.p, dir, t_min, max_distance)) continue;
            open += 1.0;
            b0 += dir.x; b1 += dir.y; b2 += dir.z;
            if (bg) {
                const D3 c = background_radiance<(GENERAL >= 2 ? GENERAL : 2)>(bg, A.texs, A.texels, dir, err);
                a0 += c.x; a1 += c.y; a2 += c.z;
            }
        }
    }
    double* q = out + 8 * pix;
    if (hits == 0) {
        for (int k = 0; k < 8; k++) q[k] = 0.;
        return;
    }
    const double nr = (double)hits * (double)rays_per_hit;
    q[0] = open / nr;
    q[1] = b0 / nr; q[2] = b1 / nr; q[3] = b2 / nr;
    q[4] = a0 / nr; q[5] = a1 / nr; q[6] = a2 / nr;
    q[7] = (double)hits / (double)ao_spp;
}

// rt_debug_occluded_device: one row per thread, {origin, direction, t_max} -> 1.0 (occluded) or 0.0
template <bool ACCEL, int GENERAL>
__global__ void __launch_bounds__(64) occluded_kernel(FlatView sv, size_t n, const double* __restrict__ rays, double t_min, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Acc A = make_acc(sv.base, sv.base, sv);
    uint32_t* stk = (uint32_t*)smem + threadIdx.x;
    const D3 o = mk(rays[7 * i], rays[7 * i + 1], rays[7 * i + 2]), d = mk(rays[7 * i + 3], rays[7 * i + 4], rays[7 * i + 5]);
    out[i] = ray_occluded<ACCEL, GENERAL>(A, stk, (int)blockDim.x, o, d, t_min, rays[7 * i + 6]) ? 1. : 0.;
}

void render_ao_device(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel, const rt_ao_config& cfg,
                      double* d_out, void* stream_, rt_stats* st) {
    hipStream_t stream = (hipStream_t)stream_;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    const int walk = choose_pixel_walk(s, cam, t_min, kernel, dev_info(dev).lds_max);  // (before the upload: a refused call touches no device)
    double upload_ms = 0.;
    const FlatView view = device_view(s, &upload_ms).view;
    typedef void (*ao_fn)(FlatView, CamK, int, int, uint64_t, double, int, int, double, double*, int*);
    const ao_fn fn = WALK_PASS_KERNEL(ao_kernel, walk == 2, s.flat.xf_nest != 0u);
    const size_t smem = walk_pass_lds(view, walk, (const void*)fn);
    run_pixel_pass(s, "rt_ao_render", width, height, (int)cfg.ao_spp, walk, upload_ms, stream, st, [&](unsigned blocks, int* err) {
        hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), smem, stream, view, to_camk(cam), width, height, seed, t_min, (int)cfg.ao_spp, (int)cfg.rays_per_hit,
                           cfg.max_distance, d_out, err);
    });
}

void render_ao(const rt_scene& s, const CameraDev& cam, int width, int height, uint64_t seed, double t_min, int kernel, const rt_ao_config& cfg,
               double* out_host, rt_stats* st) {
    const size_t npix = (size_t)width * (size_t)height;
    DevBuf dout;
    dout.alloc(npix * 8 * sizeof(double));
    render_ao_device(s, cam, width, height, seed, t_min, kernel, cfg, (double*)dout.p, nullptr, st);
    dout.download(out_host, npix * 8 * sizeof(double));
}

void debug_occluded_device(const rt_scene& s, int walk, size_t n, const double* rays, double t_min, double* out) {
    const DeviceView dv = device_view(s);
    const FlatView& view = dv.view;
    typedef void (*occ_fn)(FlatView, size_t, const double*, double, double*);
    const occ_fn fn = WALK_PASS_KERNEL(occluded_kernel, walk == 2, s.flat.xf_nest != 0u);
    if (walk == 2 && !accel2_usable(view, 0., t_min, 64, dv.di.lds_max))
        throw RtError(RT_ERR_UNSUPPORTED, "the walk stacks of this scene do not fit in this device's LDS; use kernel 1");
    const size_t smem = walk_pass_lds(view, walk, (const void*)fn);
    DevBuf dr, dout;
    dout.alloc(n * sizeof(double));
    dr.upload(rays, n * 7 * sizeof(double));
    hipLaunchKernelGGL(fn, dim3((unsigned)((n + 63) / 64)), dim3(64), smem, 0, view, n, (const double*)dr.p, t_min, (double*)dout.p);
    HIP_CHECK(hipGetLastError());
    dout.download(out, n * sizeof(double));
}

}  // namespace rtamd
