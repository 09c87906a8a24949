// SPPM pre-pass on the GPU (included by kernels.hip; shares its device functions).
//
// The reference's SPPMIntegrator::new (integrator/photon_mapper.rs:139-233), per iteration:
//   generate_photon_map   :234-276   serial photon tracing + two kd-trees      -> photon_kernel + uniform grids
//   update_sppm per pixel :277-296   eye ray to the first Diffuse hit          -> eye_kernel
//   SPPM::update          :49-63     kNN / radius gather, progressive shrink   -> gather_kernel
// Photon maps are SETS here: photons are appended with an atomic cursor and binned into a uniform grid in
// whatever order the hardware produces, because every query result is order-independent by construction:
//   * the k-th nearest squared distance is found by bisection on the f64 bit pattern of d^2 (exact);
//   * counts are integers; flux terms are accumulated in 2^-S fixed point (int64), see DESIGN.md D6.
// That is also what makes the pre-pass bit-identical to the oracle's brute-force queries.
#pragma once

struct PhotonBuf {   // SoA, capacity `cap` photons
    double* pos;     // 3 per photon
    double* power;   // 3
    double* norm;    // 3
    unsigned int* count;  // atomic cursor
    unsigned int cap;
};
struct LightK {  // device copy of AllLights (light.rs:196-217)
    int n;
    double total;          // sum of the normalised |power| weights
    const double* cum;     // n cumulative weights
    const double* flux;    // 3 per light
    const double* scale;   // per light
};
struct SppmK {
    int width, height;
    int iteration;
    int photons_per_iter;
    int k_global, k_caustic, max_bounces;
    double alpha;
    uint64_t seed;
    int S;  // fixed-point shift of the flux accumulators
    int knn_cand;  // k-nearest selection: candidates kept in LDS (<= KNN_CAND; RTAMD_KNN_CAND lowers it to test the fallback)
};
static const uint64_t SALT_PHOTON = 0x50484F544F4E5F31ULL, SALT_EYE = 0x5350504D4559455FULL;

// MEDIA: the scene holds ConstantMedium objects, whose hit() draws from the path's stream (`rng`): the accel's media walk, or the
// reference-order walk with its media brackets.  Without MEDIA the stream is not touched.
template <bool ACCEL, int GENERAL = 1, bool MEDIA = false>
DEV Hit world_hit(const Acc& A, uint32_t n_media, uint32_t* stk, int stride, D3 o, D3 d, double t_min, Rng& rng) {
    if constexpr (MEDIA)
        return ACCEL ? traverse2_media<GENERAL, false, false>(A, n_media, stk, stride, o, d, t_min, rng) : traverse<GENERAL, true>(A, o, d, t_min, INFINITY, &rng);
    else
        return ACCEL ? traverse2<true, false, false>(A, stk, stride, o, d, t_min, INFINITY) : traverse<GENERAL>(A, o, d, t_min, INFINITY);  // (no LDS node cache in these kernels)
}

DEV void photon_push(const PhotonBuf& b, D3 p, D3 power, D3 n, int* err) {
    // one atomic per wave: the lanes that push together take consecutive slots (a single cursor serialises otherwise)
    const unsigned long long m = __ballot(1);
    const int lane = (int)(threadIdx.x & 63), leader = (int)__ffsll((long long)m) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(b.count, (unsigned int)__popcll(m));
    base = __shfl(base, leader);
    const unsigned int i = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
    if (i >= b.cap) {
        atomicOr(err, 2);  // buffer too small: the host retries the iteration with a larger one
        return;
    }
    b.pos[3 * (size_t)i] = p.x; b.pos[3 * (size_t)i + 1] = p.y; b.pos[3 * (size_t)i + 2] = p.z;
    b.power[3 * (size_t)i] = power.x; b.power[3 * (size_t)i + 1] = power.y; b.power[3 * (size_t)i + 2] = power.z;
    b.norm[3 * (size_t)i] = n.x; b.norm[3 * (size_t)i + 1] = n.y; b.norm[3 * (size_t)i + 2] = n.z;
}

// generate_photon_map, photon_mapper.rs:234-262.  Persistent waves: a wave takes PHOTON_CHUNK photon indices at a time from
// a global cursor and, as in pt_kernel, hands the next index of its chunk to every lane whose path ended (paths last
// 1..max_bounces segments), so the lanes stay busy.  A photon's RNG stream is keyed by its index: which lane traces it, and
// in which order the photons land in the buffers, changes nothing.
// LDS (with ACCEL): the accel's hot tables [stage2_begin, stage2_end) are staged into LDS in front of the stacks, as in pt_kernel
#ifndef RT_PHOTON_CHUNK
#define RT_PHOTON_CHUNK 256
#endif
static const unsigned int PHOTON_CHUNK = RT_PHOTON_CHUNK;
// (the body is shared with photon_kernel_nest: GENERAL == 3 is the chain walk of nested Transforms, kernels.hip)
// MEDIA: a volume event is a pass-through (Specular) interaction (D8): it stores no photon, marks the path has_specular, and the photon
// goes on from the scatter point.  The photon's one stream draws in trace_photons' order: emit, walk (a medium's free flight), scatter, roulette.
template <bool ACCEL, bool LDS, int GENERAL, bool MEDIA = false>
DEV void photon_body(FlatView sv, SppmK sk, LightK lk, PhotonBuf all, PhotonBuf caustic, unsigned int* cursor, int* err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Acc A;
    uint32_t hot = 0;
    if (ACCEL && LDS) {
        hot = sv.stage2_end - sv.stage2_begin;
        LDS_COPY16(smem, sv.base + sv.stage2_begin, hot / 16);
        __syncthreads();
        A = make_acc(smem - sv.stage2_begin, sv.base, sv);
        if (MEDIA) {  // the media's boundary subtrees are walked in the reference-order program, which is not staged (as in pt_kernel)
            A.meta = (const uint2*)(sv.base + sv.off_meta);
            A.boxes = (const double2*)(sv.base + sv.off_boxes);
        }
    } else {
        A = make_acc(sv.base, sv.base, sv);
    }
    uint32_t* stk = (uint32_t*)(smem + hot) + threadIdx.x;
    const int stride = (int)blockDim.x;
    const int lane = threadIdx.x & 63;
    const uint64_t lanemask_lt = (1ull << lane) - 1ull;
    const unsigned int n_photons = (unsigned int)sk.photons_per_iter;
    for (;;) {
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(cursor, PHOTON_CHUNK);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= n_photons) break;  // every wave reaches this: the cursor only grows
        const unsigned int pool_end = (n_photons - base < PHOTON_CHUNK) ? n_photons : base + PHOTON_CHUNK;
        unsigned int next = base;  // wave-uniform
        bool alive = false, has_specular = false, has_diffuse = false;
        int bounce = 0;
        D3 o = mk(0, 0, 0), d = mk(0, 0, 1), power = mk(0, 0, 0);
        Rng rng;
        rng.s = 0;
        for (;;) {
            // ---- regeneration: dead lanes take the next photon index of the chunk ----
            const uint64_t dead = __ballot(!alive);
            if (dead != 0ull && next < pool_end) {
                const unsigned int i = next + (unsigned int)__popcll(dead & lanemask_lt);
                const unsigned int adv = (unsigned int)__popcll(dead);
                next = (pool_end - next < adv) ? pool_end : next + adv;
                if (!alive && i < pool_end) {
                    rng.seed_stream(sk.seed ^ SALT_PHOTON, (uint64_t)sk.iteration * (uint64_t)sk.photons_per_iter + (uint64_t)i, 0);
                    // AllLights::emit (light.rs:220-225): WeightedIndex, then Light::emit
                    double chosen = rng.gen_range(0., lk.total);
                    int idx = 0;
                    while (idx + 1 < lk.n && lk.cum[idx] <= chosen) idx++;
                    uint2 l = A.lights[idx];
                    D3 flux = mk(lk.flux[3 * idx], lk.flux[3 * idx + 1], lk.flux[3 * idx + 2]);
                    double scale = lk.scale[idx];
                    if (l.x == NK_SPHERE) {  // SphereDiffuseLight::emit, light.rs:98-103
                        double2 c0 = A.spheres[2 * l.y], c1 = A.spheres[2 * l.y + 1];
                        D3 nrm = random_in_unit_sphere(rng);
                        o = add(mk(c0.x, c0.y, c1.x), muls(nrm, c1.y + 0.0001));
                        D3 s = random_in_unit_sphere(rng);  // random_in_hemisphere(&norm), vec3.rs:144-151
                        d = (dot(s, nrm) > 0.0) ? s : neg(s);
                        power = muls(flux, scale);
                    } else {  // XZRectLight::emit, light.rs:158-166
                        double2 r0 = A.rects[3 * l.y], r1 = A.rects[3 * l.y + 1], r2 = A.rects[3 * l.y + 2];
                        double u = rng.gen_range_01(), v = rng.gen_range_01();
                        o = mk(r0.x + (r1.x - r0.x) * u, r2.x, r0.y + (r1.y - r0.y) * v);
                        D3 s = random_in_unit_sphere(rng);
                        D3 dn = mk(0., -1., 0.);
                        d = (dot(s, dn) > 0.0) ? s : neg(s);
                        power = muls(muls(flux, scale), fmax(dot(dn, d), 0.));
                    }
                    has_specular = false;
                    has_diffuse = false;
                    bounce = 0;
                    alive = sk.max_bounces > 0;
                }
            }
            if (__ballot(alive) == 0ull) {
                if (next >= pool_end) break;
                continue;
            }
            // ---- one bounce of the photon loop, photon_mapper.rs:243-261 ----
            if (alive) {
                bool go = false;
                Hit h = world_hit<ACCEL, GENERAL, MEDIA>(A, sv.n_media, stk, stride, o, d, 0.0001, rng);
                if (h.node >= 0) {
                    Rec rec = materialize<GENERAL>(A, h, o, d, err);
                    // Material::scatter_photon, material.rs:27-45
                    D3 emitted, att, ndir;
                    bool diffuse;
                    bool scattered = shade(A, rec, d, rng, emitted, att, ndir, diffuse, err);
                    if (scattered) {  // else Absorb (no random number drawn)
                        double hmax = fmax(fmax(att.x, att.y), att.z);
                        if (!(rng.gen_f64() > hmax)) {  // Russian roulette: survive
                            D3 new_power = elemul(power, divs(att, hmax));
                            if (diffuse) {
                                photon_push(all, rec.p, power, rec.normal, err);
                                if (!has_diffuse && has_specular) photon_push(caustic, rec.p, power, rec.normal, err);
                                has_diffuse = true;
                            } else {
                                has_specular = true;
                            }
                            o = rec.p;
                            d = ndir;
                            power = new_power;
                            bounce += 1;
                            go = bounce < sk.max_bounces;
                        }
                    }
                }
                alive = go;
            }
        }
    }
}
template <bool ACCEL, bool LDS>
__global__ void __launch_bounds__(256, 4) photon_kernel(FlatView sv, SppmK sk, LightK lk, PhotonBuf all, PhotonBuf caustic, unsigned int* cursor,
                                                        int* err) {
    photon_body<ACCEL, LDS, 1>(sv, sk, lk, all, caustic, cursor, err);
}
__global__ void __launch_bounds__(256, 4) photon_kernel_nest(FlatView sv, SppmK sk, LightK lk, PhotonBuf all, PhotonBuf caustic, unsigned int* cursor,
                                                             int* err) {
    photon_body<false, false, 3>(sv, sk, lk, all, caustic, cursor, err);
}
// scenes with a ConstantMedium (kinds_mask has NK_MEDIUM_BEGIN): kernels of their own, so that nothing of the media walks is compiled into the above
template <bool ACCEL, bool LDS>
__global__ void __launch_bounds__(256, 4) photon_kernel_media(FlatView sv, SppmK sk, LightK lk, PhotonBuf all, PhotonBuf caustic, unsigned int* cursor,
                                                              int* err) {
    photon_body<ACCEL, LDS, 1, true>(sv, sk, lk, all, caustic, cursor, err);
}
__global__ void __launch_bounds__(256, 4) photon_kernel_nest_media(FlatView sv, SppmK sk, LightK lk, PhotonBuf all, PhotonBuf caustic, unsigned int* cursor,
                                                                   int* err) {
    photon_body<false, false, 3, true>(sv, sk, lk, all, caustic, cursor, err);
}

// ---- uniform grid over a photon set ----
struct GridK {
    double lo[3];       // grid origin
    double inv_cell;    // 1 / cell size
    double cell;
    int dim[3];
    const unsigned int* cell_start;  // dim0*dim1*dim2 + 1 offsets
    const unsigned int* index;       // photon indices grouped by cell
    unsigned int n;                  // photons in the map
};
DEV int grid_coord(const GridK& g, double x, int a) {
    double f = floor((x - g.lo[a]) * g.inv_cell);
    int c = (f < 0.) ? 0 : ((f > (double)(g.dim[a] - 1)) ? g.dim[a] - 1 : (int)f);
    return c;
}
// order-preserving map double -> uint64 for atomic min/max of the bounding box
DEV unsigned long long f64_key(double x) {
    unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__host__ __device__ inline double f64_unkey(unsigned long long k) {
    unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
    double d;
    memcpy(&d, &u, 8);
    return d;
}
__global__ void bbox_kernel(const double* pos, unsigned int n, unsigned long long* mnmx) {  // mnmx[0..2] = min keys, [3..5] = max keys
    __shared__ unsigned long long smn[3], smx[3];
    if (threadIdx.x < 3) {
        smn[threadIdx.x] = ~0ull;
        smx[threadIdx.x] = 0ull;
    }
    __syncthreads();
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        for (int a = 0; a < 3; a++) {
            unsigned long long k = f64_key(pos[3 * (size_t)i + a]);
            atomicMin(&smn[a], k);  // LDS atomics first, one global atomic per block and axis
            atomicMax(&smx[a], k);
        }
    __syncthreads();
    if (threadIdx.x < 3) {
        atomicMin(&mnmx[threadIdx.x], smn[threadIdx.x]);
        atomicMax(&mnmx[3 + threadIdx.x], smx[threadIdx.x]);
    }
}
__global__ void cell_count_kernel(const double* pos, unsigned int n, GridK g, unsigned int* counts, unsigned int* cell_of) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int cx = grid_coord(g, pos[3 * (size_t)i], 0), cy = grid_coord(g, pos[3 * (size_t)i + 1], 1), cz = grid_coord(g, pos[3 * (size_t)i + 2], 2);
    unsigned int c = ((unsigned int)cz * g.dim[1] + cy) * g.dim[0] + cx;
    cell_of[i] = c;
    atomicAdd(&counts[c], 1u);
}
// exclusive scan of `n` counters in three launches: per-block scan, scan of the block totals, add back
__global__ void scan_block_kernel(unsigned int* data, unsigned int n, unsigned int* block_sums) {
    __shared__ unsigned int tmp[1024];
    unsigned int i = blockIdx.x * 1024 + threadIdx.x;
    unsigned int v = (i < n) ? data[i] : 0u;
    tmp[threadIdx.x] = v;
    __syncthreads();
    for (unsigned int off = 1; off < 1024; off <<= 1) {
        unsigned int t = (threadIdx.x >= off) ? tmp[threadIdx.x - off] : 0u;
        __syncthreads();
        tmp[threadIdx.x] += t;
        __syncthreads();
    }
    if (i < n) data[i] = tmp[threadIdx.x] - v;  // exclusive
    if (threadIdx.x == 1023) block_sums[blockIdx.x] = tmp[1023];
}
__global__ void scan_sums_kernel(unsigned int* block_sums, unsigned int nb) {  // one block, serial over chunks of 1024
    __shared__ unsigned int tmp[1024];
    __shared__ unsigned int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (unsigned int base = 0; base < nb; base += 1024) {
        unsigned int i = base + threadIdx.x;
        unsigned int v = (i < nb) ? block_sums[i] : 0u;
        tmp[threadIdx.x] = v;
        __syncthreads();
        for (unsigned int off = 1; off < 1024; off <<= 1) {
            unsigned int t = (threadIdx.x >= off) ? tmp[threadIdx.x - off] : 0u;
            __syncthreads();
            tmp[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb) block_sums[i] = carry + tmp[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += tmp[1023];
        __syncthreads();
    }
}
__global__ void scan_add_kernel(unsigned int* data, unsigned int n, const unsigned int* block_sums, unsigned int total_slot) {
    unsigned int i = blockIdx.x * 1024 + threadIdx.x;
    if (i < n) data[i] += block_sums[blockIdx.x];
    (void)total_slot;
}
__global__ void cell_fill_kernel(unsigned int n, const unsigned int* cell_of, const unsigned int* cell_start, unsigned int* cursor, unsigned int* index) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned int c = cell_of[i];
    unsigned int slot = cell_start[c] + atomicAdd(&cursor[c], 1u);
    index[slot] = i;
}

// update_sppm's eye path, photon_mapper.rs:277-296 ; one pixel per thread.  gp: per pixel {valid, p[3], bsdf[3]}
// (the body is shared with eye_kernel_nest: GENERAL == 3 is the chain walk of nested Transforms, kernels.hip)
// MEDIA: the eye stream goes on after the camera's draws into the walks (a medium's free flight) and the scatters; volume events are
// passed through to the first Diffuse hit.
template <bool ACCEL, int GENERAL, bool MEDIA = false>
DEV void eye_body(FlatView sv, const CamK* __restrict__ camp, SppmK sk, double* gp, int* err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Acc A = make_acc(sv.base, sv.base, sv);
    uint32_t* stk = (uint32_t*)smem + threadIdx.x;
    const int stride = (int)blockDim.x;
    const size_t npix = (size_t)sk.width * sk.height;
    for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(pix % sk.width), y = (int)(pix / sk.width);
        const CamK cam = *camp;
        Rng rng;
        rng.seed_stream(sk.seed ^ SALT_EYE, (uint64_t)pix, (uint64_t)sk.iteration);
        // camera_draw() + camera_ray(), written out
        double u = ((double)x + rng.gen_f64()) / (double)(sk.width - 1);
        double v = ((double)y + rng.gen_f64()) / (double)(sk.height - 1);
        double st = 1.0 - v;
        D3 rd = muls(random_in_unit_disk(rng), cam.lens_radius);
        D3 offset = add(muls(cam.u, rd.x), muls(cam.v, rd.y));
        D3 o = add(cam.origin, offset);
        D3 d = sub(sub(add(add(cam.llc, muls(cam.horizontal, u)), muls(cam.vertical, st)), cam.origin), offset);
        double* g = gp + 7 * pix;
        g[0] = 0.;
        for (int bounce = 0; bounce < sk.max_bounces; bounce++) {
            Hit h = world_hit<ACCEL, GENERAL, MEDIA>(A, sv.n_media, stk, stride, o, d, 0.001, rng);
            if (h.node < 0) break;
            Rec rec = materialize<GENERAL>(A, h, o, d, err);
            D3 emitted, att, ndir;
            bool diffuse;
            bool scattered = shade(A, rec, d, rng, emitted, att, ndir, diffuse, err);
            if (diffuse) {  // (Diffuse, _, _): the gather point ; bsdf(., rec) == the attenuation scatter reports
                g[0] = 1.;
                g[1] = rec.p.x; g[2] = rec.p.y; g[3] = rec.p.z;
                g[4] = att.x; g[5] = att.y; g[6] = att.z;
                break;
            }
            if (!scattered) break;
            o = rec.p;
            d = ndir;
        }
    }
}
template <bool ACCEL>
__global__ void __launch_bounds__(256) eye_kernel(FlatView sv, const CamK* __restrict__ camp, SppmK sk, double* gp, int* err) {
    eye_body<ACCEL, 1>(sv, camp, sk, gp, err);
}
__global__ void __launch_bounds__(256) eye_kernel_nest(FlatView sv, const CamK* __restrict__ camp, SppmK sk, double* gp, int* err) {
    eye_body<false, 3>(sv, camp, sk, gp, err);
}
template <bool ACCEL>
__global__ void __launch_bounds__(256) eye_kernel_media(FlatView sv, const CamK* __restrict__ camp, SppmK sk, double* gp, int* err) {
    eye_body<ACCEL, 1, true>(sv, camp, sk, gp, err);
}
__global__ void __launch_bounds__(256) eye_kernel_nest_media(FlatView sv, const CamK* __restrict__ camp, SppmK sk, double* gp, int* err) {
    eye_body<false, 3, true>(sv, camp, sk, gp, err);
}

struct Fixed3 {
    long long x, y, z;
};
// photon arrays in GRID ORDER (cell-major; permute_kernel): a cell's photons, and the cells of one x-row, are contiguous
struct PhotonSorted {
    const double* pos;
    const double* power;
    const double* norm;
};
__global__ void permute_kernel(unsigned int n, const unsigned int* index, PhotonBuf src, double* dpos, double* dpower, double* dnorm) {
    unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    size_t i = index[k];
    for (int a = 0; a < 3; a++) {
        dpos[3 * (size_t)k + a] = src.pos[3 * i + a];
        dpower[3 * (size_t)k + a] = src.power[3 * i + a];
        dnorm[3 * (size_t)k + a] = src.norm[3 * i + a];
    }
}

// ---- wave-level reductions (integers and max only: every result is independent of the order of the photons) ----
DEV unsigned int wave_sum_u32(unsigned int v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
DEV long long wave_sum_i64(long long v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
DEV double wave_max_f64(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
// one photon's term: elemul(bsdf, power) * (1 - disk_factor)  (photon_mapper.rs:77-79, 95-97, 109-111)
DEV void photon_term(const PhotonSorted& ps, unsigned int k, D3 p, D3 bsdf, int S, Fixed3& acc, int* err) {
    D3 pp = mk(ps.pos[3 * (size_t)k], ps.pos[3 * (size_t)k + 1], ps.pos[3 * (size_t)k + 2]);
    D3 pw = mk(ps.power[3 * (size_t)k], ps.power[3 * (size_t)k + 1], ps.power[3 * (size_t)k + 2]);
    D3 pn = mk(ps.norm[3 * (size_t)k], ps.norm[3 * (size_t)k + 1], ps.norm[3 * (size_t)k + 2]);
    double df = fabs(dot(pn, unit(sub(pp, p), err)));
    D3 t = muls(elemul(bsdf, pw), 1. - df);
    acc.x += __double2ll_rn(ldexp(t.x, S));
    acc.y += __double2ll_rn(ldexp(t.y, S));
    acc.z += __double2ll_rn(ldexp(t.z, S));
}
// The WAVE visits every photon of the cells overlapping the cube [p - r, p + r]: F(k, d2) runs once per photon, on
// whichever lane the photon falls to.  Rows (fixed y, z; the cells x0..x1 are one contiguous run of the sorted arrays)
// are taken 64 at a time, one per lane; an inclusive scan of the run lengths flattens them into one item list that
// the lanes stride over, finding an item's row by a 6-step binary search over the scan (ds_bpermute).
// p, r and the control flow are wave-uniform; callers reduce what F accumulated with the wave_* helpers.
template <class F>
DEV void coop_visit(const GridK& g, const PhotonSorted& ps, D3 p, double r, int lane, F f) {
    const int x0 = grid_coord(g, p.x - r, 0), x1 = grid_coord(g, p.x + r, 0);
    const int y0 = grid_coord(g, p.y - r, 1), y1 = grid_coord(g, p.y + r, 1);
    const int z0 = grid_coord(g, p.z - r, 2), z1 = grid_coord(g, p.z + r, 2);
    const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
    for (int rbase = 0; rbase < nrows; rbase += 64) {
        const int ri = rbase + lane;
        unsigned int b = 0, len = 0;
        if (ri < nrows) {
            const int z = z0 + ri / ny, y = y0 + ri % ny;
            const unsigned int row = ((unsigned int)z * g.dim[1] + y) * g.dim[0];
            b = g.cell_start[row + x0];
            len = g.cell_start[row + x1 + 1] - b;
        }
        unsigned int incl = len;  // inclusive scan over the lanes
        for (int off = 1; off < 64; off <<= 1) {
            unsigned int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        const unsigned int total = __shfl(incl, 63);
        for (unsigned int t = 0; t < total; t += 64) {
            const unsigned int item = t + lane;
            int L = 0;  // first lane whose inclusive sum exceeds item
            for (int step = 32; step >= 1; step >>= 1) {
                unsigned int v = __shfl(incl, (L + step - 1) & 63);
                if (v <= item) L += step;
            }
            const unsigned int bL = __shfl(b, L & 63), inclL = __shfl(incl, L & 63), lenL = __shfl(len, L & 63);
            if (item < total) {
                const unsigned int k = bL + (item - (inclL - lenL));
                D3 q = mk(ps.pos[3 * (size_t)k] - p.x, ps.pos[3 * (size_t)k + 1] - p.y, ps.pos[3 * (size_t)k + 2] - p.z);
                f(k, sqlen(q));
            }
        }
    }
}
static const int KNN_CAND = 1024;  // candidate squared distances a wave keeps in LDS for the k-nearest selection
// SPPM::update (photon_mapper.rs:49-63) for one map, by one wave; st = {flux[3], radius2, photons}; cand: KNN_CAND doubles of LDS
DEV void sppm_update_dev(double* st, const GridK& g, const PhotonSorted& ps, D3 p, D3 bsdf, int k_init, double alpha, int S, int lane,
                         double* cand, int knn_cand, int* err) {
    const double photons = st[4];
    if (photons == 0.) {
        // estimate_flux_by_count: the k nearest photons (all of them if the map holds fewer)
        Fixed3 acc = {0, 0, 0};
        double radius2 = 0.;
        if (g.n > 0) {
            const unsigned int kk = ((unsigned int)k_init < g.n) ? (unsigned int)k_init : g.n;
            // 1. grow a search radius until it holds >= kk photons (a cube reaching past the grid holds them all)
            double span = fmax(fmax(g.dim[0], g.dim[1]), g.dim[2]) * g.cell;
            double dist_out = 0.;  // how far p lies outside the grid
            dist_out = fmax(dist_out, fmax(g.lo[0] - p.x, p.x - (g.lo[0] + g.dim[0] * g.cell)));
            dist_out = fmax(dist_out, fmax(g.lo[1] - p.y, p.y - (g.lo[1] + g.dim[1] * g.cell)));
            dist_out = fmax(dist_out, fmax(g.lo[2] - p.z, p.z - (g.lo[2] + g.dim[2] * g.cell)));
            const double r_all = 2. * (span + dist_out) + g.cell;  // every photon is within this distance of p
            double r = g.cell;
            unsigned int n_in = 0;  // photons with d^2 <= r^2
            for (;;) {
                unsigned int cnt = 0;
                const double r2 = r * r;
                coop_visit(g, ps, p, r, lane, [&](unsigned int, double d2) { cnt += (d2 <= r2) ? 1u : 0u; });
                n_in = wave_sum_u32(cnt);
                if (n_in >= kk || r >= r_all) break;
                r = fmin(2. * r, r_all);
            }
            // 2. the kk-th smallest d^2 among the photons with d^2 <= r^2, by bisection on the f64 bit pattern (exact and
            //    independent of the photon order).  The candidates are gathered into LDS once when they fit.
            const bool in_lds = n_in <= (unsigned int)knn_cand;
            if (in_lds) {  // append through an LDS cursor: the order is arbitrary, the selection below does not depend on it
                const double r2 = r * r;
                coop_visit(g, ps, p, r, lane, [&](unsigned int, double d2) {
                    if (d2 <= r2) cand[atomicAdd((unsigned int*)&cand[KNN_CAND], 1u)] = d2;
                });
                __threadfence_block();
                __builtin_amdgcn_wave_barrier();
            }
            unsigned long long lo = 0ull, hi = (unsigned long long)__double_as_longlong(r * r);
            double r2k = -1.;
            while (lo < hi) {
                unsigned long long mid = lo + ((hi - lo) >> 1);
                double m = __longlong_as_double((long long)mid);
                unsigned int cnt = 0;
                double below = 0.;  // largest d^2 <= m
                if (in_lds) {
                    for (unsigned int j = lane; j < n_in; j += 64) {
                        double d2 = cand[j];
                        if (d2 <= m) {
                            cnt++;
                            below = fmax(below, d2);
                        }
                    }
                } else {
                    coop_visit(g, ps, p, r, lane, [&](unsigned int, double d2) {
                        if (d2 <= m) {
                            cnt++;
                            below = fmax(below, d2);
                        }
                    });
                }
                cnt = wave_sum_u32(cnt);
                if (cnt == kk) {  // exactly the kk nearest lie below m: the kk-th distance is their maximum
                    r2k = wave_max_f64(below);
                    break;
                }
                if (cnt > kk) hi = mid;
                else lo = mid + 1;
            }
            if (r2k < 0.) r2k = __longlong_as_double((long long)lo);
            // 3. sum the photons within r2k
            coop_visit(g, ps, p, r, lane, [&](unsigned int k, double d2) {
                if (d2 <= r2k) {
                    radius2 = fmax(radius2, d2);
                    photon_term(ps, k, p, bsdf, S, acc, err);
                }
            });
            radius2 = wave_max_f64(radius2);
            acc.x = wave_sum_i64(acc.x);
            acc.y = wave_sum_i64(acc.y);
            acc.z = wave_sum_i64(acc.z);
        }
        if (lane == 0) {
            st[4] = (double)k_init;
            st[0] = ldexp((double)acc.x, -S);
            st[1] = ldexp((double)acc.y, -S);
            st[2] = ldexp((double)acc.z, -S);
            st[3] = radius2;
        }
    } else {
        // estimate_flux_within_radius(rec, sqrt(radius2)): photons with d^2 < r*r
        const double radius = sqrt(st[3]);
        const double rr = radius * radius;
        Fixed3 acc = {0, 0, 0};
        unsigned int found_l = 0;
        if (g.n > 0)
            coop_visit(g, ps, p, radius, lane, [&](unsigned int k, double d2) {
                if (d2 < rr) {
                    found_l++;
                    photon_term(ps, k, p, bsdf, S, acc, err);
                }
            });
        const unsigned long long found = (unsigned long long)wave_sum_u32(found_l);
        acc.x = wave_sum_i64(acc.x);
        acc.y = wave_sum_i64(acc.y);
        acc.z = wave_sum_i64(acc.z);
        if (lane == 0) {
            D3 flux = mk(ldexp((double)acc.x, -S), ldexp((double)acc.y, -S), ldexp((double)acc.z, -S));
            unsigned long long prev = (unsigned long long)photons;
            unsigned long long now = prev + (unsigned long long)(alpha * (double)found);
            double frac = (double)now / (double)(prev + found);
            st[4] = (double)now;
            st[3] = st[3] * frac;
            st[0] = (st[0] + flux.x) * frac;
            st[1] = (st[1] + flux.y) * frac;
            st[2] = (st[2] + flux.z) * frac;
        }
    }
}
// per pixel (one WAVE each): caustic update, then global update (photon_mapper.rs:284-285).  stats: per pixel {global[5], caustic[5]}
static const int GATHER_BLOCK = 256;
__global__ void __launch_bounds__(GATHER_BLOCK) gather_kernel(SppmK sk, const double* gp, GridK gg, PhotonSorted pg, GridK gc, PhotonSorted pc,
                                                              double* stats, int* err) {
    __shared__ double cand_all[(GATHER_BLOCK / 64) * (KNN_CAND + 1)];  // per wave: candidates + an append cursor
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* cand = cand_all + wv * (KNN_CAND + 1);
    const size_t pix = (size_t)blockIdx.x * (GATHER_BLOCK / 64) + wv;
    if (pix >= (size_t)sk.width * sk.height) return;
    const double* g = gp + 7 * pix;
    if (g[0] == 0.) return;
    D3 p = mk(g[1], g[2], g[3]), bsdf = mk(g[4], g[5], g[6]);
    double* st = stats + 10 * pix;
    for (int m = 0; m < 2; m++) {
        if (lane == 0) *(unsigned int*)&cand[KNN_CAND] = 0u;
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        if (m == 0) sppm_update_dev(st + 5, gc, pc, p, bsdf, sk.k_caustic, sk.alpha, sk.S, lane, cand, sk.knn_cand, err);
        else sppm_update_dev(st, gg, pg, p, bsdf, sk.k_global, sk.alpha, sk.S, lane, cand, sk.knn_cand, err);
    }
}
// adjust_flux, photon_mapper.rs:117-119: flux / (PI * radius2 * N) per pixel -> {caustic[3], global[3]}
__global__ void estimate_kernel(const double* stats, size_t npix, double n_emitted, double* est) {
    size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const double PI = 3.14159265358979323846264338327950288;
    const double* st = stats + 10 * pix;
    double dg = PI * st[3] * n_emitted, dc = PI * st[8] * n_emitted;
    double* e = est + 6 * pix;
    e[0] = st[5] / dc; e[1] = st[6] / dc; e[2] = st[7] / dc;
    e[3] = st[0] / dg; e[4] = st[1] / dg; e[5] = st[2] / dg;
}
