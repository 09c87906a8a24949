// Kernel 6: the wavefront instance service -- kernel 5's idea (walks through LARGE mesh instances taken out of the path-tracing
// lanes and packed densely) with the packing done across the WHOLE GPU and across kernel launches instead of inside a workgroup.
// Included by kernels.hip (uses its Acc / traverse2 / materialize / shade / next_unit / blas_pass_q).
//
// A frame is rendered in CYCLES of two launches on one stream:
//   pt_kernel_wf   (1024-thread workgroups, one per CU, the path state of 1024 paths in registers): generate, world-space walk
//                  with instance items deferred, entry walk through the LDS-cached top of the instance's BVH, shade -- kernel
//                  5's loop without its serve passes.  A path whose ray needs a node or a leaf of an instance from memory is
//                  PARKED: its whole state (14 sixteen-byte units, WF_REC_U) goes to the next free record of the workgroup's
//                  segment of pool B in HBM and the lane is free at once; free lanes ADOPT the records of pool A -- the paths
//                  this workgroup parked one cycle earlier, answered by the walk launch in between -- before they generate new paths.
//   wf_walk_kernel (512-thread workgroups, 16 waves per CU, ~90 VGPRs): nothing but object-space walks.  Waves take the parked
//                  records in chunks of 256 from a global cursor, 64 walks per wave at all times (a lane that finishes takes
//                  the next record at once), NodeQ / Tri32 with the f64 Triangle::hit exactly as kernel 5's serving waves;
//                  a path with several deferred instances is walked through all of them here, one after the other.  The answer
//                  -- closest hit so far after the instances -- goes back into the record.
// then A and B swap.  Nothing spins on anything: the launches are ordered by the stream, a record is written by one kernel and
// read by the next.  The pools live in HBM because they can (2 x 256 workgroups x 16 384 records x 224 B = 1.9 GB of 288 GB):
// with ~4 M paths parked per cycle the walk launch never runs thin, which is what kernel 5's 1 024 paths per workgroup could not
// give (its serve passes ran at 42 of 64 lanes with 54 % of the wave cycles spent waiting).
//
// No pool can overflow: a workgroup generates new paths only while  parked(B) + still-to-adopt(A) + 2 048 <= segment  (every live
// lane can park at most once more before the launch ends, and the check is at most one iteration of each of the 16 waves old),
// adoption is always allowed (it moves a path from A to a lane), and each launch ends when its lanes are empty and nothing is
// left to adopt or allowed to start.  Progress: every cycle answers every parked path.
// Ordered accumulation is the ring / ticket scheme of the other kernels with longer rings (a unit stays open for as many cycles as
// its slowest path needs walks) and its LDS bookkeeping saved to / restored from global memory at the launch boundaries; a path
// is finished by a wave of the workgroup that generated it (adoption is per workgroup), so the unit counters stay in LDS.
// Results are those of kernels 2 and 5 bit for bit, for the reasons given above pt_kernel_coop.
#ifndef WF_RING_UNITS
#define WF_RING_UNITS 96               // unit buffers per wave (12 KB each; 4.8 GB for 4 096 waves).  A unit stays open until its slowest
#endif                                 // path is through -- one CYCLE per walk it needs, up to 50 -- and samples must be folded in order, so
                                       // the ring has to hold what a wave generates meanwhile (16 units: 134 Msamples/s on C4, the waves sat on full rings)
static const int WF_SLOT_BITS = 16;    // ring slot * 512 + sample * 64 + pixel < 2^16
static const int WF_REC_U = 14;        // 16-byte units per record
static const uint32_t WF_SEG_DEFAULT = 32768;  // records per workgroup segment (a multiple of WF_CHUNK)
static const uint32_t WF_CHUNK = 256;  // records a walking wave takes from the global cursor at a time
static const uint32_t WF_GATE = 2048;  // see "No pool can overflow"
static const int WF_ENTRY_STACK = 8;   // stack entries an entry walk may park (it stops descending when it would need a ninth)
static const int WF_MAX_INST = 64;     // one pending bit per instance
#ifndef WF_WALK_BLOCK
#define WF_WALK_BLOCK 512
#endif
// record, in 16-byte units (u64 pairs):
//   0..2  o, d in WORLD space
//   3     best t so far | kind|payload << 32 | order          (as posted; the walk starts from it)
//   4     node to continue at << 32 | xform of the best hit so far + 1        | instances still deferred after `inst` (64 bits)
//   5     sample slot (owner wave << 16 | ring slot * 512 + sample * 64 + pixel) | inst << 32 | stack entries saved << 40      | -
//   6,7   the saved stack of the entry walk (<= 8 entries)
//   8     ANSWER: t | kind|payload << 32 | order                (written by the walk launch)
//   9     ANSWER: xform of the closest hit + 1                  | rng
//   10..12 beta, L      13  depth << 32 | pix_id | -
struct WfArgs {
    U2* pool_a;             // records to adopt (parked one cycle earlier, answered since): [grid][seg][WF_REC_U]
    U2* pool_b;             // records parked by this launch
    const uint32_t* cnt_a;  // [grid]
    uint32_t* cnt_b;        // [grid]
    uint32_t* book;         // [grid][WF_BOOK_WORDS]: the LDS bookkeeping between launches
    uint32_t* unfinished;   // this cycle's count of workgroups that are not done with the frame
    uint32_t seg;
    int first;              // first cycle of the launch series: bookkeeping starts empty
    uint32_t ring_units;    // unit buffers per wave in HBM (<= WF_RING_UNITS): what the launch can use, within the workspace budget
};
#ifdef RTAMD_WF_STATS  // tools-only build (tools/build_variant.sh wfstats -DRTAMD_WF_STATS): schedule counters of kernel 6
__device__ unsigned long long g_wf_stats[16];
#define WF_STAT(i, v) wfs[i] += (unsigned long long)(v)
#else
#define WF_STAT(i, v) \
    do {              \
    } while (0)
#endif
static const int WF_WST = 16;  // per-wave job / ring state: next_unit()'s 8 words + the unit being generated {pool, next, s0, tx, ty, cur_slot}
static const int WF_BOOK_WORDS = (PT_BLOCK / 64) * (WF_RING_UNITS * 4 + WF_WST);

// next_unit() for kernel 6: the wave's unit buffers are a POOL, not a FIFO.  A unit stays open for as many cycles as its slowest
// path needs walks and a complete unit can only be folded when its tile's ticket has reached it, so with a FIFO one old unit at
// the head kept every later one from being folded and the wave from starting new ones (the first version: the waves sat on full
// rings).  Here every complete unit whose turn it is gets folded, whichever slot it is in, and a new unit takes any free slot.
// Jobs are single units.  rmeta per slot: {tile (local), sample block, samples | 0x100 (slot in use), paths still running};
// wst: [1] slots in use, [6] jobs left.
__device__ __attribute__((noinline)) UnitInfo next_unit_wf(uint32_t* wst, uint32_t* rmeta, const int* cfg, const double* wring, double* accum,
                                                           unsigned int* tickets, unsigned int* counter, int lane) {
    int n_used = (int)wst[1];
    bool more_jobs = wst[6] != 0u;
    const bool first_launch = cfg[CFG_S_BEGIN] == 0;
    const int ring_units = cfg[CFG_RING_UNITS];  // unit buffers this launch gives a wave (<= WF_RING_UNITS, which sizes the LDS bookkeeping)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's sample stores are in L2
    for (int round = 0; round < 4 && n_used > 0; round++) {  // (a fold can make the tile's next block foldable: look again, a few times)
        bool any = false;
        for (int base = 0; base < ring_units; base += 64) {
            const int slot = base + lane;
            bool can = false;
            if (slot < ring_units) {
                const uint32_t* m = rmeta + 4 * slot;
                if ((m[2] & 0x100u) != 0u && __hip_atomic_load(&m[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u)
                    can = __hip_atomic_load(&tickets[m[0]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == m[1];
            }
            uint64_t mask = __ballot(can);
            while (mask != 0ull) {
                const int sl = base + __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                FOLD_POOL_SLOT(uint32_t, uint64_t, ld_agent, st_agent, tickets, sl);
                n_used--;
                any = true;
            }
        }
        if (!any) break;
    }
    UnitInfo u;
    u.pool = 0; u.s0 = 0; u.tx = 0; u.ty = 0; u.cur_slot = 0; u.finished = 0;
    if (n_used < ring_units && more_jobs) {
        unsigned int job = 0;
        if (lane == 0) job = atomicAdd(counter, 1u);
        job = __builtin_amdgcn_readfirstlane(job);
        if (job >= (unsigned)cfg[CFG_N_JOBS]) {
            more_jobs = false;
        } else {
            const int job_tile = (int)(job % (unsigned)cfg[CFG_TILES_OWNED]);  // sample-major: all tiles' block k before any tile's block k+1
            const int sub_i = (int)(job / (unsigned)cfg[CFG_TILES_OWNED]);
            int slot = -1;
            for (int base = 0; base < ring_units && slot < 0; base += 64) {
                const int sl = base + lane;
                const uint64_t fm = __ballot(sl < ring_units && (rmeta[4 * sl + 2] & 0x100u) == 0u);
                if (fm != 0ull) slot = base + __ffsll((long long)fm) - 1;
            }
            const int tile = job_tile * cfg[CFG_WORLD] + cfg[CFG_RANK];
            u.tx = tile % cfg[CFG_TILES_X];
            u.ty = tile / cfg[CFG_TILES_X];
            u.s0 = cfg[CFG_S_BEGIN] + sub_i * cfg[CFG_SUB_SPP];
            const int s1 = min(u.s0 + cfg[CFG_SUB_SPP], cfg[CFG_S_END]);
            u.pool = (s1 - u.s0) * TILE_PIX;
            u.cur_slot = slot;
            n_used++;
            if (lane == 0) {
                uint32_t* m = rmeta + 4 * slot;
                m[0] = (uint32_t)job_tile;
                m[1] = (uint32_t)sub_i;
                m[2] = (uint32_t)(s1 - u.s0) | 0x100u;
                const int w_in = min(TILE_W, cfg[CFG_WIDTH] - u.tx * TILE_W), h_in = min(TILE_H, cfg[CFG_HEIGHT] - u.ty * TILE_H);
                __hip_atomic_store(&m[3], (uint32_t)((s1 - u.s0) * w_in * h_in), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    u.finished = (u.pool == 0 && !more_jobs && n_used == 0) ? 1 : 0;
    if (lane == 0) {
        wst[1] = (uint32_t)n_used;
        wst[4] = 0u;
        wst[5] = 0u;
        wst[6] = more_jobs ? 1u : 0u;
    }
    return u;
}

// TIE: the exact-tie rule, as in pt_kernel_coop (the walk launch returns the flag in the answer's order word: tie_order)
template <int INTEG, bool MIXED = false, bool TIE = false>
__global__ void __launch_bounds__(PT_BLOCK) pt_kernel_wf(FlatView sv, CamK cam, RenderK rk, double* __restrict__ ring, double* accum,
                                                         unsigned int* tickets, unsigned int* __restrict__ counter, int* __restrict__ err, WfArgs wa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS map: [world-level tables][top-of-BVH Node2 cache (world-space walk)][NodeQ cache (entry walk)][stacks][ring / job
    //          bookkeeping][8 counters]
    uint32_t staged = 0;
    Acc A = make_acc(sv.base, sv.base, sv);
    const double* qgrid_lds = nullptr;
    {
        auto stage = [&](uint32_t off, uint32_t bytes) {
            LDS_COPY16(smem + staged, sv.base + off, coop_a16(bytes) / 16);
            const char* at = smem + staged;
            staged += coop_a16(bytes);
            return at;
        };
        A.spheres = (const double2*)stage(sv.off_spheres, sv.off_rects - sv.off_spheres);
        A.rects = (const double2*)stage(sv.off_rects, sv.off_tris - sv.off_rects);
        A.xforms = (const double*)stage(sv.off_xforms, sv.stage_bytes - sv.off_xforms);
        A.inst2 = (const uint2*)stage(sv.off_inst2, 8u * sv.n_inst2);
        A.items2 = (const uint2*)stage(sv.off_items2, 8u * sv.n_world_items2);  // world leaves only: instances are deferred
        qgrid_lds = (const double*)stage(sv.off_qgrid, (uint32_t)sizeof(QGrid) * sv.n_inst2);
    }
    if (rk.n_top > 0) {
        LDS_COPY16(smem + staged, sv.base + sv.off_n2, (uint32_t)rk.n_top * NODE2_F4);
        A.n2_top = (const AS_L f32x4*)(smem + staged);
        A.n2_top_count = (uint32_t)rk.n_top;
        staged += (uint32_t)rk.n_top * (uint32_t)sizeof(Node2);
    }
    const uint4* n2q_lds = (const uint4*)(smem + staged);
    const uint32_t entry_top = (uint32_t)rk.n_topq;  // NodeQ indices below this are walked by the parking lane itself
    LDS_COPY16(smem + staged, sv.base + sv.off_n2q, (uint32_t)rk.n_topq * 2u);
    staged += (uint32_t)rk.n_topq * (uint32_t)sizeof(NodeQ);
    uint32_t* stk = (uint32_t*)(smem + staged) + threadIdx.x;
    const int stk_stride = (int)blockDim.x;
    const int lane = threadIdx.x & 63;
    const uint64_t lanemask_lt = (1ull << lane) - 1ull;
    const int wave = threadIdx.x >> 6;
    uint32_t* book = (uint32_t*)(smem + staged + walk_stack_bytes((uint32_t)rk.coop_stack, PT_BLOCK));
    uint32_t* rmeta = book + (size_t)wave * WF_RING_UNITS * 4;
    uint32_t* wst = book + (size_t)(PT_BLOCK / 64) * WF_RING_UNITS * 4 + (size_t)wave * WF_WST;
    int* cfg = (int*)(book + WF_BOOK_WORDS);
    AS_L uint32_t* wfc = (AS_L uint32_t*)(cfg + CFG_WORDS);  // {parked into B, adopted from A (may overshoot n_a), n_a}
    uint32_t* book_save = wa.book + (size_t)blockIdx.x * WF_BOOK_WORDS;
    if (wa.first) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)WF_BOOK_WORDS; i += blockDim.x) book[i] = 0u;
        __syncthreads();
        if (lane < 8) wst[lane] = (lane == 6) ? 1u : 0u;  // nothing in flight, no job yet, jobs left
    } else {
        for (uint32_t i = threadIdx.x; i < (uint32_t)WF_BOOK_WORDS; i += blockDim.x) book[i] = book_save[i];
    }
    if (threadIdx.x == 0) {
        fill_cfg(cfg, rk, (int)wa.ring_units);
        wfc[0] = 0u;
        wfc[1] = 0u;
        wfc[2] = wa.first ? 0u : wa.cnt_a[blockIdx.x];
    }
    __syncthreads();
    const uint32_t n_a = wfc[2];
    double* bring = ring + (size_t)blockIdx.x * (PT_BLOCK / 64) * wa.ring_units * UNIT_DOUBLES;  // the workgroup's rings, wave-major
    double* wring = bring + (size_t)wave * wa.ring_units * UNIT_DOUBLES;
    const AS_G U2* seg_a = (const AS_G U2*)(wa.pool_a + (size_t)blockIdx.x * wa.seg * WF_REC_U);
    AS_G U2* seg_b = (AS_G U2*)(wa.pool_b + (size_t)blockIdx.x * wa.seg * WF_REC_U);

    // the unit this wave was generating when the previous launch ended (the gate can close in the middle of a unit)
    int pool = (int)wst[8], next = (int)wst[9], s0 = (int)wst[10], tx = (int)wst[11], ty = (int)wst[12], cur_slot = (int)wst[13];
    bool finished = false;

    bool alive = false;   // the lane holds a path
    bool ready = false;   // ... whose closest hit is known (shade next); otherwise it needs its world-space walk
    D3 o = mk(0, 0, 0), d = mk(0, 0, 1), beta = mk(1, 1, 1), L = mk(0, 0, 0);
    int depth = 0, pix_id = 0;
    uint32_t out_slot = 0;  // owner wave << WF_SLOT_BITS | (ring slot * UNIT_SPP + sample within the unit) * 64 + pixel
    uint64_t pend = 0ull;
    int dec_slot = -1;      // a finished path whose unit counter still has to be decremented
    Rng rng;
    rng.s = 0;
    Hit h;
    h.t = INFINITY; h.node = -1; h.xf = -1; h.kp = 0;
#ifdef RTAMD_WF_STATS
    unsigned long long wfs[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
#endif

    for (;;) {
        WF_STAT(3, 1);
        WF_STAT(8, __popcll(__ballot(alive)));
        // ---- unit counters of the paths finished last iteration: their sample stores have completed by now ----
        if (__ballot(dec_slot >= 0) != 0ull) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (dec_slot >= 0) {
                atomicSub(book + (size_t)(dec_slot >> WF_SLOT_BITS) * WF_RING_UNITS * 4 + 4 * ((dec_slot & ((1 << WF_SLOT_BITS) - 1)) >> 9) + 3, 1u);
                dec_slot = -1;
            }
        }
        // ---- free lanes adopt the answered paths of pool A first ----
        {
            uint64_t fr = __ballot(!alive);
            if ((int)__popcll(fr) < COOP_ADOPT_MIN && fr != ~0ull) fr = 0ull;
            if (fr != 0ull && lds_load(&wfc[1]) < n_a) {
                uint32_t base = 0;
                if (lane == 0) base = __hip_atomic_fetch_add(&wfc[1], (uint32_t)__popcll(fr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                base = __builtin_amdgcn_readfirstlane(base);
                const uint32_t idx = base + (uint32_t)__popcll(fr & lanemask_lt);
                if (!alive && idx < n_a) {
                    const AS_G U2* q = seg_a + (size_t)idx * WF_REC_U;
                    const U2 u0 = q[0], u1 = q[1], u2 = q[2], u5 = q[5], u8 = q[8], u9 = q[9];
                    const U2 u10 = q[10], u11 = q[11], u12 = q[12], u13 = q[13];
                    h.t = bitsd(u8.x);
                    h.node = (int)(uint32_t)u8.y;
                    const bool a_tied = TIE && tie_flagged(h.node);  // the walks met a triangle at exactly the best t
                    if (a_tied) h.node ^= TIE_FLAG;
                    h.kp = (uint32_t)(u8.y >> 32);
                    h.xf = (int)(uint32_t)u9.x - 1;
                    o = mk(bitsd(u0.x), bitsd(u0.y), bitsd(u1.x));
                    d = mk(bitsd(u1.y), bitsd(u2.x), bitsd(u2.y));
                    if (a_tied) h.xf ^= TIE_FLAG;  // settled right before the shading
                    out_slot = (uint32_t)u5.x;
                    rng.s = u9.y;
                    beta = mk(bitsd(u10.x), bitsd(u10.y), bitsd(u11.x));
                    L = mk(bitsd(u11.y), bitsd(u12.x), bitsd(u12.y));
                    depth = (int)(uint32_t)(u13.x >> 32);
                    pix_id = (int)(uint32_t)u13.x;
                    pend = 0ull;
                    alive = true;
                    ready = true;
                }
                WF_STAT(1, __popcll(__ballot(!alive ? false : (idx < n_a && ((fr >> lane) & 1ull) != 0ull))));
            }
        }
        // ---- the other free lanes generate new paths, while the workgroup may still start any ----
        const uint32_t a_done = min(lds_load(&wfc[1]), n_a);
        const bool gate_open = lds_load(&wfc[0]) + (n_a - a_done) + WF_GATE <= wa.seg;
        uint64_t dead = __ballot(!alive);
        if ((int)__popcll(dead) < REGEN_MIN && dead != ~0ull) dead = 0ull;
        bool stuck = !gate_open || finished;  // no new unit can be started by this wave right now
        if (dead != 0ull && next >= pool && !stuck) {
            const UnitInfo u = next_unit_wf(wst, rmeta, cfg, wring, accum, tickets, counter, lane);
            if (u.pool > 0) {
                pool = u.pool;
                next = 0;
                s0 = u.s0;
                tx = u.tx;
                ty = u.ty;
                cur_slot = u.cur_slot;
            } else {
                stuck = true;  // ring full of open units, or no job left
            }
            finished = u.finished != 0;
        }
        if (dead != 0ull && next < pool && gate_open) {
            int k = next + __popcll(dead & lanemask_lt);
            next = min(next + (int)__popcll(dead), pool);
            if (!alive && k < pool) {
                int pix = k & (TILE_PIX - 1), s = s0 + (k >> 6);
                int x = tx * TILE_W + (pix & (TILE_W - 1)), y = ty * TILE_H + (pix >> 3);
                if (x < rk.width && y < rk.height) {  // camera_draw() + camera_ray(), written out
                    rng.seed_stream(rk.seed, (uint64_t)y * (uint64_t)rk.width + (uint64_t)x, (uint64_t)s);
                    double u = ((double)x + rng.gen_f64()) / (double)(rk.width - 1);
                    double v = ((double)y + rng.gen_f64()) / (double)(rk.height - 1);
                    double stt = 1.0 - v;
                    D3 rd = muls(random_in_unit_disk(rng), cam.lens_radius);
                    D3 offset = add(muls(cam.u, rd.x), muls(cam.v, rd.y));
                    o = add(cam.origin, offset);
                    d = sub(sub(add(add(cam.llc, muls(cam.horizontal, u)), muls(cam.vertical, stt)), cam.origin), offset);
                    beta = mk(1., 1., 1.);
                    L = mk(0., 0., 0.);
                    depth = rk.max_depth;
                    pix_id = y * rk.width + x;
                    out_slot = ((uint32_t)wave << WF_SLOT_BITS) | (((uint32_t)cur_slot * (uint32_t)UNIT_SPP + (uint32_t)(k >> 6)) * (uint32_t)TILE_PIX + (uint32_t)pix);
                    alive = true;
                    ready = false;
                    pend = 0ull;
                }
            }
            WF_STAT(2, __popcll(__ballot(alive)) - __popcll(~dead));
        }
        // ---- nothing in the lanes: leave when nothing is left to adopt and nothing may be started ----
        if (__ballot(alive) == 0ull) {
            if (__ballot(dec_slot >= 0) != 0ull) continue;
            if (lds_load(&wfc[1]) < n_a) continue;   // (another wave may take them first; then this wave comes back here)
            if (next < pool && gate_open) continue;  // edge tile: the 64 indices handed out were all outside the image
            if (next >= pool && !stuck) continue;    // a unit can still be started
            WF_STAT(!gate_open ? 5 : (finished ? 6 : 4), 1);
            break;
        }
        // ---- world-space walk of the lanes that start a segment, instances deferred ----
        if (alive && !ready && pend == 0ull) {
            h = traverse2<true, true, true, false, uint64_t, false, MIXED, false, false, TIE>(A, stk, stk_stride, o, d, rk.t_min, INFINITY, &pend);
            if (TIE && tie_flagged(h.xf)) pend = 0ull;  // two world-level objects share the best t: the reference-order walk (before the shading) answers for the whole ray
            if (pend == 0ull) ready = true;
        }
        // ---- enter the first deferred instance: walk the LDS-cached top of its BVH here, park what is left of the walk ----
        {
            const bool want = alive && !ready;  // (pend != 0)
            if (__ballot(want) != 0ull) {
                uint32_t ent_cur = REF_DONE, ni = 0u;
                int ent_sp = 0;
                if (want) {
                    ni = (uint32_t)(__ffsll((long long)pend) - 1);
                    const double* Minv = A.xforms + 32 * A.inst2[ni].x;
                    const D3 oo = xf_point(Minv, o), dd = xf_dir(Minv, d);
                    const double* g = qgrid_lds + 8 * ni;
                    const D3 og = mk((oo.x - g[0]) * g[3] + g[6], (oo.y - g[1]) * g[4] + g[6], (oo.z - g[2]) * g[5] + g[6]);
                    const D3 dg = mk(dd.x * g[3], dd.y * g[4], dd.z * g[5]);
                    const Ray32 r = make_ray32(og, dg, rk.t_min, h.t);
                    ent_cur = A.inst2[ni].y;
                    while ((ent_cur >> REF_TAG_SHIFT) == 0u && ent_cur < entry_top) {
                        const uint4* p = n2q_lds + 2 * ent_cur;
                        const uint4 u0 = p[0], u1 = p[1];
                        float e0, e1;
                        const bool h0 = box32((float)(u0.x & 0xffffu), (float)(u0.y & 0xffffu), (float)(u0.z & 0xffffu), (float)(u0.w & 0xffffu),
                                              (float)(u1.x & 0xffffu), (float)(u1.y & 0xffffu), r, e0);
                        const bool h1 = box32((float)(u0.x >> 16), (float)(u0.y >> 16), (float)(u0.z >> 16), (float)(u0.w >> 16),
                                              (float)(u1.x >> 16), (float)(u1.y >> 16), r, e1);
                        const uint32_t c0 = u1.z, c1 = u1.w;
                        if (h0 && h1) {
                            if (ent_sp == WF_ENTRY_STACK * stk_stride) break;  // the record holds 8 entries: the walk launch goes on from here
                            const bool swap = e1 < e0;
                            stk[ent_sp] = swap ? c0 : c1;
                            ent_sp += stk_stride;
                            ent_cur = swap ? c1 : c0;
                        } else if (h0) {
                            ent_cur = c0;
                        } else if (h1) {
                            ent_cur = c1;
                        } else if (ent_sp > 0) {
                            ent_sp -= stk_stride;
                            ent_cur = stk[ent_sp];
                        } else {
                            ent_cur = REF_DONE;
                        }
                    }
                    if (ent_cur == REF_DONE) {  // nothing of this instance within reach: next one (next iteration), or shade
                        pend &= pend - 1ull;
                        if (pend == 0ull) ready = true;
                    }
                }
                const bool park = want && ent_cur != REF_DONE;
                const uint64_t mp = __ballot(park);
                WF_STAT(0, __popcll(mp));
                WF_STAT(9, __popcll(__ballot(want)));
                if (mp != 0ull) {
                    const int leader = __ffsll((long long)mp) - 1;
                    uint32_t base = 0;
                    if (lane == leader) base = __hip_atomic_fetch_add(&wfc[0], (uint32_t)__popcll(mp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    base = __shfl(base, leader);
                    const uint32_t slot = base + (uint32_t)__popcll(mp & lanemask_lt);
                    if (park) {
                        if (slot < wa.seg) {
                            pend &= pend - 1ull;
                            const int n = ent_sp / stk_stride;
                            AS_G U2* q = seg_b + (size_t)slot * WF_REC_U;
                            U2 w;
                            w.x = dbits(o.x); w.y = dbits(o.y); q[0] = w;
                            w.x = dbits(o.z); w.y = dbits(d.x); q[1] = w;
                            w.x = dbits(d.y); w.y = dbits(d.z); q[2] = w;
                            w.x = dbits(h.t); w.y = ((uint64_t)h.kp << 32) | (uint64_t)(uint32_t)h.node; q[3] = w;
                            w.x = ((uint64_t)ent_cur << 32) | (uint64_t)(uint32_t)(h.xf + 1); w.y = pend; q[4] = w;
                            w.x = (uint64_t)out_slot | ((uint64_t)ni << 32) | ((uint64_t)n << 40); w.y = 0ull; q[5] = w;
                            uint32_t e[WF_ENTRY_STACK];
                            for (int i = 0; i < WF_ENTRY_STACK; i++) e[i] = (i < n) ? stk[i * stk_stride] : 0u;
                            w.x = (uint64_t)e[0] | ((uint64_t)e[1] << 32); w.y = (uint64_t)e[2] | ((uint64_t)e[3] << 32); q[6] = w;
                            w.x = (uint64_t)e[4] | ((uint64_t)e[5] << 32); w.y = (uint64_t)e[6] | ((uint64_t)e[7] << 32); q[7] = w;
                            w.x = 0ull; w.y = rng.s; q[9] = w;
                            w.x = dbits(beta.x); w.y = dbits(beta.y); q[10] = w;
                            w.x = dbits(beta.z); w.y = dbits(L.x); q[11] = w;
                            w.x = dbits(L.y); w.y = dbits(L.z); q[12] = w;
                            w.x = ((uint64_t)(uint32_t)depth << 32) | (uint64_t)(uint32_t)pix_id; w.y = 0ull; q[13] = w;
                            alive = false;
                        } else {
                            atomicOr(err, 8);  // cannot happen (see "No pool can overflow"): reported, the path is dropped
                            alive = false;
                        }
                    }
                }
            }
        }
        // ---- shade: sample_ray's loop body after World::hit, photon_mapper.rs:336-362 ----
        if (alive && ready) {
            bool done = true;
            if (TIE && tie_flagged(h.xf)) h = tie_resolve_view(A.tie_view, o.x, o.y, o.z, d.x, d.y, d.z, rk.t_min, INFINITY);  // as pt_kernel_coop
            if (h.node >= 0 && depth > 0) {
                depth -= 1;
                Rec rec = materialize<true>(A, h, o, d, err);
                D3 emitted, att, ndir;
                bool diffuse;
                bool scattered = shade(A, rec, d, rng, emitted, att, ndir, diffuse, err);
                L = add(L, elemul(beta, emitted));
                if (scattered) {
                    bool go = true;
                    if (INTEG == 2 && diffuse) {
                        const double* e = rk.sppm_est + 6 * (size_t)pix_id;
                        L = add(L, elemul(beta, mk(e[0], e[1], e[2])));
                        L = add(L, elemul(beta, mk(e[3], e[4], e[5])));
                        go = false;
                    } else if (INTEG == 1 && diffuse) {
                        go = mixture_step(A, rec, rng, att, beta, ndir, err);
                    } else {
                        beta = elemul(beta, att);
                    }
                    if (go) {
                        o = rec.p;
                        d = ndir;
                        done = false;
                    }
                }
            }
            ready = false;
            pend = 0ull;
            if (done) {  // into the ring slot of the wave that generated the path; its unit counter moves next iteration
                double* dst = bring + (size_t)(out_slot >> WF_SLOT_BITS) * wa.ring_units * UNIT_DOUBLES + 3 * (size_t)(out_slot & ((1u << WF_SLOT_BITS) - 1u));
                dst[0] = L.x;
                dst[1] = L.y;
                dst[2] = L.z;
                dec_slot = (int)out_slot;
                alive = false;
            }
        }
    }
#ifdef RTAMD_WF_STATS
    wfs[7] = __builtin_amdgcn_s_memtime() - t_start;
    if (lane == 0)
        for (int i = 0; i < 10; i++) atomicAdd(&g_wf_stats[i], wfs[i]);
#endif
    // ---- end of the launch: save the bookkeeping (the last next_unit() call above folded what was complete), report ----
    if (lane == 0) {
        wst[8] = (uint32_t)pool; wst[9] = (uint32_t)next; wst[10] = (uint32_t)s0; wst[11] = (uint32_t)tx; wst[12] = (uint32_t)ty;
        wst[13] = (uint32_t)cur_slot;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)WF_BOOK_WORDS; i += blockDim.x) book_save[i] = book[i];
    if (threadIdx.x == 0) {
        const uint32_t parked = min(lds_load(&wfc[0]), wa.seg);
        wa.cnt_b[blockIdx.x] = parked;
        bool open = parked != 0u;
        for (int w = 0; w < PT_BLOCK / 64; w++) {
            const uint32_t* ws = book + (size_t)(PT_BLOCK / 64) * WF_RING_UNITS * 4 + (size_t)w * WF_WST;
            if (ws[1] != 0u || ws[6] != 0u || ws[5] < ws[4]) open = true;  // units in the ring, jobs left, or a job half done
        }
        if (open) atomicAdd(wa.unfinished, 1u);
    }
}

// ------------------------------------------------------------------ the walk launch ----
struct WfWalkK {
    U2* pool;             // the records parked by the launch before: [grid_pt][seg][WF_REC_U]
    const uint32_t* cnt;  // [grid_pt] records per workgroup segment
    uint32_t* cursor;     // global fetch cursor over the chunk space [0, grid_pt * seg / WF_CHUNK), zeroed before the launch
    uint32_t grid_pt, seg;
    uint32_t n_topq;      // NodeQ cached in LDS
    uint32_t stack;       // stack entries per lane
    double t_min;
};
template <bool TIE>
__global__ void __launch_bounds__(WF_WALK_BLOCK) wf_walk_kernel(FlatView sv, WfWalkK wk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS map: [transforms][instance table][grids][NodeQ cache][stacks: wk.stack x WF_WALK_BLOCK words]
    uint32_t staged = 0;
    ServeCtx X;
    {
        auto stage = [&](uint32_t off, uint32_t bytes) {
            LDS_COPY16(smem + staged, sv.base + off, coop_a16(bytes) / 16);
            AS_L char* at = (AS_L char*)(smem + staged);
            staged += coop_a16(bytes);
            return at;
        };
        X.xforms = (const AS_L double*)stage(sv.off_xforms, sv.stage_bytes - sv.off_xforms);
        X.inst2 = (const AS_L uint32_t*)stage(sv.off_inst2, 8u * sv.n_inst2);
        X.qgrid = (const AS_L double*)stage(sv.off_qgrid, (uint32_t)sizeof(QGrid) * sv.n_inst2);
        X.n2q_top = (const AS_L u32x4*)stage(sv.off_n2q, wk.n_topq * (uint32_t)sizeof(NodeQ));
    }
    X.n_topq = wk.n_topq;
    X.n2q = (const AS_G u32x4*)(sv.base + sv.off_n2q);
    X.tri32 = (const AS_G u32x4*)(sv.base + sv.off_tri32);
    X.pool = (AS_G U2*)wk.pool;
    X.t_min = wk.t_min;
    __syncthreads();
    AS_L uint32_t* stk = (AS_L uint32_t*)(smem + staged) + threadIdx.x;
    const int stride = WF_WALK_BLOCK;
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t lanemask_lt = (1ull << lane) - 1ull;
    const double t_min = wk.t_min;
    const uint32_t chunks_per_seg = wk.seg / WF_CHUNK, n_chunks = wk.grid_pt * chunks_per_seg;

    // the wave's current chunk of records: [w_next, w_end) of segment w_seg
    uint32_t w_seg = 0, w_next = 0, w_end = 0;
    bool exhausted = false;

    long long rid = -1;  // record index (segment * seg + slot) this lane walks, -1: none
    D3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    Ray32 r = make_ray32(o, mk(1, 1, 1), t_min, 0.);
    double ht = 0.;
    int hnode = -1, hnode_in = -1;
    uint32_t hkp = 0, hxf = 0, cur = REF_DONE, inst = 0;
    uint64_t pend = 0ull;
    int sp = 0;
    bool tied = false;  // TIE: a triangle shares the best t exactly with the hit the walk holds (over all of the path's instances; a closer hit clears it)
    for (;;) {
        // ---- refill: idle lanes take the next records of the wave's chunk; an empty chunk is replaced from the global cursor ----
        uint64_t need = __ballot(rid < 0);
        while (need != 0ull && !exhausted) {
            if (w_next == w_end) {
                uint32_t c = 0;
                if (lane == 0) c = atomicAdd(wk.cursor, 1u);
                c = __builtin_amdgcn_readfirstlane(c);
                if (c >= n_chunks) {
                    exhausted = true;
                    break;
                }
                w_seg = c / chunks_per_seg;
                const uint32_t first = (c % chunks_per_seg) * WF_CHUNK, have = wk.cnt[w_seg];
                w_next = min(first, have);
                w_end = min(first + WF_CHUNK, have);
                continue;  // (an empty chunk: take the next one)
            }
            const uint32_t take = min((uint32_t)__popcll(need), w_end - w_next);
            const uint32_t rank = (uint32_t)__popcll(need & lanemask_lt);
            if (((need >> lane) & 1ull) != 0ull && rank < take) {
                rid = (long long)w_seg * (long long)wk.seg + (long long)(w_next + rank);
                const AS_G U2* q = X.pool + (size_t)rid * WF_REC_U;
                const U2 u0 = q[0], u1 = q[1], u2 = q[2], u3 = q[3], u4 = q[4], u5 = q[5];
                inst = (uint32_t)(u5.x >> 32) & 0xffu;
                const int n_saved = (int)((u5.x >> 40) & 0xffu);
                pend = u4.y;
                const uint32_t xfi = X.inst2[2 * inst];
                const AS_L double* m = X.xforms + 32 * xfi;  // M^-1: Transform::hit, transform.rs:153-156 (xf_point / xf_dir)
                const D3 wo = mk(bitsd(u0.x), bitsd(u0.y), bitsd(u1.x)), wd = mk(bitsd(u1.y), bitsd(u2.x), bitsd(u2.y));
                o = mk(m[0] * wo.x + m[1] * wo.y + m[2] * wo.z + m[3] * 1., m[4] * wo.x + m[5] * wo.y + m[6] * wo.z + m[7] * 1.,
                       m[8] * wo.x + m[9] * wo.y + m[10] * wo.z + m[11] * 1.);
                d = mk(m[0] * wd.x + m[1] * wd.y + m[2] * wd.z + m[3] * 0., m[4] * wd.x + m[5] * wd.y + m[6] * wd.z + m[7] * 0.,
                       m[8] * wd.x + m[9] * wd.y + m[10] * wd.z + m[11] * 0.);
                cur = (uint32_t)(u4.x >> 32);
                hxf = (uint32_t)u4.x;
                ht = bitsd(u3.x);
                hnode = (int)(uint32_t)u3.y;
                hnode_in = hnode;
                tied = false;
                hkp = (uint32_t)(u3.y >> 32);
                if (n_saved > 0) {  // what the entry walk left on its stack
                    const U2 s0 = q[6];
                    stk[0] = (uint32_t)s0.x;
                    if (n_saved > 1) stk[stride] = (uint32_t)(s0.x >> 32);
                    if (n_saved > 2) stk[2 * stride] = (uint32_t)s0.y;
                    if (n_saved > 3) stk[3 * stride] = (uint32_t)(s0.y >> 32);
                    if (n_saved > 4) {
                        const U2 s1 = q[7];
                        stk[4 * stride] = (uint32_t)s1.x;
                        if (n_saved > 5) stk[5 * stride] = (uint32_t)(s1.x >> 32);
                        if (n_saved > 6) stk[6 * stride] = (uint32_t)s1.y;
                        if (n_saved > 7) stk[7 * stride] = (uint32_t)(s1.y >> 32);
                    }
                }
                sp = n_saved * stride;
                const AS_L double* g = X.qgrid + 8 * inst;  // the ray on the instance's grid: same t (QGrid, flat.h)
                const D3 og = mk((o.x - g[0]) * g[3] + g[6], (o.y - g[1]) * g[4] + g[6], (o.z - g[2]) * g[5] + g[6]);
                const D3 dg = mk(d.x * g[3], d.y * g[4], d.z * g[5]);
                r = make_ray32(og, dg, t_min, ht);
            }
            w_next += take;
            need = __ballot(rid < 0);
        }
        if (__ballot(rid >= 0) == 0ull) break;  // (only once the cursor is exhausted)
        for (;;) {
#ifdef RTAMD_WF_STATS
            if (lane == 0) {
                atomicAdd(&g_wf_stats[10], 1ull);
                atomicAdd(&g_wf_stats[11], (unsigned long long)__popcll(__ballot(rid >= 0)));
            }
#endif
            blas_pass_q<TIE>(X, rid >= 0, stk, stride, o, d, t_min, r, ht, hnode, hkp, cur, sp, tied);
            const bool fin = rid >= 0 && cur == REF_DONE;
            if (fin) {  // this instance is done: the next deferred one of the same segment, or the answer
                if (hnode != hnode_in) hxf = X.inst2[2 * inst] + 1u;  // the walk accepted a candidate of this instance
                if (pend != 0ull) {
                    inst = (uint32_t)(__ffsll((long long)pend) - 1);
                    pend &= pend - 1ull;
                    const AS_G U2* q = X.pool + (size_t)rid * WF_REC_U;
                    const U2 u0 = q[0], u1 = q[1], u2 = q[2];
                    const AS_L double* m = X.xforms + 32 * X.inst2[2 * inst];
                    const D3 wo = mk(bitsd(u0.x), bitsd(u0.y), bitsd(u1.x)), wd = mk(bitsd(u1.y), bitsd(u2.x), bitsd(u2.y));
                    o = mk(m[0] * wo.x + m[1] * wo.y + m[2] * wo.z + m[3] * 1., m[4] * wo.x + m[5] * wo.y + m[6] * wo.z + m[7] * 1.,
                           m[8] * wo.x + m[9] * wo.y + m[10] * wo.z + m[11] * 1.);
                    d = mk(m[0] * wd.x + m[1] * wd.y + m[2] * wd.z + m[3] * 0., m[4] * wd.x + m[5] * wd.y + m[6] * wd.z + m[7] * 0.,
                           m[8] * wd.x + m[9] * wd.y + m[10] * wd.z + m[11] * 0.);
                    cur = X.inst2[2 * inst + 1];
                    hnode_in = hnode;
                    sp = 0;
                    const AS_L double* g = X.qgrid + 8 * inst;
                    const D3 og = mk((o.x - g[0]) * g[3] + g[6], (o.y - g[1]) * g[4] + g[6], (o.z - g[2]) * g[5] + g[6]);
                    const D3 dg = mk(d.x * g[3], d.y * g[4], d.z * g[5]);
                    r = make_ray32(og, dg, t_min, ht);
                } else {
                    AS_G U2* q = X.pool + (size_t)rid * WF_REC_U;
                    U2 a8;
                    a8.x = dbits(ht);
                    a8.y = ((uint64_t)hkp << 32) | (uint64_t)tie_order(hnode, TIE && tied);
                    q[8] = a8;
                    ((AS_G uint32_t*)(q + 9))[0] = hxf;
                    rid = -1;
                }
            }
            const int busy = __popcll(__ballot(rid >= 0));
            if (busy == 0) break;
            if (busy < COOP_REFILL_TH && !exhausted) break;  // idle lanes: refill
        }
    }
}
