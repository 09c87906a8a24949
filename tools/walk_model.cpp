// A CPU model of the BVH2 walk's WAVE-STEPS: what a 64-lane wave of pt_kernel's LDS form spends in traverse2, counted
// in the quantities tools/phase_stats.sh measures -- node steps, leaf-item steps and leaf sections per iteration with the lanes of each
// step, node steps and sphere tests per ray -- and priced with per-step costs given on the command line.  It ranks ideas about the NUMBER of
// steps (box pads, when a wave changes phase) in seconds; it knows nothing of registers, LDS or clocks.  Round 7 (profiles/r07/README.md): its
// relative changes for the pads were within a point of the measured ones; for the early leaf exit it missed how far leaf sections fragment.
//
// Host only: the product's own builder (csrc/host/accel.cpp) makes the tree, everything else is below.
//   g++ -O2 -std=c++17 -ffp-contract=off -Irust-raytracer_amd/csrc -Iinclude tools/walk_model.cpp -o build/walk_model
//   python3 -c "import json,sys; f=lambda n:[print(n['center']['x'],n['center']['y'],n['center']['z'],n['radius']) if n.get('type')=='Sphere' else None]+[f(v) for v in n.values()] if isinstance(n,dict) else [f(v) for v in n] if isinstance(n,list) else None; f(json.load(open(sys.argv[1])))" tests/golden/scenes/scene_500.json | sort -u > build/s500.txt
//   build/walk_model build/s500.txt                       the product's pad (|o|max = 64 x extent), while-while
//   build/walk_model build/s500.txt --omax-extents 2      the pad of a render from inside the scene (O_r = 2 x extent)
//   build/walk_model build/s500.txt --exit-k8 7           leave the node loop once lanes at a leaf >= 7/8 lanes still walking
//   build/walk_model build/s500m.txt --omax-extents 2 --start-leaf    every walk begins where csrc/common/walk_start.h says
// A line of the list may carry a fifth column, the sphere's material: L Lambertian, M Metal, D Dielectric, E DiffuseLight (s500m.txt: the
// command above with  ,n['material']['type'][0] if n['material']['type']!='DiffuseLight' else 'E'  added to the print, and no sort).  A
// list with that column is shaded by it: L diffuse with albedo 0.5, M mirror with albedo 0.8, D straight on with 12 % mirror and no
// absorption, E ends the path (a light scatters nothing); a list without it gets the stock mix below.
// options: --omax-extents F  --exit-k8 K  --tiles N (8x8-pixel tiles of primary rays, default 400)  --spp N (16)  --depth N (50)  --seed N
//          --start-leaf
//          --cam lx ly lz ax ay az vfov  --regen N (8: free lanes before a wave takes new paths)  --costs node item section test (38 78 10 1)
// The paths: primary rays per tile through a pinhole, then per sphere (by index) 80 % diffuse, 12 % mirror, 8 % glass-like (straight on),
// the ground diffuse; a path ends on a miss, at the depth limit, or by absorption (albedo 0.5 .. 0.9).
#include "host/accel.cpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>

#include "common/walk_start.h"

namespace rtamd {
Tuning tuning() { return Tuning{}; }
}  // namespace rtamd
using namespace rtamd;

struct V3 { double x, y, z; };
static V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V3 unit(V3 a) { return a * (1. / std::sqrt(dot(a, a))); }

struct Sph { V3 c; double r; char mat; };  // mat: L, M, D, E, or 0 = the stock mix
static std::vector<Sph> S;
static AccelBuild AB;
static uint32_t ROOT;

struct Lane {
    bool active = false;  // holds a path
    V3 o, d, inv;
    int depth = 0;
    // the walk
    uint32_t cur = REF_DONE;
    std::vector<uint32_t> stack;
    double best = 0;
    int hit = -1;
};
static bool slab(const Node2& nd, int k, const Lane& L, double& entry) {
    const double lo[3] = {nd.lo_x[k], nd.lo_y[k], nd.lo_z[k]}, hi[3] = {nd.hi_x[k], nd.hi_y[k], nd.hi_z[k]};
    const double o[3] = {L.o.x, L.o.y, L.o.z}, iv[3] = {L.inv.x, L.inv.y, L.inv.z};
    double tn = -INFINITY, tf = INFINITY;
    for (int a = 0; a < 3; a++) {
        const double p = (lo[a] - o[a]) * iv[a], q = (hi[a] - o[a]) * iv[a];
        tn = std::fmax(tn, std::fmin(p, q));
        tf = std::fmin(tf, std::fmax(p, q));
    }
    entry = tn;
    return !(tn > tf) && !(tn > L.best) && !(1e-3 > tf);
}
static void pop(Lane& L) {
    if (L.stack.empty()) L.cur = REF_DONE;
    else { L.cur = L.stack.back(); L.stack.pop_back(); }
}
static void node_step(Lane& L) {
    const Node2& nd = AB.nodes[L.cur];
    double e0, e1;
    const bool h0 = slab(nd, 0, L, e0), h1 = slab(nd, 1, L, e1);
    if (h0 && h1) {
        const bool swap = e1 < e0;
        L.stack.push_back(nd.child[swap ? 0 : 1]);
        L.cur = nd.child[swap ? 1 : 0];
    } else if (h0) L.cur = nd.child[0];
    else if (h1) L.cur = nd.child[1];
    else pop(L);
}
static void item_test(Lane& L, uint32_t item) {
    const Sph& s = S[AB.items[2 * (size_t)item] >> NK_BITS];
    const V3 oc = L.o - s.c;
    const double a = dot(L.d, L.d), hb = dot(oc, L.d), c = dot(oc, oc) - s.r * s.r, disc = hb * hb - a * c;
    if (disc < 0.) return;
    const double sq = std::sqrt(disc);
    double t = (-hb - sq) / a;
    if (!(t >= 1e-3 && t <= L.best)) t = (-hb + sq) / a;
    if (!(t >= 1e-3 && t <= L.best)) return;
    L.best = t;
    L.hit = (int)(AB.items[2 * (size_t)item] >> NK_BITS);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: walk_model SPHERES.txt [options]  (see the head of tools/walk_model.cpp)\n"); return 2; }
    double omax_ext = 64., cam[7] = {-6, 2, -6, 0, 0, -1, 45}, cost[4] = {38, 78, 10, 1};
    bool start_leaf = false;
    int k8 = 0, tiles = 400, spp = 16, max_depth = 50, regen = 8;
    uint64_t seed = 1;
    for (int i = 2; i < argc; i++) {
        auto next = [&](int n) { if (i + n >= argc) { fprintf(stderr, "%s needs %d value(s)\n", argv[i], n); exit(2); } };
        if (!strcmp(argv[i], "--omax-extents")) { next(1); omax_ext = atof(argv[++i]); }
        else if (!strcmp(argv[i], "--exit-k8")) { next(1); k8 = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--start-leaf")) start_leaf = true;
        else if (!strcmp(argv[i], "--tiles")) { next(1); tiles = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--spp")) { next(1); spp = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--depth")) { next(1); max_depth = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--regen")) { next(1); regen = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--seed")) { next(1); seed = strtoull(argv[++i], nullptr, 10); }
        else if (!strcmp(argv[i], "--cam")) { next(7); for (int k = 0; k < 7; k++) cam[k] = atof(argv[++i]); }
        else if (!strcmp(argv[i], "--costs")) { next(4); for (int k = 0; k < 4; k++) cost[k] = atof(argv[++i]); }
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    std::ifstream in(argv[1]);
    bool with_mat = false;
    for (std::string line; std::getline(in, line);) {
        std::istringstream ls(line);
        Sph s;
        s.mat = 0;
        if (!(ls >> s.c.x >> s.c.y >> s.c.z >> s.r)) continue;
        std::string m;
        if (ls >> m) { s.mat = m[0]; with_mat = true; }
        S.push_back(s);
    }
    if (S.empty()) { fprintf(stderr, "no spheres in %s (lines of: cx cy cz r)\n", argv[1]); return 1; }
    std::vector<AccelItem> items(S.size());
    double ew = 0.;
    for (size_t i = 0; i < S.size(); i++) {
        const double c[3] = {S[i].c.x, S[i].c.y, S[i].c.z}, r = std::fabs(S[i].r);
        Box b;
        for (int k = 0; k < 3; k++) { b.mn[k] = c[k] - r; b.mx[k] = c[k] + r; ew = std::fmax(ew, std::fmax(std::fabs(b.mn[k]), std::fabs(b.mx[k]))); }
        items[i] = AccelItem{b, NK_SPHERE | ((uint32_t)i << NK_BITS), (int32_t)i};
    }
    const double pad = 3. * std::ldexp(omax_ext * ew, -22);  // as build_bvhs pads for |o|max (the pad does not enter the SAH: the same tree)
    ROOT = accel_build_bvh(AB, items, pad, 0);
    if (!AB.ok) { fprintf(stderr, "the builder gave up\n"); return 1; }
    // where a walk begins: the root, or (--start-leaf) what the kernels' own rule says for this root
    const WalkStart begin = start_leaf ? walk_start(AB.nodes[ROOT], ROOT) : WalkStart{ROOT, WALK_START_NONE};

    // camera (pinhole): 1200-pixel-wide image, tile t = the t-th 8x8 tile of a stride that spreads the tiles over the frame
    const V3 from = {cam[0], cam[1], cam[2]}, w = unit(from - V3{cam[3], cam[4], cam[5]}), u = unit(cross(V3{0, 1, 0}, w)), v = cross(w, u);
    const double half = std::tan(cam[6] * M_PI / 360.);
    const int W = 1200, TX = W / 8, n_tiles_img = TX * TX;
    std::mt19937_64 gen(seed);
    std::uniform_real_distribution<double> U(0., 1.);
    long next_path = 0;
    const long n_paths = (long)tiles * 64 * spp;
    auto primary = [&](Lane& L) {
        const long p = next_path++;
        const int tile = (int)((p / (64L * spp)) * (n_tiles_img / tiles) % n_tiles_img), pix = (int)(p % 64);
        const double px = ((tile % TX) * 8 + (pix & 7) + U(gen)) / W * 2. - 1., py = 1. - ((tile / TX) * 8 + (pix >> 3) + U(gen)) / W * 2.;
        L.o = from;
        L.d = u * (px * half) + v * (py * half) - w;
        L.depth = 0;
        L.active = true;
    };
    auto rand_unit = [&]() {
        for (;;) {
            V3 p = {2 * U(gen) - 1, 2 * U(gen) - 1, 2 * U(gen) - 1};
            const double l = dot(p, p);
            if (l < 1. && l > 1e-12) return p * (1. / std::sqrt(l));
        }
    };

    std::vector<Lane> wave(64);
    // counters: wave-steps and lane-steps of node steps [0], item steps [1], sections [2]; iterations; rays by primary / secondary
    double ws[3] = {0, 0, 0}, ls[3] = {0, 0, 0};
    long iters = 0, rays[2] = {0, 0}, ray_nodes[2] = {0, 0}, ray_items[2] = {0, 0}, ray_leaves[2] = {0, 0}, one_lane_steps = 0;
    for (;;) {
        int free_lanes = 0, busy = 0;
        for (auto& L : wave) free_lanes += !L.active;
        if (free_lanes >= regen || free_lanes == 64)
            for (auto& L : wave)
                if (!L.active && next_path < n_paths) primary(L);
        for (auto& L : wave) busy += L.active;
        if (!busy) break;
        iters++;
        for (auto& L : wave) {
            L.cur = L.active ? begin.start_ref : REF_DONE;
            L.stack.clear();
            if (L.active && begin.push_ref != WALK_START_NONE) L.stack.push_back(begin.push_ref);
            L.best = INFINITY;
            L.hit = -1;
            L.inv = {1. / L.d.x, 1. / L.d.y, 1. / L.d.z};
            if (L.active) rays[L.depth > 0]++;
        }
        for (;;) {  // traverse2, while-while
            int n_round = 0, n_done = 0;
            for (auto& L : wave) n_round += L.cur != REF_DONE;
            if (!n_round) break;
            for (;;) {
                int n_inner = 0;
                for (auto& L : wave) n_inner += (L.cur >> REF_TAG_SHIFT) == 0u;
                if (!n_inner) break;
                ws[0]++; ls[0] += n_inner;
                one_lane_steps += n_inner == 1;
                for (auto& L : wave)
                    if ((L.cur >> REF_TAG_SHIFT) == 0u) {
                        ray_nodes[L.depth > 0]++;
                        node_step(L);
                        n_done += L.cur == REF_DONE;
                    }
                if (k8 > 0) {
                    n_inner = 0;
                    for (auto& L : wave) n_inner += (L.cur >> REF_TAG_SHIFT) == 0u;
                    if ((8 - k8) * (n_round - n_done) >= 8 * n_inner) break;
                }
            }
            int max_cnt = 0, n_leaf = 0;
            for (auto& L : wave)
                if ((L.cur >> REF_TAG_SHIFT) == 1u) { n_leaf++; max_cnt = std::max(max_cnt, (int)((L.cur >> REF_LEAF_COUNT_SHIFT) & 7u) + 1); }
            if (!n_leaf) continue;  // (everybody through, or -- never with k8 > 0 -- nobody at a leaf)
            ws[2]++; ls[2] += n_leaf;
            for (int i = 0; i < max_cnt; i++) {
                int n = 0;
                for (auto& L : wave)
                    if ((L.cur >> REF_TAG_SHIFT) == 1u && i <= (int)((L.cur >> REF_LEAF_COUNT_SHIFT) & 7u)) {
                        n++;
                        ray_items[L.depth > 0]++;
                        item_test(L, (L.cur & REF_LEAF_FIRST_MASK) + (uint32_t)i);
                    }
                ws[1]++; ls[1] += n;
            }
            for (auto& L : wave)
                if ((L.cur >> REF_TAG_SHIFT) == 1u) { ray_leaves[L.depth > 0]++; pop(L); }
        }
        for (auto& L : wave) {  // shade
            if (!L.active) continue;
            if (L.hit < 0 || ++L.depth >= max_depth) { L.active = false; continue; }
            const Sph& sp = S[L.hit];
            const V3 p = L.o + L.d * L.best, n = (p - sp.c) * (1. / sp.r);
            if (with_mat) {
                if (sp.mat == 'E') { L.active = false; continue; }
                const double alb = sp.mat == 'D' ? 1. : sp.mat == 'M' ? 0.8 : 0.5;
                if (U(gen) > alb) { L.active = false; continue; }
                L.o = p;
                if (sp.mat == 'M' || (sp.mat == 'D' && U(gen) < 0.12)) L.d = L.d - n * (2. * dot(L.d, n));
                else if (sp.mat != 'D') L.d = (dot(n, L.d) < 0 ? n : n * -1.) + rand_unit();
                continue;
            }
            const uint32_t h = (uint32_t)L.hit * 2654435761u;
            const double kind = sp.r > 10. ? 0. : (h >> 8 & 0xffff) / 65536., albedo = 0.5 + 0.4 * ((h >> 4 & 0xff) / 256.);
            if (U(gen) > albedo) { L.active = false; continue; }
            L.o = p;
            if (kind < 0.80) L.d = (dot(n, L.d) < 0 ? n : n * -1.) + rand_unit();
            else if (kind < 0.92) L.d = L.d - n * (2. * dot(L.d, n));
            // else glass-like: straight on, through the sphere
        }
    }
    const double it = (double)iters;
    printf("spheres %zu  nodes %zu  extent %g  pad %.3g (|o|max = %g x extent)  exit-k8 %d  paths %ld  iterations %ld\n", S.size(), AB.nodes.size(), ew, pad, omax_ext, k8, n_paths, iters);
    printf("materials: %s  walks begin at 0x%08x with 0x%08x pushed%s\n", with_mat ? "the list's column" : "the stock mix", begin.start_ref, begin.push_ref,
           begin.push_ref == WALK_START_NONE ? " (nothing: the root)" : "");
    const char* nm[3] = {"inner-node steps", "leaf items", "leaf sections"};
    for (int k = 0; k < 3; k++) printf("%-18s wave-exec/iter %8.3f  lanes/exec %5.1f\n", nm[k], ws[k] / it, ws[k] ? ls[k] / ws[k] : 0.);
    printf("node steps with one lane: %.1f %%\n", ws[0] ? 100. * one_lane_steps / ws[0] : 0.);
    const char* rn[2] = {"primary", "secondary"};
    for (int k = 0; k < 2; k++)
        printf("per %-9s ray (%ld): node steps %.2f  sphere tests %.2f  leaf visits %.2f\n", rn[k], rays[k], rays[k] ? (double)ray_nodes[k] / rays[k] : 0.,
               rays[k] ? (double)ray_items[k] / rays[k] : 0., rays[k] ? (double)ray_leaves[k] / rays[k] : 0.);
    const double valu = ws[0] * (cost[0] + (k8 > 0 ? cost[3] : 0.)) + ws[1] * cost[1] + ws[2] * cost[2];
    printf("VALU-equivalents per iteration %.1f  (node %g%s, item %g, section %g)\n", valu / it, cost[0], k8 > 0 ? " + test" : "", cost[1], cost[2]);
    return 0;
}
