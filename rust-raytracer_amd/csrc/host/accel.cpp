// Kernel-2 acceleration structure: binned-SAH BVH2 with conservative f32 child boxes.
//
// This hierarchy is NOT the reference's (objects/bvh.rs:60-83 is a random-axis median split and
// the scene files carry their own trees); it only prunes.  The reference's result is preserved
// because primitives keep their f64 tests and the tie rule is carried by AccelItem::order
// (see common/flat.h).  Host-side, once per rt_scene_commit.
#include "accel.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace rtamd {

namespace {

float round_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
    return f;
}
float round_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
    return f;
}
Box merge(const Box& a, const Box& b) {
    Box r;
    for (int i = 0; i < 3; i++) {
        r.mn[i] = std::fmin(a.mn[i], b.mn[i]);
        r.mx[i] = std::fmax(a.mx[i], b.mx[i]);
    }
    return r;
}
double area(const Box& b) {
    double dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}
Box empty_box() {
    const double inf = std::numeric_limits<double>::infinity();
    return Box{{inf, inf, inf}, {-inf, -inf, -inf}};
}

struct Ctx {
    AccelBuild& out;
    std::vector<AccelItem>& items;
    double pad;
    double c_box;  // rt_tuning.sah_box_cost and .max_leaf, snapshotted once per build (read at commit time)
    int max_leaf;
};

const double C_PRIM = 2.0;  // relative costs of a child-box pair test (c_box()) and a primitive test
#ifndef RT_SAH_BINS
#define RT_SAH_BINS 32  // (16: headline -0.4 %, 64: +-0)
#endif
const int BINS = RT_SAH_BINS;
int clamp_max_leaf(int m) {  // items per leaf, 1..ACCEL_DEFAULT_LEAF
    return m < 1 ? ACCEL_DEFAULT_LEAF : (m > ACCEL_DEFAULT_LEAF ? ACCEL_DEFAULT_LEAF : m);
}

uint32_t make_leaf(Ctx& c, int begin, int end) {
    uint32_t first = (uint32_t)(c.out.items.size() / 2);
    for (int i = begin; i < end; i++) {
        c.out.items.push_back(c.items[i].kp);
        c.out.items.push_back((uint32_t)c.items[i].order);
    }
    if (first + (uint32_t)(end - begin) > REF_LEAF_FIRST_MASK) {
        c.out.ok = false;
        return REF_DONE;
    }
    return REF_LEAF | ((uint32_t)(end - begin - 1) << REF_LEAF_COUNT_SHIFT) | first;
}

// force_split: the root of a BVH with >= 2 items is always an inner node with two real children, so that every BVH starts with
// a box test and no node needs an "empty" child
uint32_t build(Ctx& c, int begin, int end, int depth, bool force_split = false) {
    if (depth > c.out.max_depth) c.out.max_depth = depth;
    const int n = end - begin;
    bool has_instance = false;  // an instance must sit alone in its leaf (the traversal enters one instance per leaf)
    for (int i = begin; i < end; i++) has_instance |= (c.items[i].kp & NK_MASK) == NK_INSTANCE;
    if (has_instance && n > 1 && depth >= ACCEL_MAX_STACK - 4) {
        c.out.ok = false;
        return REF_DONE;
    }
    if (n <= 1 || depth >= ACCEL_MAX_STACK - 4) {
        if (n > ACCEL_MAX_LEAF) {  // depth cap hit with too many items: give up on the accel, kernel 1 remains
            c.out.ok = false;
            return REF_DONE;
        }
        return make_leaf(c, begin, end);
    }
    Box bounds = empty_box(), cb = empty_box();
    for (int i = begin; i < end; i++) {
        bounds = merge(bounds, c.items[i].box);
        for (int a = 0; a < 3; a++) {
            double ctr = 0.5 * (c.items[i].box.mn[a] + c.items[i].box.mx[a]);
            cb.mn[a] = std::fmin(cb.mn[a], ctr);
            cb.mx[a] = std::fmax(cb.mx[a], ctr);
        }
    }
    // binned SAH over the three axes
    double best_cost = std::numeric_limits<double>::infinity();
    int best_axis = -1, best_bin = -1;
    const double parent_area = area(bounds);
    for (int a = 0; a < 3; a++) {
        double lo = cb.mn[a], ext = cb.mx[a] - cb.mn[a];
        if (!(ext > 0.) || !std::isfinite(ext)) continue;
        Box bb[BINS];
        int cnt[BINS];
        for (int b = 0; b < BINS; b++) { bb[b] = empty_box(); cnt[b] = 0; }
        for (int i = begin; i < end; i++) {
            double ctr = 0.5 * (c.items[i].box.mn[a] + c.items[i].box.mx[a]);
            int b = (int)((ctr - lo) / ext * BINS);
            if (b < 0) b = 0;
            if (b >= BINS) b = BINS - 1;
            bb[b] = merge(bb[b], c.items[i].box);
            cnt[b]++;
        }
        double right_area[BINS];
        int right_cnt[BINS];
        Box acc = empty_box();
        int k = 0;
        for (int b = BINS - 1; b > 0; b--) {
            acc = merge(acc, bb[b]);
            k += cnt[b];
            right_area[b] = k ? area(acc) : 0.;
            right_cnt[b] = k;
        }
        acc = empty_box();
        k = 0;
        for (int b = 0; b < BINS - 1; b++) {
            acc = merge(acc, bb[b]);
            k += cnt[b];
            if (k == 0 || right_cnt[b + 1] == 0) continue;
            double cost = c.c_box + C_PRIM * (area(acc) * k + right_area[b + 1] * right_cnt[b + 1]) / parent_area;
            if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = b; }
        }
    }
    int mid = -1;
    if (best_axis >= 0 && (n > c.max_leaf || has_instance || force_split || best_cost < C_PRIM * n)) {
        double lo = cb.mn[best_axis], ext = cb.mx[best_axis] - cb.mn[best_axis];
        auto it = std::stable_partition(c.items.begin() + begin, c.items.begin() + end, [&](const AccelItem& it2) {
            double ctr = 0.5 * (it2.box.mn[best_axis] + it2.box.mx[best_axis]);
            int b = (int)((ctr - lo) / ext * BINS);
            if (b < 0) b = 0;
            if (b >= BINS) b = BINS - 1;
            return b <= best_bin;
        });
        mid = (int)(it - c.items.begin());
        if (mid == begin || mid == end) mid = -1;
    }
    if (mid < 0) {
        if (n <= c.max_leaf && !has_instance && !force_split) return make_leaf(c, begin, end);
        mid = begin + n / 2;  // identical centroids (e.g. concentric spheres): split by index
    }
    uint32_t idx = (uint32_t)c.out.nodes.size();
    c.out.nodes.push_back(Node2{});
    uint32_t child[2];
    Box cbx[2] = {empty_box(), empty_box()};
    for (int i = begin; i < mid; i++) cbx[0] = merge(cbx[0], c.items[i].box);
    for (int i = mid; i < end; i++) cbx[1] = merge(cbx[1], c.items[i].box);
    child[0] = build(c, begin, mid, depth + 1);
    child[1] = build(c, mid, end, depth + 1);
    Node2& nd = c.out.nodes[idx];
    for (int k = 0; k < 2; k++) {
        nd.lo_x[k] = round_down(cbx[k].mn[0] - c.pad); nd.hi_x[k] = round_up(cbx[k].mx[0] + c.pad);
        nd.lo_y[k] = round_down(cbx[k].mn[1] - c.pad); nd.hi_y[k] = round_up(cbx[k].mx[1] + c.pad);
        nd.lo_z[k] = round_down(cbx[k].mn[2] - c.pad); nd.hi_z[k] = round_up(cbx[k].mx[2] + c.pad);
        nd.child[k] = child[k];
    }
    nd.pad[0] = nd.pad[1] = 0;
    return idx;
}

}  // namespace

// Node2.pad[k] = the smallest reference-order index among the items of child k's subtree: lets a walk that only cares about items
// below some index (the media logic of kernel 2: "what the reference has visited before this medium") skip whole subtrees.
static uint32_t fill_min_order(AccelBuild& out, uint32_t ref) {
    if ((ref >> REF_TAG_SHIFT) == 1u) {
        const uint32_t first = ref & REF_LEAF_FIRST_MASK, cnt = ((ref >> REF_LEAF_COUNT_SHIFT) & 7u) + 1u;
        uint32_t m = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < cnt; i++) m = std::min(m, out.items[2 * (size_t)(first + i) + 1]);
        return m;
    }
    if ((ref >> REF_TAG_SHIFT) != 0u) return 0xFFFFFFFFu;
    Node2& nd = out.nodes[ref];
    const uint32_t c0 = nd.child[0], c1 = nd.child[1];
    const uint32_t m0 = fill_min_order(out, c0), m1 = fill_min_order(out, c1);
    out.nodes[ref].pad[0] = m0;
    out.nodes[ref].pad[1] = m1;
    return std::min(m0, m1);
}

static uint32_t accel_build_bvh_impl(AccelBuild& out, std::vector<AccelItem>& items, double pad, int depth0);
uint32_t accel_build_bvh(AccelBuild& out, std::vector<AccelItem>& items, double pad, int depth0) {
    const uint32_t root = accel_build_bvh_impl(out, items, pad, depth0);
    if (out.ok && root != REF_DONE) fill_min_order(out, root);
    return root;
}
static uint32_t accel_build_bvh_impl(AccelBuild& out, std::vector<AccelItem>& items, double pad, int depth0) {
    if (items.empty() || !std::isfinite(pad)) {
        out.ok = false;
        return REF_DONE;
    }
    for (auto& it : items)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(it.box.mn[a]) || !std::isfinite(it.box.mx[a])) {
                out.ok = false;
                return REF_DONE;
            }
    const Tuning tun = tuning();
    Ctx c{out, items, pad, tun.c_box > 0. ? tun.c_box : 1.0, clamp_max_leaf(tun.max_leaf)};
    if (items.size() == 1) {
        // A single item still gets one inner node so that the root is box-tested like everything else.  Its second child is a
        // ZERO-SIZE box at the low corner of the first (finite, inside the BVH's bounds, quantisable like any other box): a ray
        // passes the slab test of a point only when it goes through it to within the test's 1e-6 relative slack, and if one
        // ever does, re-testing the same item changes nothing (tie rule by order).  An inverted or infinite "empty" box does
        // NOT work here: the slab test takes min/max per axis, so +-inf bounds pass every ray.
        uint32_t idx = (uint32_t)out.nodes.size();
        out.nodes.push_back(Node2{});
        uint32_t leaf = make_leaf(c, 0, 1);
        Node2& nd = out.nodes[idx];
        const Box& b = items[0].box;
        nd.lo_x[0] = round_down(b.mn[0] - pad); nd.hi_x[0] = round_up(b.mx[0] + pad);
        nd.lo_y[0] = round_down(b.mn[1] - pad); nd.hi_y[0] = round_up(b.mx[1] + pad);
        nd.lo_z[0] = round_down(b.mn[2] - pad); nd.hi_z[0] = round_up(b.mx[2] + pad);
        nd.lo_x[1] = nd.hi_x[1] = nd.lo_x[0];
        nd.lo_y[1] = nd.hi_y[1] = nd.lo_y[0];
        nd.lo_z[1] = nd.hi_z[1] = nd.lo_z[0];
        nd.child[0] = leaf;
        nd.child[1] = leaf;
        nd.pad[0] = nd.pad[1] = 0;
        if (depth0 + 1 > out.max_depth) out.max_depth = depth0 + 1;
        return idx;
    }
    return build(c, 0, (int)items.size(), depth0, true);
}

// ---- the accel of a scene: the stages of build_scene_accel, in the order it calls them -------------------------------------------
namespace {

bool is_f32(double x) { return (double)(float)x == x; }

// An instance's item in the enclosing space carries the Transform's own bounding box (the box of the 8 transformed corners
// of the child's box, transform.rs:104-150): loose for a rotated mesh.  For culling, the union of the transformed boxes of the
// instance's ITEMS is as valid (affine images of the items lie inside it; the f64 rounding of M * corner is orders of
// magnitude below the pad added at build time) and tighter: fewer rays enter the object-space BVH for nothing.
// (innermost chains first: an instance's own item box, in its parent's context, is tightened before the parent's items are unioned)
void tighten_instance_boxes(std::vector<AccelContext>& ctx, const std::vector<size_t>& by_depth) {
    for (size_t k = by_depth.size(); k-- > 0;) {
        const size_t i = by_depth[k];
        const auto& c = ctx[i];
        if (c.items.empty() || !c.M) continue;
        Box tb = empty_box();
        for (const auto& it : c.items)
            for (int corner = 0; corner < 8; corner++) {
                const double x = (corner & 1) ? it.box.mx[0] : it.box.mn[0], y = (corner & 2) ? it.box.mx[1] : it.box.mn[1],
                             z = (corner & 4) ? it.box.mx[2] : it.box.mn[2];
                for (int a = 0; a < 3; a++) {
                    const double w = c.M[4 * a] * x + c.M[4 * a + 1] * y + c.M[4 * a + 2] * z + c.M[4 * a + 3];
                    tb.mn[a] = std::fmin(tb.mn[a], w);
                    tb.mx[a] = std::fmax(tb.mx[a], w);
                }
            }
        bool finite = true;
        for (int a = 0; a < 3; a++) finite = finite && std::isfinite(tb.mn[a]) && std::isfinite(tb.mx[a]);
        if (!finite) continue;
        const uint32_t want = NK_INSTANCE | ((uint32_t)(i - 1) << NK_BITS);
        for (auto& pc : ctx)
            for (auto& it : pc.items)
                if (it.kp == want)
                    for (int a = 0; a < 3; a++) {  // never larger than the Transform's own box; a margin of 2^-40 of its size for the rounding
                        const double m = std::ldexp(std::fabs(tb.mx[a]) + std::fabs(tb.mn[a]), -40);
                        it.box.mn[a] = std::fmax(it.box.mn[a], tb.mn[a] - m);
                        it.box.mx[a] = std::fmin(it.box.mx[a], tb.mx[a] + m);
                    }
    }
}

// Which instances can kernels 5 / 6 defer?  Those that hold nothing but triangles with f32 vertices (flat.h "Compact instance data").
// The others are entered in the lane: their items in the world's context become NK_INSTANCE_INLINE.  Also bounds every instance's
// object-space ray origins (inst_oo); an instance beyond the range the box tests are proven for rules the accel out.
void classify_instances(SceneAccel& a, std::vector<AccelContext>& ctx, const std::vector<size_t>& by_depth, const TriTables& t) {
    a.compact_cand.assign(ctx.size() - 1, 1);
    a.inst_oo.assign(ctx.size() - 1, 0.);
    for (size_t i : by_depth) {
        if (!a.ab.ok) break;
        auto& c = ctx[i];
        // object-space origin bound: |M^-1 o| <= sum_b |Minv[a][b]| * |o|max + |Minv[a][3]|, composed along the chain (the
        // parent's bound is its own object-space one; by_depth computes it first)
        const double o_parent = c.parent == 0 ? a.origin_limit : a.inst_oo[c.parent - 1];
        double oo = 0.;
        for (int k = 0; k < 3; k++)
            oo = std::fmax(oo, (std::fabs(c.Minv[4 * k]) + std::fabs(c.Minv[4 * k + 1]) + std::fabs(c.Minv[4 * k + 2])) * o_parent +
                                   std::fabs(c.Minv[4 * k + 3]));
        for (auto& it : c.items)  // hit points inside the instance also serve as origins of secondary rays (in world space only)
            for (int k = 0; k < 3; k++) oo = std::fmax(oo, std::fmax(std::fabs(it.box.mn[k]), std::fabs(it.box.mx[k])));
        if (!(oo < 68719476736.)) { a.ab.ok = false; break; }
        a.inst_oo[i - 1] = oo;
        char& cand = a.compact_cand[i - 1];
        for (auto& it : c.items) {
            if ((it.kp & NK_MASK) != NK_TRI) { cand = 0; break; }
            const uint32_t tri = it.kp >> NK_BITS;
            for (int c3 = 0; c3 < 3 && cand; c3++)
                for (int k = 0; k < 3; k++)
                    if (!is_f32(t.vpos[3 * (size_t)t.tris[4 * (size_t)tri + c3] + k])) cand = 0;
            if (!cand) break;
        }
        if (!cand) {
            const uint32_t want = NK_INSTANCE | ((uint32_t)(i - 1) << NK_BITS);
            for (auto& it : ctx[0].items)
                if (it.kp == want) it.kp = NK_INSTANCE_INLINE | ((uint32_t)(i - 1) << NK_BITS);
        }
    }
}

// The world BVH, then the BVHs of the inline instances, then those of the deferrable ones: the inline instances' leaves sit right
// behind the world's in the item array, and kernels 5 / 6 stage that prefix in LDS.
void build_bvhs(SceneAccel& a, std::vector<AccelContext>& ctx, const std::vector<size_t>& by_depth, bool nested, double media_extent,
                const TriTables& t) {
    AccelBuild& ab = a.ab;
    if (ctx[0].items.empty()) ab.ok = false;
    if (!ab.ok) return;
    // E_w: largest |coordinate| of the world items; boxes are padded so that rounding a ray origin with
    // max-abs coordinate <= 64*E_w to f32 (relative error 2^-24) can never make the f32 slab test cull a box
    // the exact test keeps: 4 * 2^-24 * |o|max covers of = fl32(o) and c = fl32(of * iv)  (derivation above box32
    // in csrc/device/kernels.hip, which also needs every coordinate below 2^36 in magnitude); the pad is THREE times that
    // (12 * 2^-24 * |o|max) since round 3 so that box32w, the test of the LDS-resident node table, needs no widening factor
    // on the far side (its proof, above box32w, uses the extra margin against the relative error of the slab parameters)
    double ew = media_extent;
    for (auto& it : ctx[0].items)
        for (int k = 0; k < 3; k++) ew = std::fmax(ew, std::fmax(std::fabs(it.box.mn[k]), std::fabs(it.box.mx[k])));
    if (!(ew > 0.) || !std::isfinite(ew)) {
        ab.ok = false;
        return;
    }
    a.origin_limit = 64. * ew;
    const double pad_w = 3. * std::ldexp(a.origin_limit, -22);  // 12 * 2^-24 * |o|max
    if (!(a.origin_limit < 68719476736.)) ab.ok = false;  // 2^36
    a.root2 = accel_build_bvh(ab, ctx[0].items, pad_w, 0);
    const int depth_tlas = ab.max_depth;
    a.world_depth = (uint32_t)depth_tlas;
    ab.inst.assign(2 * (ctx.size() - 1), 0u);
    classify_instances(a, ctx, by_depth, t);
    // (the world BVH was built above with the items' kinds as they were: its leaf items are patched below, after the build)
    // stack depth at which each context's BVH starts: below its parent's deepest level and one REF_RESTORE entry per level
    std::vector<int> end_depth(ctx.size(), depth_tlas);
    for (int pass = 0; pass < 2; pass++) {
        for (size_t i : by_depth) {  // (a parent holds an instance item: never deferrable, so pass 0 builds it before its children)
            if (!ab.ok) break;
            if ((a.compact_cand[i - 1] != 0) != (pass == 1)) continue;  // pass 0: inline instances, pass 1: deferrable ones
            auto& c = ctx[i];
            const size_t nodes_before = ab.nodes.size();
            const int depth_before = ab.max_depth;
            const int start = end_depth[c.parent] + 1;
            ab.max_depth = start;
            uint32_t r = accel_build_bvh(ab, c.items, 3. * std::ldexp(a.inst_oo[i - 1], -22), start);
            end_depth[i] = ab.max_depth;
            if (pass == 1) {
                a.max_inst_nodes = std::max<uint32_t>(a.max_inst_nodes, (uint32_t)(ab.nodes.size() - nodes_before));
                a.inst_depth = std::max<uint32_t>(a.inst_depth, (uint32_t)std::max(1, ab.max_depth - depth_tlas + 1));
            }
            ab.max_depth = std::max(ab.max_depth, depth_before);
            ab.inst[2 * (i - 1)] = nested ? c.chain : c.xform;
            ab.inst[2 * (i - 1) + 1] = r;
        }
        if (pass == 0) {
            a.n_world_items = (uint32_t)(ab.items.size() / 2);
            a.stack_inline = (uint32_t)(ab.max_depth + 2);
        }
    }
    for (size_t j = 0; j < ab.items.size() / 2; j++) {  // the world leaves' instance items, as classified
        const uint32_t kp = ab.items[2 * j];
        if ((kp & NK_MASK) == NK_INSTANCE && !a.compact_cand[kp >> NK_BITS]) ab.items[2 * j] = NK_INSTANCE_INLINE | (kp & ~NK_MASK);
    }
}

// Relabels the Node2 array by depth (all BVHs interleaved): the first K nodes are the K shallowest, which is what the kernels cache
// in LDS when the whole scene does not fit.  The world-space nodes then all have an index below world_top.
void sort_nodes_by_depth(SceneAccel& a) {
    AccelBuild& ab = a.ab;
    const size_t nn = ab.nodes.size();
    std::vector<int> depth(nn, 0);
    std::vector<uint32_t> stack, world;
    auto walk = [&](uint32_t root, bool is_world) {
        if ((root >> REF_TAG_SHIFT) != 0u) return;
        depth[root] = 0;
        stack.assign(1, root);
        while (!stack.empty()) {
            uint32_t n = stack.back();
            stack.pop_back();
            if (is_world) world.push_back(n);
            for (int k = 0; k < 2; k++) {
                uint32_t c = ab.nodes[n].child[k];
                if ((c >> REF_TAG_SHIFT) == 0u) {
                    depth[c] = depth[n] + 1;
                    stack.push_back(c);
                }
            }
        }
    };
    walk(a.root2, true);
    for (size_t i = 0; i + 1 < ab.inst.size(); i += 2) walk(ab.inst[i + 1], false);
    std::vector<uint32_t> order(nn);
    for (size_t i = 0; i < nn; i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return depth[x] < depth[y]; });
    std::vector<uint32_t> new_of(nn);
    for (size_t i = 0; i < nn; i++) new_of[order[i]] = (uint32_t)i;
    auto remap = [&](uint32_t r) { return ((r >> REF_TAG_SHIFT) == 0u) ? new_of[r] : r; };
    std::vector<Node2> sorted(nn);
    for (size_t i = 0; i < nn; i++) {
        Node2 nd = ab.nodes[order[i]];
        nd.child[0] = remap(nd.child[0]);
        nd.child[1] = remap(nd.child[1]);
        sorted[i] = nd;
    }
    ab.nodes.swap(sorted);
    a.root2 = remap(a.root2);
    for (size_t i = 0; i + 1 < ab.inst.size(); i += 2) ab.inst[i + 1] = remap(ab.inst[i + 1]);
    for (uint32_t n : world) a.world_top = std::max(a.world_top, new_of[n] + 1);
}

// per item slot, the triangle's {pa, e0, e1} record (zeros for non-triangles)
std::vector<double> triangles_in_item_order(const AccelBuild& ab, const std::vector<double>& tripre) {
    std::vector<double> tripre2;
    if (tripre.empty()) return tripre2;
    const size_t n_items = ab.items.size() / 2;
    tripre2.assign(n_items * 10, 0.0);
    for (size_t j = 0; j < n_items; j++) {
        uint32_t kp = ab.items[2 * j];
        if ((kp & NK_MASK) == NK_TRI) {
            const double* src = &tripre[(size_t)(kp >> NK_BITS) * 10];
            std::copy(src, src + 10, &tripre2[j * 10]);
        }
    }
    return tripre2;
}

}  // namespace

SceneAccel build_scene_accel(std::vector<AccelContext>& ctx, bool usable, bool nested, double media_extent, const TriTables& t) {
    SceneAccel a;
    a.ab.ok = usable;
    // contexts by chain depth, outermost first (a nested instance's item lives in its parent's context; scenes of depth <= 1: 1, 2, 3 ...)
    std::vector<size_t> by_depth;
    for (size_t i = 1; i < ctx.size(); i++) by_depth.push_back(i);
    std::stable_sort(by_depth.begin(), by_depth.end(), [&](size_t x, size_t y) { return ctx[x].depth < ctx[y].depth; });
    if (a.ab.ok) tighten_instance_boxes(ctx, by_depth);
    build_bvhs(a, ctx, by_depth, nested, media_extent, t);
    if (a.ab.max_depth + 2 > ACCEL_MAX_STACK) a.ab.ok = false;
    if (a.ab.ok) {
        sort_nodes_by_depth(a);
        a.tripre2 = triangles_in_item_order(a.ab, t.tripre);
    } else {  // an unusable accel leaves no tables behind (the depths and counts stay what they were when it gave up)
        a.ab.nodes.clear();
        a.ab.items.clear();
        a.ab.inst.clear();
    }
    return a;
}

}  // namespace rtamd
