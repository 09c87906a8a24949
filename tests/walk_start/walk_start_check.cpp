// Stand-alone host check of csrc/common/walk_start.h (tests/test_walk_start.py builds and runs it): the start rule on hand-made root
// records and on the roots the product's own builder (csrc/host/accel.cpp) makes for sphere lists.
//   walk_start_check [NAME SPHERES.txt]...      SPHERES.txt: lines of  cx cy cz r  in the scene's order
// For every list it prints one line  "tree NAME: ..."  with the root's refs, both area ratios and the rule's answer; the test reads them.
#include "host/accel.cpp"

#include <cstdio>
#include <fstream>

#include "common/walk_start.h"

namespace rtamd {
Tuning tuning() { return Tuning{}; }  // the builder's only link into the rest of the host
}  // namespace rtamd

using namespace rtamd;

static long failures = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

static const uint32_t ROOT_REF = 7u;  // any inner ref: the rule hands it back untouched

static void set_box(Node2& nd, int k, float lx, float ly, float lz, float hx, float hy, float hz) {
    nd.lo_x[k] = lx; nd.lo_y[k] = ly; nd.lo_z[k] = lz;
    nd.hi_x[k] = hx; nd.hi_y[k] = hy; nd.hi_z[k] = hz;
}
static uint32_t leaf(uint32_t first, uint32_t count) { return REF_LEAF | ((count - 1u) << REF_LEAF_COUNT_SHIFT) | first; }
static bool is(const WalkStart& w, uint32_t start, uint32_t push) { return w.start_ref == start && w.push_ref == push; }
static double ratio(const Node2& nd, int k) {
    double a, u;
    walk_start_areas(nd, k, a, u);
    return a / u;
}

static void hand_made() {
    Node2 nd{};
    // a ground leaf under a slab of inner nodes, as the book scenes have it: child 0 a leaf of 200^3, child 1 inner, 30 x 1 x 30 on top of it
    set_box(nd, 0, -100.f, -200.5f, -100.f, 100.f, -0.5f, 100.f);
    set_box(nd, 1, -15.f, -0.5f, -15.f, 15.f, 0.5f, 15.f);
    nd.child[0] = leaf(0, 1); nd.child[1] = 1u;
    CHECK(is(walk_start(nd, ROOT_REF), leaf(0, 1), 1u), "ground leaf as child 0");
    CHECK(ratio(nd, 0) > 0.99 && ratio(nd, 0) <= 1., "ground leaf: ratio %.6f", ratio(nd, 0));
    // the same with the children exchanged: a large leaf as child 1
    set_box(nd, 1, -100.f, -200.5f, -100.f, 100.f, -0.5f, 100.f);
    set_box(nd, 0, -15.f, -0.5f, -15.f, 15.f, 0.5f, 15.f);
    nd.child[1] = leaf(0, 1); nd.child[0] = 1u;
    CHECK(is(walk_start(nd, ROOT_REF), leaf(0, 1), 1u), "large leaf as child 1");
    // two inner children, whatever their boxes
    nd.child[0] = 1u; nd.child[1] = 2u;
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "two inner children");
    // two leaves of the same size, a box's width apart: 6 / 14 of the union's area each
    set_box(nd, 0, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    set_box(nd, 1, 2.f, 0.f, 0.f, 3.f, 1.f, 1.f);
    nd.child[0] = leaf(0, 2); nd.child[1] = leaf(2, 3);
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "two leaves of the same size, apart (ratio %.4f)", ratio(nd, 0));
    CHECK(ratio(nd, 0) < 0.5 && ratio(nd, 1) < 0.5, "two like leaves: ratios %.4f %.4f", ratio(nd, 0), ratio(nd, 1));
    // a small leaf far away from a large inner child: far under half
    set_box(nd, 0, 50.f, 50.f, 50.f, 50.5f, 50.5f, 50.5f);
    set_box(nd, 1, -10.f, -10.f, -10.f, 10.f, 10.f, 10.f);
    nd.child[0] = leaf(0, 1); nd.child[1] = 1u;
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "a small far leaf (ratio %.6f)", ratio(nd, 0));
    CHECK(ratio(nd, 0) < 1e-3, "a small far leaf: ratio %.6f", ratio(nd, 0));
    // ... and with the large child a leaf as well, still nothing: the union reaches out to the small one, 2 400 of 21 961.5
    nd.child[1] = leaf(1, 4);
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "a large leaf with a small one far off (ratio %.4f)", ratio(nd, 1));
    // a small leaf beside a large one: the large one qualifies, as child 1
    set_box(nd, 0, 10.f, 0.f, 0.f, 10.5f, 0.5f, 0.5f);
    CHECK(is(walk_start(nd, ROOT_REF), leaf(1, 4), leaf(0, 1)), "a large leaf beside a small one");
    // both qualify (one leaf's box inside the other's, more than half its area): child 0
    set_box(nd, 0, 0.f, 0.f, 0.f, 9.f, 9.f, 9.f);
    set_box(nd, 1, 0.f, 0.f, 0.f, 10.f, 10.f, 10.f);
    nd.child[0] = leaf(0, 1); nd.child[1] = leaf(1, 1);
    CHECK(ratio(nd, 0) >= 0.5 && ratio(nd, 1) >= 0.5, "both qualify: ratios %.4f %.4f", ratio(nd, 0), ratio(nd, 1));
    CHECK(is(walk_start(nd, ROOT_REF), leaf(0, 1), leaf(1, 1)), "both qualify: child 0 starts");
    // one half is a condition (>=): a 2 x 2 x 1 leaf has 16 of the 32 of a 2 x 2 x 3 union, and starts the walk; with the union one ulp
    // taller it does not; nor does a 2 x 1 x 0.5 leaf with 7 of the 16 of a 2 x 1 x 2 union
    set_box(nd, 0, 0.f, 0.f, 0.f, 2.f, 2.f, 1.f);
    set_box(nd, 1, 0.f, 0.f, 1.f, 2.f, 2.f, 3.f);
    nd.child[0] = leaf(0, 1); nd.child[1] = 1u;
    {
        double a, u;
        walk_start_areas(nd, 0, a, u);
        CHECK(a == 16. && u == 32., "areas %.17g %.17g", a, u);
    }
    CHECK(is(walk_start(nd, ROOT_REF), leaf(0, 1), 1u), "exactly one half");
    nd.hi_z[1] = std::nextafterf(3.f, 4.f);
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "an ulp under one half");
    set_box(nd, 0, 0.f, 0.f, 0.f, 2.f, 1.f, 0.5f);
    set_box(nd, 1, 0.f, 0.f, 0.5f, 2.f, 1.f, 2.f);
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "7 of 16");
    // anything that is not a number, and two points, give the root
    set_box(nd, 0, 0.f, NAN, 0.f, 2.f, 2.f, 1.f);
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "a NaN plane");
    set_box(nd, 0, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f);
    set_box(nd, 1, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f);
    nd.child[0] = leaf(0, 1); nd.child[1] = leaf(1, 1);
    CHECK(is(walk_start(nd, ROOT_REF), ROOT_REF, WALK_START_NONE), "two points");
}

// the world BVH of a sphere list as build_bvhs makes it: item boxes c -+ r, pad 3 * 2^-22 * 64 * extent
static uint32_t build_tree(const std::vector<double>& s, AccelBuild& ab) {
    const size_t n = s.size() / 4;
    std::vector<AccelItem> items(n);
    double ew = 0.;
    for (size_t i = 0; i < n; i++) {
        Box b;
        for (int k = 0; k < 3; k++) {
            b.mn[k] = s[4 * i + k] - std::fabs(s[4 * i + 3]);
            b.mx[k] = s[4 * i + k] + std::fabs(s[4 * i + 3]);
            ew = std::fmax(ew, std::fmax(std::fabs(b.mn[k]), std::fabs(b.mx[k])));
        }
        items[i] = AccelItem{b, NK_SPHERE | ((uint32_t)i << NK_BITS), (int32_t)i};
    }
    return accel_build_bvh(ab, items, 3. * std::ldexp(64. * ew, -22), 0);
}

int main(int argc, char** argv) {
    hand_made();
    // a one-item scene: both refs name the one leaf, whose box is all of the union -- left alone
    {
        AccelBuild ab;
        const uint32_t root = build_tree({0., 0., 0., 100.}, ab);
        CHECK(ab.ok && root == 0u && ab.nodes.size() == 1 && ab.nodes[0].child[0] == ab.nodes[0].child[1], "one-item BVH");
        CHECK(is(walk_start(ab.nodes[root], root), root, WALK_START_NONE), "a one-item scene is left alone");
    }
    for (int i = 1; i + 1 < argc; i += 2) {
        std::ifstream in(argv[i + 1]);
        std::vector<double> s;
        double v;
        while (in >> v) s.push_back(v);
        CHECK(!s.empty() && s.size() % 4 == 0, "%s: not a sphere list", argv[i + 1]);
        if (s.empty() || s.size() % 4 != 0) continue;
        AccelBuild ab;
        const uint32_t root = build_tree(s, ab);
        CHECK(ab.ok && (root >> REF_TAG_SHIFT) == 0u, "%s: no BVH", argv[i]);
        if (!ab.ok) continue;
        const Node2& nd = ab.nodes[root];
        const WalkStart w = walk_start(nd, root);
        double ground_r = 0.;  // the radius of the start leaf's one sphere (0: no start leaf, or more than one item)
        if (w.push_ref != WALK_START_NONE && ((w.start_ref >> REF_LEAF_COUNT_SHIFT) & 7u) == 0u)
            ground_r = s[4 * (size_t)(ab.items[2 * (size_t)(w.start_ref & REF_LEAF_FIRST_MASK)] >> NK_BITS) + 3];
        printf("tree %s: spheres %zu root %u child0 0x%08x child1 0x%08x ratio0 %.6f ratio1 %.6f start 0x%08x push 0x%08x start_radius %g\n", argv[i], s.size() / 4, root,
               nd.child[0], nd.child[1], (nd.child[0] >> REF_TAG_SHIFT) == 1u ? ratio(nd, 0) : 0., (nd.child[1] >> REF_TAG_SHIFT) == 1u ? ratio(nd, 1) : 0., w.start_ref,
               w.push_ref, ground_r);
    }
    if (failures) {
        printf("walk_start_check: %ld FAILURES\n", failures);
        return 1;
    }
    printf("walk_start_check: ok\n");
    return 0;
}
