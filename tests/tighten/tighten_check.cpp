// Stand-alone host check of csrc/common/tighten.h over BVHs built by the product's own builder (tests/test_tighten.py builds and runs it).
// For random item boxes at four coordinate scales and render origin bounds from the scene's extent up to and beyond origin_limit2:
// every tightened child box contains the union of its items' boxes grown by pad_r on every side (compared in long double), lies
// inside the stored box, and equals the stored box when shrink is 0.
#include "host/accel.cpp"

#include <cstdio>
#include <random>

#include "common/tighten.h"

namespace rtamd {
Tuning tuning() { return Tuning{}; }  // the builder's only link into the rest of the host
}  // namespace rtamd

using namespace rtamd;

struct LBox {
    long double mn[3], mx[3];
};
static long failures = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

// union of the item boxes under `ref` (boxes indexed by the item's order)
static LBox subtree(const AccelBuild& ab, const std::vector<Box>& boxes, uint32_t ref) {
    LBox u;
    for (int k = 0; k < 3; k++) { u.mn[k] = INFINITY; u.mx[k] = -INFINITY; }
    if ((ref >> REF_TAG_SHIFT) == 1u) {
        const uint32_t first = ref & REF_LEAF_FIRST_MASK, cnt = ((ref >> REF_LEAF_COUNT_SHIFT) & 7u) + 1u;
        for (uint32_t i = 0; i < cnt; i++) {
            const Box& b = boxes[ab.items[2 * (size_t)(first + i) + 1]];
            for (int k = 0; k < 3; k++) { u.mn[k] = std::fmin(u.mn[k], (long double)b.mn[k]); u.mx[k] = std::fmax(u.mx[k], (long double)b.mx[k]); }
        }
        return u;
    }
    const Node2& nd = ab.nodes[ref];
    for (int c = 0; c < 2; c++) {
        const LBox s = subtree(ab, boxes, nd.child[c]);
        for (int k = 0; k < 3; k++) { u.mn[k] = std::fmin(u.mn[k], s.mn[k]); u.mx[k] = std::fmax(u.mx[k], s.mx[k]); }
    }
    return u;
}

static void child_box(const Node2& nd, int c, float lo[3], float hi[3]) {
    lo[0] = nd.lo_x[c]; lo[1] = nd.lo_y[c]; lo[2] = nd.lo_z[c];
    hi[0] = nd.hi_x[c]; hi[1] = nd.hi_y[c]; hi[2] = nd.hi_z[c];
}

int main() {
    const double scales[4] = {1e-3, 1., 1e3, 1e5};
    std::mt19937_64 gen(20251019);
    std::uniform_real_distribution<double> uni(-1., 1.), size(1e-3, 0.1);
    long boxes_checked = 0, planes_moved = 0;
    for (double scale : scales) {
        const int n = 2000;
        std::vector<AccelItem> items(n);
        std::vector<Box> boxes(n);
        double ew = 0.;
        for (int i = 0; i < n; i++) {
            Box b;
            for (int k = 0; k < 3; k++) {
                const double c = scale * uni(gen), h = scale * size(gen);
                b.mn[k] = c - h;
                b.mx[k] = c + h;
                ew = std::fmax(ew, std::fmax(std::fabs(b.mn[k]), std::fabs(b.mx[k])));
            }
            boxes[i] = b;
            items[i] = AccelItem{b, NK_SPHERE | ((uint32_t)i << NK_BITS), i};
        }
        // as build_bvhs pads the world BVH
        const double limit = 64. * ew, pad_w = 3. * std::ldexp(limit, -22);
        AccelBuild ab;
        const uint32_t root = accel_build_bvh(ab, items, pad_w, 0);
        CHECK(ab.ok && (root >> REF_TAG_SHIFT) == 0u, "scale %g: no BVH", scale);
        std::vector<LBox> unions(2 * ab.nodes.size());
        for (size_t i = 0; i < ab.nodes.size(); i++)
            for (int c = 0; c < 2; c++) unions[2 * i + c] = subtree(ab, boxes, ab.nodes[i].child[c]);

        const double bounds[6] = {render_origin_bound(limit, 0.), 8. * ew, limit * (1. - 1. / 1024.), limit, 2. * limit, 1e300};
        CHECK(bounds[0] == 2. * ew, "render_origin_bound(limit, 0) is not 2 ew");
        CHECK(render_origin_bound(limit, 5. * ew) == 10. * ew, "render_origin_bound(limit, 5 ew) is not 10 ew");
        float prev = INFINITY;
        for (int bi = -1; bi < 6; bi++) {
            // bi = -1: O_r = ew itself (the smallest bound the proof allows), not reachable through render_origin_bound
            const double o_r = bi < 0 ? ew : bounds[bi];
            const float shrink = box_shrink(limit, o_r, true);
            const long double pad_r = 3.0L * std::ldexp((long double)std::fmin(o_r, limit), -22);
            CHECK(box_shrink(limit, o_r, false) == 0.f, "scale %g O_r %g: an ineligible scene has shrink %g", scale, o_r, (double)box_shrink(limit, o_r, false));
            CHECK(shrink >= 0.f && shrink <= prev, "scale %g O_r %g: shrink %g is not monotonic", scale, o_r, (double)shrink);
            CHECK((long double)shrink <= (long double)pad_w - pad_r, "scale %g O_r %g: shrink %g above pad_w - pad_r", scale, o_r, (double)shrink);
            if (o_r >= limit) CHECK(shrink == 0.f, "scale %g O_r %g: shrink %g at or beyond the limit", scale, o_r, (double)shrink);
            else CHECK(shrink > 0.f && (double)shrink >= 0.999 * (double)((long double)pad_w - pad_r), "scale %g O_r %g: shrink %g is not the pad difference", scale, o_r, (double)shrink);
            prev = shrink;
            for (size_t i = 0; i < ab.nodes.size(); i++)
                for (int c = 0; c < 2; c++) {
                    float lo[3], hi[3], slo[3], shi[3];
                    child_box(ab.nodes[i], c, slo, shi);
                    child_box(ab.nodes[i], c, lo, hi);
                    tighten_box(lo, hi, shrink);
                    const LBox& u = unions[2 * i + c];
                    boxes_checked++;
                    for (int k = 0; k < 3; k++) {
                        CHECK((long double)lo[k] <= u.mn[k] - pad_r && (long double)hi[k] >= u.mx[k] + pad_r,
                              "scale %g O_r %g node %zu child %d axis %d: [%.9g, %.9g] does not hold [%.17Lg, %.17Lg] -+ %.9Lg", scale, o_r, i, c, k,
                              (double)lo[k], (double)hi[k], u.mn[k], u.mx[k], pad_r);
                        CHECK(lo[k] >= slo[k] && hi[k] <= shi[k], "scale %g O_r %g node %zu child %d axis %d: outside the stored box", scale, o_r, i, c, k);
                        if (shrink == 0.f) CHECK(lo[k] == slo[k] && hi[k] == shi[k], "scale %g node %zu: shrink 0 moved a plane", scale, i);
                        planes_moved += (lo[k] != slo[k]) + (hi[k] != shi[k]);
                    }
                }
        }
        // a one-item BVH: the zero-size second child stays a point, the first is tightened like any other
        std::vector<AccelItem> one(1, AccelItem{boxes[0], NK_SPHERE, 0});
        AccelBuild ab1;
        const uint32_t r1 = accel_build_bvh(ab1, one, pad_w, 0);
        CHECK(ab1.ok && r1 == 0u && ab1.nodes.size() == 1, "scale %g: one-item BVH", scale);
        float lo[3], hi[3], slo[3], shi[3];
        child_box(ab1.nodes[0], 1, lo, hi);
        child_box(ab1.nodes[0], 1, slo, shi);
        tighten_box(lo, hi, box_shrink(limit, ew, true));
        for (int k = 0; k < 3; k++) CHECK(lo[k] == slo[k] && hi[k] == shi[k] && lo[k] == hi[k], "scale %g: the empty child moved", scale);
    }
    CHECK(planes_moved > boxes_checked, "the check is vacuous: %ld planes moved over %ld boxes", planes_moved, boxes_checked);
    CHECK(box_shrink(NAN, 1., true) == 0.f && box_shrink(64., NAN, true) == 0.f && box_shrink(INFINITY, 1., true) == 0.f, "not-a-number bounds");
    if (failures) {
        printf("tighten_check: %ld FAILURES\n", failures);
        return 1;
    }
    printf("tighten_check: ok (%ld child boxes, %ld planes moved)\n", boxes_checked, planes_moved);
    return 0;
}
