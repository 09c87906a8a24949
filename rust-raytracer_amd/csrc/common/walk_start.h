// Where a closest-hit walk of the world BVH2 begins.
//
// The walks descend near child first and never test a popped entry against the ray they have shortened since.  A scene whose root has a
// LEAF child as large as the whole scene -- the ground sphere of the book scenes, alone in a leaf under the root -- therefore meets that leaf
// last on nearly every ray: the origins lie in or above the other child's box, the leaf is pushed, and each lane pops it at the end of
// its own walk, in whatever round that is, having walked until then without the one bound most rays end on.  Starting AT that leaf,
// with the other child as the one stack entry, tests it once for every lane of a wave in step and hands the bound to the whole descent.
//
// The rule, on the root's Node2 record as the blob stores it (f32 planes, stored pads):
//   child k qualifies  iff  it is a leaf, the two child refs differ, and  2 * area(box k) >= area(union of both boxes);
//   child 0 qualifies            ->  {child 0, child 1}
//   else child 1 qualifies       ->  {child 1, child 0}
//   else                         ->  {root, WALK_START_NONE}: the walk as it always was.
// The area test keeps a small leaf that most rays miss from being tested by every lane; one half is a condition, not a tuned number (a
// ground leaf's ratio is close to 1, two leaves of like size are near 1/2 and below once their boxes are apart).  The refs differ in every
// tree but the one-item BVH (host/accel.cpp: both refs name the same leaf, the second box is a point), which is left alone.  Anything
// that is not a number fails the comparison and gives the root.
// Only the ORDER of visits changes: the candidates a walk accepts do not depend on it (smaller t, an exact tie to the later item in
// reference order), so neither does its result.  Host and device run the code below; tests/test_walk_start.py drives it from a host program.
#pragma once
#include <cstdint>

#include "flat.h"

#if defined(__HIPCC__)
#define RT_WALK_START_HD __host__ __device__
#else
#define RT_WALK_START_HD
#endif

namespace rtamd {

static const uint32_t WALK_START_NONE = REF_DONE;  // push_ref of a walk that starts at the root: nothing to push

struct WalkStart {
    uint32_t start_ref, push_ref;  // refs as the Node2 record holds them
};

// surface area of the box [lo, hi], in f64 from the f32 planes (every product and sum of f32 differences below is far inside f64's range)
RT_WALK_START_HD inline double walk_start_area(const float lo[3], const float hi[3]) {
    const double x = (double)hi[0] - (double)lo[0], y = (double)hi[1] - (double)lo[1], z = (double)hi[2] - (double)lo[2];
    return 2. * (x * y + y * z + z * x);
}

// area of child k's box and of the union of both child boxes
RT_WALK_START_HD inline void walk_start_areas(const Node2& root, int k, double& child, double& both) {
    const float lo[3] = {root.lo_x[k], root.lo_y[k], root.lo_z[k]}, hi[3] = {root.hi_x[k], root.hi_y[k], root.hi_z[k]};
    const float ulo[3] = {root.lo_x[0] < root.lo_x[1] ? root.lo_x[0] : root.lo_x[1], root.lo_y[0] < root.lo_y[1] ? root.lo_y[0] : root.lo_y[1],
                          root.lo_z[0] < root.lo_z[1] ? root.lo_z[0] : root.lo_z[1]};
    const float uhi[3] = {root.hi_x[0] > root.hi_x[1] ? root.hi_x[0] : root.hi_x[1], root.hi_y[0] > root.hi_y[1] ? root.hi_y[0] : root.hi_y[1],
                          root.hi_z[0] > root.hi_z[1] ? root.hi_z[0] : root.hi_z[1]};
    child = walk_start_area(lo, hi);
    both = walk_start_area(ulo, uhi);
}

RT_WALK_START_HD inline bool walk_start_qualifies(const Node2& root, int k) {
    if ((root.child[k] >> REF_TAG_SHIFT) != 1u || root.child[0] == root.child[1]) return false;
    double a, u;
    walk_start_areas(root, k, a, u);
    return u > 0. && 2. * a >= u;  // (false for anything that is not a number)
}

RT_WALK_START_HD inline WalkStart walk_start(const Node2& root, uint32_t root_ref) {
    if (walk_start_qualifies(root, 0)) return WalkStart{root.child[0], root.child[1]};
    if (walk_start_qualifies(root, 1)) return WalkStart{root.child[1], root.child[0]};
    return WalkStart{root_ref, WALK_START_NONE};
}

}  // namespace rtamd
