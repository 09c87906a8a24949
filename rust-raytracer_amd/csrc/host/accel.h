// Host-side builder of the kernel-2 acceleration structure (common/flat.h "Accel").
#pragma once
#include <cstdint>
#include <map>
#include <vector>

#include "scene.h"

namespace rtamd {

struct AccelItem {
    Box box;         // f64 box in the space of its BVH (world, or object space under a Transform)
    uint32_t kp;     // kind | payload << 4
    int32_t order;   // DFS index of the primitive in the reference-order program (tie rule)
};
struct AccelBuild {
    std::vector<Node2> nodes;
    std::vector<uint32_t> items;  // 2 words per item
    std::vector<uint32_t> inst;   // 2 words per instance
    int max_depth = 0;            // deepest root-to-leaf path over all BVHs
    bool ok = true;
};
// Builds one BVH2 (binned SAH) over `items`, boxes padded by `pad` and rounded outward to f32.
// Returns the root ref.  `depth0` is the stack depth already used above this BVH.
uint32_t accel_build_bvh(AccelBuild& out, std::vector<AccelItem>& items, double pad, int depth0);

// The items of one BVH as the flattener collects them: context 0 = world space, context 1+i = object space of instance i
struct AccelContext {
    std::vector<AccelItem> items;
    std::map<int, size_t> of;  // object id -> item slot (a re-emitted object keeps one slot, latest order)
    uint32_t xform = 0;
    const double* Minv = nullptr;  // the chain's innermost level: parent's space <-> this context's object space
    const double* M = nullptr;
    uint32_t chain = 0;    // nested scenes: the instance record carries the chain instead of the xform
    size_t parent = 0;     // context of the enclosing chain (0: world space)
    uint32_t depth = 1;    // levels of the chain
};
// The triangle tables the accel reads (the flattener's): 4 words per triangle, the global vertex table, the hoisted {pa, e0, e1, pad}
struct TriTables {
    const std::vector<uint32_t>& tris;
    const std::vector<double>& vpos;
    const std::vector<double>& tripre;
};
// The accel of a scene: every BVH in one Node2 / item array, and what FlatView says about them.  `ab.ok` is the one notion of "the accel
// is usable"; when it is false the rest only holds what the stages had computed by the time they gave up.
struct SceneAccel {
    AccelBuild ab;
    uint32_t root2 = REF_DONE, max_inst_nodes = 0, inst_depth = 0, n_world_items = 0, world_depth = 0, stack_inline = 0, world_top = 0;
    std::vector<char> compact_cand;  // per instance: only triangles with f32 vertices (kernels 5 / 6 can defer it)
    std::vector<double> inst_oo;     // per instance: bound of |object-space ray origin|
    double origin_limit = 0.;
    std::vector<double> tripre2;     // triangle records in ACCEL ITEM order: a leaf's 1..4 triangles are contiguous
};
// ctx: the flattener's contexts (their instance items are tightened and reclassified in place); usable: nothing the flattener met rules
// the accel out; nested: instance records carry chain ids; media_extent: largest |coordinate| of the media's boxes
SceneAccel build_scene_accel(std::vector<AccelContext>& ctx, bool usable, bool nested, double media_extent, const TriTables& t);

}  // namespace rtamd
