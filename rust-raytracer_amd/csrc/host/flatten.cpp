// Flattener: object graph -> linear DFS pre-order program + SoA tables in one blob
// (layout: common/flat.h).  The emission order IS the reference's visit order:
//   BVHNode::hit   box, then left subtree, then right subtree   (bvh.rs:86-102)
//   Vec<..>::hit   items in insertion order                     (hit.rs:57-67)
//   Cube::hit      its 6 sides as a list -- ONE node, the scan is inside the kernel's cube_hit  (cube.rs:64-66)
//   Mesh::hit      its inner BVHNode                            (mesh.rs:201-203)
//   Transform::hit enter object space, inner object, leave      (transform.rs:152-165)
// so the kernel's closest-hit update ("accept when t <= best", later wins ties)
// reproduces the reference's result including its tie rule.
#include <cstring>
#include <map>
#include <string>
#include <utility>

#include <algorithm>
#include <cmath>

#include "accel.h"
#include "scene.h"

namespace rtamd {

namespace {

// Program emission: walks the object graph once and appends to the tables of the hot part, and collects the accel's items per context.
struct Builder {
    const rt_scene& s;
    std::vector<uint32_t> meta;
    std::vector<double> boxes, spheres, rects, xforms, vpos, vnrm;
    std::vector<int32_t> sphere_mat, rect_mat;
    std::vector<uint32_t> tris;
    std::vector<double> tripre;  // per triangle: pa, e0 = pb - pa, e1 = pc - pa, pad (10 doubles = 80 B)
    std::vector<MediumDev> media;
    std::vector<double> msph;  // moving spheres: {center0, center1, time0, time1, radius, material} (10 f64)
    std::map<int, uint32_t> msph_of;
    double media_extent = 0.;  // largest |coordinate| of the media's bounding boxes: scatter points inside a medium are ray origins too
    int medium_depth = 0;
    std::map<int, uint32_t> sphere_of, rect_of, tri_of, xform_of;  // (rect_of: rectangles and cubes share the rect table)
    int n_cubes = 0;
    std::vector<uint32_t> mesh_base;
    uint32_t kinds = 0;
    int xf_depth = 0, depth = 0, max_depth = 0;
    std::map<int, bool> in_xform;  // object id -> emitted inside a Transform
    std::map<int, bool> in_medium;  // object id -> emitted inside the boundary of a ConstantMedium
    // accel (kernel 2) item collection: context 0 = world space, context 1+i = object space of instance i
    std::vector<AccelContext> actx{1};
    std::vector<size_t> ctx_stack{0};
    std::map<uint32_t, size_t> ctx_of_chain;  // chain -> its context (one per chain: a Transform under two parents has two)
    bool accel_ok = true;  // nothing emitted so far rules the accel out (handed to build_scene_accel)
    // chains of Transforms (common/flat.h "Nested Transforms"): one per distinct path from the root, keyed by (parent chain, xform)
    std::vector<ChainRec> chains;
    std::map<std::pair<int32_t, uint32_t>, uint32_t> chain_of;
    int32_t cur_chain = -1;
    uint32_t xf_nest = 0;  // levels of the deepest chain
    std::vector<std::pair<uint32_t, uint32_t>> xf_begin, xf_end;  // {node, chain} / {node, parent chain + 1}: the nested payloads

    // global vertex table: meshes concatenated
    explicit Builder(const rt_scene& sc) : s(sc) {
        uint32_t nv = 0;
        for (auto& m : s.meshes) {
            mesh_base.push_back(nv);
            nv += (uint32_t)(m->pos.size() / 3);
            vpos.insert(vpos.end(), m->pos.begin(), m->pos.end());
            vnrm.insert(vnrm.end(), m->nrm.begin(), m->nrm.end());
        }
    }

    void accel_item(int obj_id, const ObjectRec& o, uint32_t kp, uint32_t node_index, const Box* tight = nullptr) {
        if (medium_depth > 0) return;  // the boundary of a ConstantMedium is not a surface: only the medium's own two queries see it
        AccelContext& c = actx[ctx_stack.back()];
        if (!o.has_box) {
            accel_ok = false;
            return;
        }
        auto it = c.of.find(obj_id);
        if (it == c.of.end()) {
            c.of.emplace(obj_id, c.items.size());
            c.items.push_back(AccelItem{tight ? *tight : o.box, kp, (int32_t)node_index});
        } else {
            c.items[it->second].order = (int32_t)node_index;  // the later visit wins ties (Q5/Q14)
        }
    }

    uint32_t node(uint32_t kind, uint32_t payload, uint32_t skip = 0) {
        if (payload >= (1u << (32 - NK_BITS))) throw RtError(RT_ERR_UNSUPPORTED, "scene too large for 28-bit payload index");
        meta.push_back(kind | (payload << NK_BITS));
        meta.push_back(skip);
        kinds |= 1u << kind;
        return (uint32_t)(meta.size() / 2 - 1);
    }
    // a primitive is one node of the program and one item of the current accel context
    void leaf(int id, const ObjectRec& o, uint32_t kind, uint32_t payload, const Box* tight = nullptr) {
        const uint32_t n = node(kind, payload);
        accel_item(id, o, kind | (payload << NK_BITS), n, tight);
    }

    // the object's record in a table: index `next`, written by add() at the object's first use
    template <class Add>
    uint32_t slot(std::map<int, uint32_t>& of, int id, size_t next, Add add) {
        auto it = of.find(id);
        if (it != of.end()) return it->second;
        add();
        return of.emplace(id, (uint32_t)next).first->second;
    }
    // (used by emit, and by the light table for a light that is not part of the hitable list: still addressable)
    uint32_t sphere_slot(int id) {
        const ObjectRec& o = s.objects[id];
        return slot(sphere_of, id, sphere_mat.size(), [&] {
            spheres.insert(spheres.end(), {o.c[0], o.c[1], o.c[2], o.r});
            sphere_mat.push_back(o.material);
        });
    }
    uint32_t rect_slot(int id) {
        const ObjectRec& o = s.objects[id];
        return slot(rect_of, id, rect_mat.size(), [&] {
            rects.insert(rects.end(), {o.a0, o.b0, o.a1, o.b1, o.k, 0.0});
            rect_mat.push_back(o.material);
        });
    }

    void emit_moving_sphere(int id, const ObjectRec& o) {  // D9
        leaf(id, o, NK_MSPHERE, slot(msph_of, id, msph.size() / 10, [&] {
                 msph.insert(msph.end(), {o.c[0], o.c[1], o.c[2], o.c1[0], o.c1[1], o.c1[2], o.time0, o.time1, o.r, (double)o.material});
             }));
    }
    void emit_triangle(int id, const ObjectRec& o) {
        const double* P = s.meshes[o.mesh]->pos.data();
        const double *pa = P + 3 * o.ia, *pb = P + 3 * o.ib, *pc = P + 3 * o.ic;
        const uint32_t tri = slot(tri_of, id, tris.size() / 4, [&] {
            uint32_t base = mesh_base[o.mesh];
            tris.insert(tris.end(), {base + o.ia, base + o.ib, base + o.ic, (uint32_t)o.material});
            // what Triangle::hit recomputes per call (mesh.rs:69): edge = [pb - pa, pc - pa]; same f64 subtractions
            tripre.insert(tripre.end(), {pa[0], pa[1], pa[2], pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2], pc[0] - pa[0], pc[1] - pa[1],
                                         pc[2] - pa[2], 0.0});
        });
        // accel: the TIGHT vertex box (the reference's +-0.1 object-space padding, mesh.rs:33-42, only serves its
        // own BVH; any box containing the triangle prunes correctly)
        Box tb;
        for (int a = 0; a < 3; a++) {
            tb.mn[a] = std::fmin(std::fmin(pa[a], pb[a]), pc[a]);
            tb.mx[a] = std::fmax(std::fmax(pa[a], pb[a]), pc[a]);
        }
        leaf(id, o, NK_TRI, tri, &tb);
    }
    void emit_cube(int id, const ObjectRec& o) {  // one record in the rect table + one node (flat.h NK_CUBE); o.box is exactly (box_min, box_max), cube.rs:67-69
        const uint32_t rec = slot(rect_of, id, rect_mat.size(), [&] {
            rects.insert(rects.end(), {o.box.mn[0], o.box.mn[1], o.box.mn[2], o.box.mx[0], o.box.mx[1], o.box.mx[2]});
            rect_mat.push_back(o.material);
            n_cubes++;
        });
        if (rec >= (1u << (32 - NK_BITS - 3))) throw RtError(RT_ERR_UNSUPPORTED, "scene too large for the cube payload (record index * 8 + side)");
        leaf(id, o, NK_CUBE, rec * 8u);
    }
    void emit_bvh(const ObjectRec& o) {
        uint32_t bi = (uint32_t)(boxes.size() / 6);
        boxes.insert(boxes.end(), {o.box.mn[0], o.box.mn[1], o.box.mn[2], o.box.mx[0], o.box.mx[1], o.box.mx[2]});
        uint32_t n = node(NK_BOX, bi);
        if (bi >= 0x7FFFFFFFu) throw RtError(RT_ERR_UNSUPPORTED, "too many BVH nodes");
        emit(o.children[0]);
        emit(o.children[1]);
        meta[2 * n + 1] = (uint32_t)(meta.size() / 2);
    }

    // the chain a visit of Transform `xf` under chain `parent` enters: the same Transform under two different parents is two chains (each
    // transforms with its own matrices)
    uint32_t chain_slot(int32_t parent, uint32_t xf) {
        auto ch = chain_of.find({parent, xf});
        if (ch != chain_of.end()) return ch->second;
        ChainRec r{};
        if (parent >= 0) r = chains[parent];
        if (r.depth >= XF_MAX_DEPTH)
            throw RtError(RT_ERR_UNSUPPORTED, "Transforms nested deeper than " + std::to_string(XF_MAX_DEPTH) + " levels are not supported");
        r.xf[r.depth++] = xf;
        r.inner = xf;
        if (chains.size() >= (1u << (32 - NK_BITS)) - 1u) throw RtError(RT_ERR_UNSUPPORTED, "scene too large for 28-bit chain ids");
        chains.push_back(r);
        xf_nest = std::max(xf_nest, r.depth);
        return chain_of.emplace(std::make_pair(parent, xf), (uint32_t)(chains.size() - 1)).first->second;
    }
    // the accel context of a chain: the Transform is one item of the enclosing space; its subtree gets its own object-space BVH
    // (a Transform emitted twice -- BVHNode::new's 1-object leaf, Q14 -- re-enters its own context, so its
    // items take the later visit's indices exactly as a re-emitted primitive does)
    size_t context_slot(uint32_t chain, uint32_t xf, const ObjectRec& o) {
        auto ci = ctx_of_chain.find(chain);
        if (ci != ctx_of_chain.end()) return ci->second;
        actx.push_back(AccelContext{{}, {}, xf, o.Minv, o.M, chain, ctx_stack.back(), chains[chain].depth});
        return ctx_of_chain.emplace(chain, actx.size() - 1).first->second;
    }
    void emit_transform(int id, const ObjectRec& o) {
        const uint32_t xf = slot(xform_of, id, xforms.size() / 32, [&] {
            xforms.insert(xforms.end(), o.Minv, o.Minv + 16);
            xforms.insert(xforms.end(), o.M, o.M + 16);
        });
        const int32_t parent = cur_chain;
        const uint32_t chain = chain_slot(parent, xf);
        const uint32_t n = node(NK_XFORM_BEGIN, xf);
        xf_begin.push_back({n, chain});
        cur_chain = (int32_t)chain;
        const bool in_accel = medium_depth == 0;  // a Transform inside a medium's boundary: reference-order program only, no accel context
        if (in_accel) {
            const size_t ci = context_slot(chain, xf, o);
            accel_item(id, o, NK_INSTANCE | ((uint32_t)(ci - 1) << NK_BITS), n);
            ctx_stack.push_back(ci);
        }
        xf_depth++;
        emit(o.children[0]);
        xf_depth--;
        if (in_accel) ctx_stack.pop_back();
        cur_chain = parent;
        xf_end.push_back({node(NK_XFORM_END, xf), (uint32_t)(parent + 1)});
        meta[2 * n + 1] = (uint32_t)(meta.size() / 2);
    }

    void emit_medium(const ObjectRec& o) {
        // ConstantMedium::hit consumes a random number INSIDE hit (medium.rs:37-38), so what the path draws depends on
        // the order in which the reference visits objects.  Kernel 1 walks the reference-order program; the accel kernel
        // (kernel 2) reproduces the visit order for the media only (traverse2_media in kernels.hip), which needs every
        // medium in world space (not under a Transform).
        if (medium_depth > 0) throw RtError(RT_ERR_UNSUPPORTED, "a ConstantMedium inside the boundary of a ConstantMedium is not supported");
        // one MediumDev per VISIT: BVHNode::new duplicates a single object into both children (Q14), so the reference visits
        // such a medium twice, and each visit may draw
        const uint32_t mi = (uint32_t)media.size();
        media.push_back(MediumDev{-1. / o.density, o.material, 0, 0, 0, 0, 0});
        if (xf_depth > 0) accel_ok = false;  // a medium under a Transform: reference order only
        if (o.has_box)
            for (int a = 0; a < 3; a++) media_extent = std::fmax(media_extent, std::fmax(std::fabs(o.box.mn[a]), std::fabs(o.box.mx[a])));
        else
            accel_ok = false;
        medium_depth++;
        uint32_t beg = node(NK_MEDIUM_BEGIN, mi);
        emit(o.children[0]);
        uint32_t mid = node(NK_MEDIUM_MID, mi);
        emit(o.children[0]);
        uint32_t end = node(NK_MEDIUM_END, mi);
        meta[2 * mid + 1] = end;
        media[mi].n_begin = beg;
        media[mi].n_mid = mid;
        media[mi].n_end = end;
        const ObjectRec& bo = s.objects[o.children[0]];
        auto si = sphere_of.find(o.children[0]);
        if (bo.type == OBJ_SPHERE && xf_depth == 0 && si != sphere_of.end() && mid == beg + 2 && end == mid + 2)
            media[mi].boundary_kp = NK_SPHERE | (si->second << NK_BITS);
        medium_depth--;
    }

    void emit(int id) {
        const ObjectRec& o = s.objects[id];
        if (xf_depth > 0) in_xform[id] = true;
        if (medium_depth > 0) in_medium[id] = true;
        depth++;
        if (depth > max_depth) max_depth = depth;
        switch (o.type) {
            case OBJ_SPHERE: leaf(id, o, NK_SPHERE, sphere_slot(id)); break;
            case OBJ_MOVING_SPHERE: emit_moving_sphere(id, o); break;
            case OBJ_RECT: leaf(id, o, o.axis == 0 ? NK_RECT_YZ : (o.axis == 1 ? NK_RECT_XZ : NK_RECT_XY), rect_slot(id)); break;
            case OBJ_TRIANGLE: emit_triangle(id, o); break;
            case OBJ_CUBE: emit_cube(id, o); break;
            case OBJ_LIST:
            case OBJ_MESH:
                for (int c : o.children) emit(c);
                break;
            case OBJ_BVH: emit_bvh(o); break;
            case OBJ_TRANSFORM: emit_transform(id, o); break;
            case OBJ_MEDIUM: emit_medium(o); break;
            default:
                throw RtError(RT_ERR_ARG, "unknown object type in flatten");
        }
        depth--;
    }

    // the reference-order program of the whole scene
    void emit_program() {
        emit(s.root);
        if (xf_nest < 2) return;
        // the chain walk (common/flat.h "Nested Transforms"): BEGIN / END and the accel's instance records carry chain ids
        for (auto& p : xf_begin) meta[2 * p.first] = NK_XFORM_BEGIN | (p.second << NK_BITS);
        for (auto& p : xf_end) meta[2 * p.first] = NK_XFORM_END | (p.second << NK_BITS);
    }

    // World::new's lights -> {kind, payload} pairs addressing the sphere / rect tables
    std::vector<uint32_t> light_table() {
        std::vector<uint32_t> lights;
        for (int lid : s.lights) {
            if (in_xform.count(lid)) throw RtError(RT_ERR_UNSUPPORTED, "a light under a Transform is not supported");
            const bool sphere = s.objects[lid].type == OBJ_SPHERE;
            lights.push_back(sphere ? NK_SPHERE : NK_RECT_XZ);
            lights.push_back(sphere ? sphere_slot(lid) : rect_slot(lid));
        }
        return lights;
    }
};

template <class T>
uint32_t append(std::vector<char>& blob, const std::vector<T>& v) {
    size_t off = (blob.size() + 15) & ~size_t(15);
    blob.resize(off);
    if (!v.empty()) {
        blob.resize(off + v.size() * sizeof(T));
        std::memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    }
    if (blob.size() > 0xFFFFFFF0u) throw RtError(RT_ERR_UNSUPPORTED, "flattened scene exceeds 4 GiB");
    return (uint32_t)off;
}

// ---- area lights (rtamd.h "area lights"): objects -> world-space triangles, in the order the header pins ----
struct AreaLower {
    const rt_scene& s;
    std::vector<const double*> xf;  // the Transforms above the current object, outermost first (their stored `trans`)
    std::vector<rt_area_tri>& out;
    int light;
    void tri(const double* pa, const double* pb, const double* pc) {
        double v[3][3];
        const double* src[3] = {pa, pb, pc};
        for (int k = 0; k < 3; k++) {
            double p[3] = {src[k][0], src[k][1], src[k][2]};
            for (size_t l = xf.size(); l-- > 0;) {  // innermost first (xf_point, vec3.rs:174-178)
                const double* t = xf[l];
                double o[3];
                for (int i = 0; i < 3; i++) o[i] = t[i * 4 + 0] * p[0] + t[i * 4 + 1] * p[1] + t[i * 4 + 2] * p[2] + t[i * 4 + 3] * 1.;
                for (int i = 0; i < 3; i++) p[i] = o[i];
            }
            for (int i = 0; i < 3; i++) v[k][i] = p[i];
        }
        rt_area_tri r{};
        for (int i = 0; i < 3; i++) {
            r.a[i] = v[0][i];
            r.e0[i] = v[1][i] - v[0][i];
            r.e1[i] = v[2][i] - v[0][i];
        }
        r.n[0] = r.e0[1] * r.e1[2] - r.e0[2] * r.e1[1];
        r.n[1] = r.e0[2] * r.e1[0] - r.e0[0] * r.e1[2];
        r.n[2] = r.e0[0] * r.e1[1] - r.e0[1] * r.e1[0];
        r.area2 = std::sqrt(r.n[0] * r.n[0] + r.n[1] * r.n[1] + r.n[2] * r.n[2]);
        r.light = light;
        if (!(r.area2 > 0.) || !std::isfinite(r.area2)) return;  // degenerate: dropped
        out.push_back(r);
    }
    void rect(const ObjectRec& o) {
        double P[4][3];  // P00, P10, P01, P11: the first in-plane axis varies first
        const double a[2] = {o.a0, o.a1}, b[2] = {o.b0, o.b1};
        for (int j = 0; j < 2; j++)
            for (int i = 0; i < 2; i++) {
                double* p = P[2 * j + i];
                if (o.axis == 2) { p[0] = a[i]; p[1] = b[j]; p[2] = o.k; }
                else if (o.axis == 1) { p[0] = a[i]; p[1] = o.k; p[2] = b[j]; }
                else { p[0] = o.k; p[1] = a[i]; p[2] = b[j]; }
            }
        tri(P[0], P[1], P[3]);
        tri(P[0], P[3], P[2]);
    }
    void lower(int id) {
        const ObjectRec& o = s.objects[id];
        switch (o.type) {
            case OBJ_RECT:
                rect(o);
                break;
            case OBJ_TRIANGLE: {
                const double* P = s.meshes[o.mesh]->pos.data();
                tri(P + 3 * o.ia, P + 3 * o.ib, P + 3 * o.ic);
                break;
            }
            case OBJ_MESH:  // the order of `indices`, not of the inner BVH
                for (int t = 0; t < o.tri_count; t++) lower(o.tri_first + t);
                break;
            case OBJ_TRANSFORM:
                xf.push_back(o.M);
                lower(o.children[0]);
                xf.pop_back();
                break;
            case OBJ_CUBE:
            case OBJ_LIST:
            case OBJ_BVH:
                for (int c : o.children) lower(c);
                break;
            default:
                throw RtError(RT_ERR_ARG, "an area light holds rectangles, cubes and triangles only");
        }
    }
};
// the table as the blob holds it (common/flat.h: AreaHdr, AreaLightDev[], AreaTriDev[]); `tris` = what rt_scene_area_light_tris reports
std::vector<char> lower_area_lights(const rt_scene& s, std::vector<rt_area_tri>& tris) {
    tris.clear();
    const size_t n_lights = s.area_lights.size();
    std::vector<AreaLightDev> lights(n_lights);
    for (size_t l = 0; l < n_lights; l++) {
        check_area_light(s, s.area_lights[l]);
        AreaLower lo{s, {}, tris, (int)l};
        lights[l].first = (uint32_t)tris.size();
        lo.lower(s.area_lights[l]);
        lights[l].count = (uint32_t)(tris.size() - lights[l].first);
        if (tris.size() > (size_t)AREA_MAX_TRIS)
            throw RtError(RT_ERR_UNSUPPORTED, "the area lights of a scene hold at most 1024 triangles (their pdf is a linear scan)");
        if (lights[l].count == 0u) throw RtError(RT_ERR_ARG, "area light " + std::to_string(l) + " has no triangle of non-zero area");
    }
    std::vector<AreaTriDev> dev(tris.size());
    for (size_t l = 0; l < n_lights; l++) {
        const uint32_t first = lights[l].first, end = first + lights[l].count;
        double amax = 0.;
        for (uint32_t k = first; k < end; k++) amax = std::fmax(amax, tris[k].area2);
        uint64_t cum = 0;
        for (uint32_t k = first; k < end; k++) {
            rt_area_tri& t = tris[k];
            const double f = std::floor(t.area2 / amax * 4294967295.0);
            t.q = f >= 1. ? (uint32_t)f : 1u;
            cum += t.q;
            AreaTriDev& d = dev[k];
            for (int i = 0; i < 3; i++) {
                d.a[i] = t.a[i]; d.e0[i] = t.e0[i]; d.e1[i] = t.e1[i]; d.n[i] = t.n[i];
            }
            d.area2 = t.area2;
            d.cum = cum;
            d.q = t.q;
            d.light = (uint32_t)l;
            d.pad = 0;
        }
        lights[l].total = cum;
    }
    AreaHdr hdr{};
    hdr.n_lights = (uint32_t)n_lights;
    hdr.n_tris = (uint32_t)tris.size();
    std::vector<char> tab(sizeof(hdr) + lights.size() * sizeof(AreaLightDev) + dev.size() * sizeof(AreaTriDev));
    std::memcpy(tab.data(), &hdr, sizeof(hdr));
    std::memcpy(tab.data() + sizeof(hdr), lights.data(), lights.size() * sizeof(AreaLightDev));
    if (!dev.empty()) std::memcpy(tab.data() + sizeof(hdr) + lights.size() * sizeof(AreaLightDev), dev.data(), dev.size() * sizeof(AreaTriDev));
    return tab;
}


std::vector<MatDev> material_table(const rt_scene& s) {
    std::vector<MatDev> mats;
    for (auto& m : s.materials) {
        MatDev md{m.type, m.tex, m.param, 0., 0., 0.};
        if (m.type == MAT_DIELECTRIC) {
            md.inv_ir = 1.0 / m.param;
            const double qf = (1. - md.inv_ir) / (1. + md.inv_ir), qb = (1. - m.param) / (1. + m.param);
            md.r0_front = qf * qf;
            md.r0_back = qb * qb;
        }
        mats.push_back(md);
    }
    return mats;
}

// -> the texture records; their texels (images) and tables (noise) are appended to `texels`
std::vector<TexDev> texture_table(const rt_scene& s, std::vector<uint8_t>& texels) {
    std::vector<TexDev> texs;
    for (auto& t : s.textures) {
        TexDev d{};
        d.type = t.type;
        d.t0 = t.t0, d.t1 = t.t1;
        d.w = t.w, d.h = t.h;
        if (t.type == TEX_NOISE) texels.resize((texels.size() + 7) & ~size_t(7));  // its f64 gradient vectors are read as doubles
        d.texel_off = (uint32_t)texels.size();
        for (int i = 0; i < 3; i++) d.color[i] = t.color[i];
        texels.insert(texels.end(), t.rgb.begin(), t.rgb.end());
        texs.push_back(d);
    }
    return texs;
}

// ---- kernel 5: compact object-space data (common/flat.h "Compact instance data") ----
struct CompactData {  // all empty: not available
    std::vector<NodeQ> n2q;
    std::vector<Tri32> tri32;
    std::vector<QGrid> qgrid;
};

// The 16-bit grid over the bounds of the BVH under `rn`, for ray origins bounded by `oo`, and its pad P in grid units; false: out of the
// range box32 is proven for
bool instance_grid(const Node2& rn, double oo, QGrid& g, double& P) {
    double mn[3], mx[3];
    const float* lo[3] = {rn.lo_x, rn.lo_y, rn.lo_z};
    const float* hi[3] = {rn.hi_x, rn.hi_y, rn.hi_z};
    for (int a = 0; a < 3; a++) {
        mn[a] = std::fmin((double)lo[a][0], (double)lo[a][1]);
        mx[a] = std::fmax((double)hi[a][0], (double)hi[a][1]);
    }
    // A flat instance (a single triangle, a planar mesh) has an extent of twice the pad along one axis: its grid scale would be
    // astronomical and the ray's grid coordinates (origin bound x scale) would leave the range box32 is proven for (2^35).  A
    // thin axis is therefore widened around its centre until  (origin bound) * QGRID_MAX / extent <= 2^33  -- the boxes of
    // that axis are then only rounded outward onto a coarser grid: still conservative.
    double mab = 0.;
    for (int a = 0; a < 3; a++) mab = std::fmax(mab, std::fmax(std::fabs(mn[a]), std::fabs(mx[a])));
    const double emin = QGRID_MAX * (oo + mab) / 8589934592.;
    for (int a = 0; a < 3; a++)
        if (mx[a] - mn[a] < emin) {
            const double c = 0.5 * (mn[a] + mx[a]);
            mn[a] = c - 0.5 * emin;
            mx[a] = c + 0.5 * emin;
        }
    // grid: g(x) = (x - mn) * k + shift, shift = P + 1, (mx - mn) * k = QGRID_MAX - 2 P - 2
    double k0 = 0., mabs = 0.;
    for (int a = 0; a < 3; a++) {
        const double ext = mx[a] - mn[a];
        k0 = std::fmax(k0, ext > 0. ? QGRID_MAX / ext : 1.);
        mabs = std::fmax(mabs, std::fabs(mn[a]));
    }
    const double og = (oo + mabs) * k0 + 65536.;  // bound of |o_g|
    if (!(og < 34359738368.)) return false;  // 2^35: box32 needs coordinates below 2^36
    P = std::ceil(std::ldexp(og, -22)) + 2.;
    if (!(P <= 4096.)) return false;
    for (int a = 0; a < 3; a++) {
        const double ext = mx[a] - mn[a];
        g.mn[a] = mn[a];
        g.k[a] = ext > 0. ? (QGRID_MAX - 2. * P - 2.) / ext : 1.;
    }
    g.shift = P + 1.;
    return true;
}

// both children's boxes on the grid, rounded outward and padded by P; false: a bound does not fit 16 bits
bool quantise_node(const Node2& nd, const QGrid& g, double P, NodeQ& q) {
    const float* l[3] = {nd.lo_x, nd.lo_y, nd.lo_z};
    const float* h[3] = {nd.hi_x, nd.hi_y, nd.hi_z};
    uint32_t ql[3], qh[3];
    for (int a = 0; a < 3; a++) {
        uint32_t w_lo = 0, w_hi = 0;
        for (int c = 0; c < 2; c++) {
            const double a_lo = std::floor(((double)l[a][c] - g.mn[a]) * g.k[a]) + 1.;           // g(lo) - P, rounded down
            const double a_hi = std::ceil(((double)h[a][c] - g.mn[a]) * g.k[a]) + 2. * P + 1.;   // g(hi) + P, rounded up
            if (!(a_lo >= 0. && a_hi <= QGRID_MAX && a_lo <= a_hi)) return false;
            w_lo |= (uint32_t)a_lo << (16 * c);
            w_hi |= (uint32_t)a_hi << (16 * c);
        }
        ql[a] = w_lo;
        qh[a] = w_hi;
    }
    q = NodeQ{ql[0], ql[1], ql[2], qh[0], qh[1], qh[2], {nd.child[0], nd.child[1]}};
    return true;
}

// Item j of a deferrable instance as a Tri32.  (The classification pass of build_scene_accel made the instance deferrable because every
// item of its context is a triangle with f32 vertices, and its BVH's leaves hold exactly those items: the two give-ups this function
// used to have on "not a triangle" and "not an f32" cannot be reached and are gone.)  false: the hoisted record does not hold the
// vertices' own values.
bool compact_triangle(const AccelBuild& ab, uint32_t j, const TriTables& t, Tri32& tr) {
    const uint32_t kp = ab.items[2 * j];
    const uint32_t tri = kp >> NK_BITS;
    const double* pre = &t.tripre[(size_t)tri * 10];
    double v[3][3];
    for (int c3 = 0; c3 < 3; c3++)
        for (int a = 0; a < 3; a++) v[c3][a] = t.vpos[3 * (size_t)t.tris[4 * (size_t)tri + c3] + a];
    for (int a = 0; a < 3; a++) {
        tr.pa[a] = (float)v[0][a];
        tr.pb[a] = (float)v[1][a];
        tr.pc[a] = (float)v[2][a];
        // the lane forms pb - pa, pc - pa in f64: must be the hoisted record's values, bit for bit
        if (v[0][a] != pre[a] || v[1][a] - v[0][a] != pre[3 + a] || v[2][a] - v[0][a] != pre[6 + a]) return false;
    }
    tr.order = ab.items[2 * j + 1];
    tr.kp = kp;
    // the largest edge component, rounded up to f32 (tri_miss32's error scale)
    double me = 0.;
    for (int a = 0; a < 3; a++) me = std::fmax(me, std::fmax(std::fabs(pre[3 + a]), std::fabs(pre[6 + a])));
    float mf = (float)me;
    if ((double)mf < me) mf = std::nextafterf(mf, INFINITY);
    tr.me = mf;
    return true;
}

// the grid, the NodeQ of every node and the Tri32 of every item of deferrable instance i; false: it has to give up
bool quantise_instance(const SceneAccel& acc, size_t i, const TriTables& t, CompactData& out) {
    const AccelBuild& ab = acc.ab;
    const uint32_t root = ab.inst[2 * i + 1];
    if ((root >> REF_TAG_SHIFT) != 0u) return false;
    QGrid g{};
    double P = 0.;
    if (!instance_grid(ab.nodes[root], acc.inst_oo[i], g, P)) return false;
    out.qgrid[i] = g;
    std::vector<uint32_t> st{root};
    while (!st.empty()) {
        const uint32_t n = st.back();
        st.pop_back();
        const Node2& nd = ab.nodes[n];
        if (!quantise_node(nd, g, P, out.n2q[n])) return false;
        for (int c = 0; c < 2; c++) {
            const uint32_t r = nd.child[c];
            if ((r >> REF_TAG_SHIFT) == 0u) {
                st.push_back(r);
            } else if ((r >> REF_TAG_SHIFT) == 1u) {
                const uint32_t first = r & REF_LEAF_FIRST_MASK, cnt = ((r >> REF_LEAF_COUNT_SHIFT) & 7u) + 1u;
                for (uint32_t j = first; j < first + cnt; j++)
                    if (!compact_triangle(ab, j, t, out.tri32[j])) return false;
            }
        }
    }
    return true;
}

CompactData compact_instance_data(const SceneAccel& acc, bool nested, const TriTables& t) {
    const AccelBuild& ab = acc.ab;
    bool any = false;
    for (char c : acc.compact_cand) any = any || c != 0;
    if (!ab.ok || ab.inst.empty() || nested || !any) return {};  // kernels 5 / 6 have no chain walk: nested scenes never reach them
    CompactData d;
    d.n2q.assign(ab.nodes.size(), NodeQ{});
    d.tri32.assign(ab.items.size() / 2, Tri32{});
    d.qgrid.assign(ab.inst.size() / 2, QGrid{});
    for (size_t i = 0; i < ab.inst.size() / 2; i++)
        if (acc.compact_cand[i] && !quantise_instance(acc, i, t, d)) return {};  // (an inline instance has no compact copy)
    return d;
}

// ---- the blob (layout: common/flat.h) ----
// The tie view: where the reference-order program lies in the blob, for the one walk that must read it from global memory whatever the
// kernel staged (tie_resolve, kernels.hip); word 6 is the record's own offset.
// The chain records follow its eight words (scenes of depth <= 1 have none: their blob is unchanged).  The kernels
// reach them as tie_view + 8 (chain_rec, kernels.hip): the tie view is always written and always read from global memory, so
// it doubles as the chain table's locator -- a change to its size must move chain_rec's offset with it.
std::vector<uint32_t> tie_view(const FlatView& v, const Builder& b, bool nested, size_t own_offset) {
    std::vector<uint32_t> tv = {v.off_meta, v.off_boxes, v.off_spheres, v.off_rects, v.off_tripre, v.off_xforms, (uint32_t)own_offset,
                                (uint32_t)(b.meta.size() / 2)};
    if (nested)
        for (const ChainRec& r : b.chains) {
            const uint32_t* w = (const uint32_t*)&r;
            tv.insert(tv.end(), w, w + CHAIN_WORDS);
        }
    return tv;
}

BgDev background_record(const rt_scene& s) {
    BgDev bg{};
    bg.kind = s.background.kind;
    bg.tex = s.background.kind == 3 ? s.background.texture : 0;
    for (int c = 0; c < 3; c++) {
        bg.c0[c] = s.background.color0[c];
        bg.c1[c] = s.background.color1[c];
    }
    bg.scale = s.background.scale;
    return bg;
}

EnvDev env_record(const rt_scene& s) {
    if (s.background.kind == 0) throw RtError(RT_ERR_ARG, "env sampling needs a background (rt_scene_set_background) to sample");
    EnvDev e{};
    e.enabled = 1;
    e.w = s.env_sampling.width;
    e.h = s.env_sampling.height;
    if (e.w == 0) {  // automatic: an image map gets one cell per texel, halved per axis down to 4096 x 2048; anything else 256 x 128
        e.w = 256;
        e.h = 128;
        if (s.background.kind == 3 && s.textures[s.background.texture].type == TEX_IMAGE) {
            e.w = s.textures[s.background.texture].w;
            e.h = s.textures[s.background.texture].h;
            while (e.w > 4096 || e.h > 2048) {
                e.w = std::max(1, e.w / 2);
                e.h = std::max(1, e.h / 2);
            }
        }
    }
    return e;
}

// The one place that knows the order of the sections: the order of the append calls and of the 16-byte alignments IS the layout.
FlatScene write_blob(const rt_scene& s, const Builder& b, const std::vector<uint32_t>& lights, const std::vector<MatDev>& mats,
                     const std::vector<TexDev>& texs, const std::vector<uint8_t>& texels, const SceneAccel& acc, const CompactData& cd) {
    const AccelBuild& ab = acc.ab;
    const bool nested = b.xf_nest >= 2;
    FlatScene f;
    FlatView v{};
    auto align16 = [&] { f.blob.resize((f.blob.size() + 15) & ~size_t(15)); };
    // hot part (read once per visited node): candidates for LDS residency
    v.off_meta = append(f.blob, b.meta);
    v.off_boxes = append(f.blob, b.boxes);
    v.off_spheres = append(f.blob, b.spheres);
    v.stage2_begin = v.off_spheres;
    v.off_rects = append(f.blob, b.rects);
    v.off_tris = append(f.blob, b.tris);
    v.off_tripre = append(f.blob, b.tripre);
    v.off_xforms = append(f.blob, b.xforms);
    align16();
    v.stage_bytes = (uint32_t)f.blob.size();
    // kernel 2 stages [spheres .. xforms | items2 | inst2 | tripre2 | n2] into LDS when it fits
    v.off_items2 = append(f.blob, ab.items);
    v.off_inst2 = append(f.blob, ab.inst);
    v.off_tripre2 = append(f.blob, acc.tripre2);  // triangle records in item order (big meshes); staged with the rest when everything fits
    v.off_n2 = append(f.blob, ab.nodes);
    align16();
    v.stage2_end = (uint32_t)f.blob.size();
    v.off_n2q = append(f.blob, cd.n2q);  // kernel 5's compact object-space data: never staged as a whole
    v.off_tri32 = append(f.blob, cd.tri32);
    v.off_qgrid = append(f.blob, cd.qgrid);
    v.n_nodes2 = (uint32_t)ab.nodes.size();
    v.accel_ok = ab.ok ? 1u : 0u;
    v.root2 = acc.root2;
    v.stack2 = (uint32_t)(ab.max_depth + 2);
    v.n_inst2 = (uint32_t)(ab.inst.size() / 2);
    v.max_inst_nodes2 = acc.max_inst_nodes;
    v.inst_depth2 = acc.inst_depth;
    v.n_world_items2 = acc.n_world_items;
    v.stack2_inline = acc.stack_inline;
    for (char c : acc.compact_cand) v.n_inline2 += c ? 0u : 1u;
    v.coop_data_ok = cd.qgrid.empty() ? 0u : 1u;
    v.world_top2 = acc.world_top;
    v.world_depth2 = acc.world_depth;
    v.origin_limit2 = acc.origin_limit;
    // cold part (read once per path segment, by the winning leaf only): always global
    v.off_sphere_mat = append(f.blob, b.sphere_mat);
    v.off_rect_mat = append(f.blob, b.rect_mat);
    v.off_mats = append(f.blob, mats);
    v.off_texs = append(f.blob, texs);
    v.off_media = append(f.blob, b.media);
    v.n_media = (uint32_t)b.media.size();
    for (auto& tx : s.textures) v.has_noise |= (tx.type == TEX_NOISE) ? 1u : 0u;
    v.off_msph = append(f.blob, b.msph);
    v.n_msph = (uint32_t)(b.msph.size() / 10);
    for (size_t i = 0; i + 10 <= b.msph.size(); i += 10) {
        f.msph_t0_max = std::max(f.msph_t0_max, b.msph[i + 6]);
        f.msph_t1_min = std::min(f.msph_t1_min, b.msph[i + 7]);
    }
    align16();
    v.off_tie_view = append(f.blob, tie_view(v, b, nested, f.blob.size()));
    v.off_lights = append(f.blob, lights);
    v.n_lights = (uint32_t)(lights.size() / 2);
    // a scene without area lights / a background / env sampling keeps its blob, and its fingerprint, byte for byte: offset 0 = none
    if (!s.area_lights.empty()) v.off_area = append(f.blob, lower_area_lights(s, f.area_tris));
    v.off_vpos = append(f.blob, b.vpos);  // kept for introspection; the kernels read tripre instead
    v.off_vnrm = append(f.blob, b.vnrm);
    v.off_texels = append(f.blob, texels);
    if (s.background.kind != 0) v.off_bg = append(f.blob, std::vector<BgDev>{background_record(s)});
    if (s.env_sampling.enabled != 0) v.off_env = append(f.blob, std::vector<EnvDev>{env_record(s)});
    align16();
    v.total_bytes = (uint32_t)f.blob.size();
    v.n_nodes = (uint32_t)(b.meta.size() / 2);
    v.kinds_mask = b.kinds;
    f.view = v;
    f.xf_nest = nested ? b.xf_nest : 0u;
    for (int lid : s.lights) f.light_in_medium = f.light_in_medium || b.in_medium.count(lid) != 0;
    return f;
}

void fill_info(FlatScene& f, const Builder& b, size_t n_materials, size_t n_textures, const AccelBuild& ab) {
    rt_scene_info& in = f.info;
    in.n_nodes = (int32_t)f.view.n_nodes;
    in.n_boxes = (int32_t)(b.boxes.size() / 6);
    in.n_spheres = (int32_t)b.sphere_mat.size();
    in.n_rects = (int32_t)b.rect_mat.size() - b.n_cubes;
    in.n_cubes = b.n_cubes;
    in.n_tris = (int32_t)(b.tris.size() / 4);
    in.n_xforms = (int32_t)(b.xforms.size() / 32);
    in.n_materials = (int32_t)n_materials;
    in.n_textures = (int32_t)n_textures;
    in.n_verts = (int32_t)(uint32_t)(b.vpos.size() / 3);
    in.max_depth = b.max_depth;
    in.committed = 1;
    in.bytes = f.blob.size();
    in.accel_ok = ab.ok ? 1 : 0;
    in.accel_nodes = (int32_t)ab.nodes.size();
    in.accel_items = (int32_t)(ab.items.size() / 2);
    in.accel_instances = (int32_t)(ab.inst.size() / 2);
    in.accel_stack = (int32_t)f.view.stack2;
    in.accel_compact = (int32_t)f.view.coop_data_ok;
}

}  // namespace

void flatten(rt_scene& s) {
    if (s.root < 0) throw RtError(RT_ERR_ARG, "scene has no root (rt_world_new / rt_scene_set_root)");
    Builder b(s);
    b.emit_program();
    const std::vector<uint32_t> lights = b.light_table();
    const std::vector<MatDev> mats = material_table(s);
    std::vector<uint8_t> texels;
    const std::vector<TexDev> texs = texture_table(s, texels);
    const bool nested = b.xf_nest >= 2;
    const TriTables tri{b.tris, b.vpos, b.tripre};
    const SceneAccel acc = build_scene_accel(b.actx, b.accel_ok, nested, b.media_extent, tri);
    const CompactData compact = compact_instance_data(acc, nested, tri);
    FlatScene f = write_blob(s, b, lights, mats, texs, texels, acc, compact);
    fill_info(f, b, mats.size(), texs.size(), acc.ab);
    s.flat = std::move(f);  // (a commit that throws has left the scene as it was)
    s.committed = true;
}

}  // namespace rtamd
