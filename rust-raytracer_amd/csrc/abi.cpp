// extern "C" entry points of librtamd.so (declared in include/rtamd.h).
// Every function converts C++ exceptions into rt_status codes; nothing unwinds
// across the boundary.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "common/grid_shape.h"
#include "common/rng.h"
#include "common/schedule.h"
#include "device/adaptive.h"
#include "device/ao.h"
#include "device/denoise.h"
#include "device/device.h"
#include "device/temporal.h"
#include "host/frame.h"
#include "host/scene.h"
#include "rtamd.h"

using namespace rtamd;

static thread_local std::string g_err;
static Tuning g_tuning;
static std::mutex g_tuning_mu;
namespace rtamd {
// a consistent snapshot: callers take ONE copy per API call (render_tiles, render_sppm, accel_build_bvh, make_plan) and pass
// it down, so a concurrent rt_tuning_set can never make one render see two different settings
Tuning tuning() {
    std::lock_guard<std::mutex> g(g_tuning_mu);
    return g_tuning;
}
}  // namespace rtamd

rt_scene::~rt_scene() { free_device_copies(*this); }

template <class F>
static int guard(F&& f) {
    try {
        return f();
    } catch (const RtError& e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "out of memory";
        return RT_ERR_ARG;
    } catch (const std::exception& e) {
        g_err = e.what();
        return RT_ERR_ARG;
    } catch (...) {
        g_err = "unknown error";
        return RT_ERR_ARG;
    }
}

static void not_committed_only(const rt_scene* s) {
    REQUIRE(s, "null scene");
    if (s->committed) throw RtError(RT_ERR_ARG, "scene is immutable after rt_scene_commit");
}

// The device half of the env sampling diagnostics (device/kernels.hip).  Referenced weakly: a build of the host half alone, linked
// against a stand-in for the device layer that predates them, still links, and the diagnostics then report that there is no device.
namespace rtamd {
void debug_env_table_device(const rt_scene& s, int* w, int* h, uint32_t* q_host) __attribute__((weak));
void debug_env_eval_device(const rt_scene& s, int mode, size_t n, const double* in, double* out) __attribute__((weak));
}  // namespace rtamd
namespace rtamd {
void debug_area_eval_device(const rt_scene& s, int mode, size_t n, const double* in, double* out) __attribute__((weak));  // (likewise)
void debug_shade_device(const rt_scene& s, size_t n, const double* in, const uint64_t* keys, double* out) __attribute__((weak));
void debug_light_eval_device(const rt_scene& s, int mode, size_t n, const double* in, const uint64_t* keys, double* out) __attribute__((weak));
bool debug_sppm_gather_device(rt_debug_sppm_gather& io) __attribute__((weak));
bool debug_sppm_trace_device(const rt_scene& s, const CameraDev& cam, rt_debug_sppm_trace& io) __attribute__((weak));
bool debug_walk_device(const rt_scene& s, int kernel, size_t n, const double* rays, const uint64_t* keys, double t_min, double* out) __attribute__((weak));
}  // namespace rtamd
static bool env_debug_linked() { return &rtamd::debug_env_table_device != nullptr && &rtamd::debug_env_eval_device != nullptr; }

extern "C" {

int rt_abi_version(void) { return RTAMD_ABI_VERSION; }
const char* rt_last_error(void) { return g_err.c_str(); }

void rt_default_params(rt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->width = 800;      // main.rs:34
    p->height = 800;     // main.rs:45 (aspect 1)
    p->spp = 256;        // camera.rs:73
    p->max_depth = 50;   // photon_mapper.rs:334
    p->t_min = 0.001;    // photon_mapper.rs:335
    p->seed = 1;
    p->rank = 0;
    p->world = 1;
    p->spp_chunk = 0;
    p->kernel = 0;
    p->device = -1;
    p->integrator = 0;
    p->time0 = 0.;  // (book-2 extension: shutter closed = no time draw)
    p->time1 = 0.;
}
int rt_device_count(void) { return device_count(); }

int64_t rt_release_workspaces(void) {
    int64_t n = 0;
    guard([&] {
        int cur = -1;
        try {
            cur = dev_get_device();
        } catch (...) {
        }
        n = (int64_t)release_workspaces();
        n += (int64_t)frame_pool_release();
        if (cur >= 0) dev_set_device(cur);
        exchange_release_idle();
        return (int)RT_OK;
    });
    return n;
}
void rt_tuning_default(rt_tuning* t) {
    if (!t) return;
    std::memset(t, 0, sizeof(*t));
    t->top_nodes = -1;
    t->sppm_knn_candidates = -1;
}
int rt_tuning_set(const rt_tuning* t) {
    return guard([&] {
        REQUIRE(t, "null argument");
        REQUIRE(t->max_leaf >= 0 && t->max_leaf <= 4, "max_leaf must be 0 (auto) or 1..4");
        REQUIRE(t->sah_box_cost >= 0. && t->sah_box_cost < 1e6, "sah_box_cost out of range");
        Tuning n;
        n.no_lds = t->no_lds != 0;
        n.n_top = t->top_nodes < 0 ? -1 : t->top_nodes;
        n.sub_spp = std::max(0, t->sub_spp);
        n.max_leaf = t->max_leaf;
        n.coop_pool = std::max(0, t->coop_pool);
        n.sppm_cap = std::max(0, t->sppm_photon_capacity);
        n.knn_cand = t->sppm_knn_candidates < 0 ? -1 : t->sppm_knn_candidates;
        n.multi_force_rccl = t->multi_force_rccl != 0;
        n.wf_workspace_mb = std::max(0, t->wf_workspace_mb);
        n.c_box = t->sah_box_cost;
        {
            std::lock_guard<std::mutex> g(g_tuning_mu);
            g_tuning = n;
        }
        return (int)RT_OK;
    });
}

int rt_scene_create(rt_scene** out) {
    return guard([&] {
        REQUIRE(out, "null out pointer");
        *out = new rt_scene();
        return (int)RT_OK;
    });
}
void rt_scene_destroy(rt_scene* s) { delete s; }

int rt_texture_constant(rt_scene* s, const double color[3]) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(color, "null color");
        return add_texture_constant(*s, color);
    });
}
int rt_texture_checker(rt_scene* s, int t0, int t1) {
    return guard([&] {
        not_committed_only(s);
        return add_texture_checker(*s, t0, t1);
    });
}
int rt_texture_image(rt_scene* s, int width, int height, const uint8_t* rgb) {
    return guard([&] {
        not_committed_only(s);
        return add_texture_image(*s, width, height, rgb);
    });
}
int rt_texture_noise(rt_scene* s, double scale, uint64_t seed) {
    return guard([&] {
        not_committed_only(s);
        return add_texture_noise(*s, scale, seed);
    });
}
int rt_material_lambertian(rt_scene* s, int tex) {
    return guard([&] {
        not_committed_only(s);
        return add_material(*s, MAT_LAMBERTIAN, tex, 0.);
    });
}
int rt_material_metal(rt_scene* s, int tex, double fuzz) {
    return guard([&] {
        not_committed_only(s);
        return add_material(*s, MAT_METAL, tex, fuzz);
    });
}
int rt_material_dielectric(rt_scene* s, double ir, int tex) {
    return guard([&] {
        not_committed_only(s);
        return add_material(*s, MAT_DIELECTRIC, tex, ir);
    });
}
int rt_material_isotropic(rt_scene* s, int tex) {
    return guard([&] {
        not_committed_only(s);
        return add_material(*s, MAT_ISOTROPIC, tex, 0.);
    });
}
int rt_object_constant_medium(rt_scene* s, double density, int boundary, int phase_material) {
    return guard([&] {
        not_committed_only(s);
        return add_medium(*s, density, boundary, phase_material);
    });
}
int rt_material_diffuse_light(rt_scene* s, int tex) {
    return guard([&] {
        not_committed_only(s);
        return add_material(*s, MAT_DIFFUSE_LIGHT, tex, 0.);
    });
}

int rt_object_sphere(rt_scene* s, const double center[3], double radius, int material) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(center, "null center");
        return add_sphere(*s, center, radius, material);
    });
}
int rt_object_moving_sphere(rt_scene* s, const double center0[3], const double center1[3], double time0, double time1, double radius, int material) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(center0 && center1, "null center");
        return add_moving_sphere(*s, center0, center1, time0, time1, radius, material);
    });
}
int rt_object_rect_xy(rt_scene* s, double x0, double y0, double x1, double y1, double z, int material) {
    return guard([&] {
        not_committed_only(s);
        return add_rect(*s, 2, x0, y0, x1, y1, z, material);
    });
}
int rt_object_rect_xz(rt_scene* s, double x0, double z0, double x1, double z1, double y, int material) {
    return guard([&] {
        not_committed_only(s);
        return add_rect(*s, 1, x0, z0, x1, z1, y, material);
    });
}
int rt_object_rect_yz(rt_scene* s, double y0, double z0, double y1, double z1, double x, int material) {
    return guard([&] {
        not_committed_only(s);
        return add_rect(*s, 0, y0, z0, y1, z1, x, material);
    });
}
int rt_object_cube(rt_scene* s, const double box_min[3], const double box_max[3], int material) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(box_min && box_max, "null box");
        return add_cube(*s, box_min, box_max, material);
    });
}
static int mark_light(rt_scene* s, int obj, const double flux[3], double scale) {
    ObjectRec& o = s->objects[obj];
    for (int i = 0; i < 3; i++) o.light_flux[i] = flux[i];
    o.light_scale = scale;
    return obj;
}
int rt_object_sphere_light(rt_scene* s, const double center[3], double radius, const double flux[3], double scale) {
    return guard([&] {  // SphereDiffuseLight::new, light.rs:74-86
        not_committed_only(s);
        REQUIRE(center && flux, "null argument");
        int m = add_material(*s, MAT_DIFFUSE_LIGHT, add_texture_constant(*s, flux), 0.);
        return mark_light(s, add_sphere(*s, center, radius, m), flux, scale);
    });
}
int rt_object_xz_rect_light(rt_scene* s, double x0, double z0, double x1, double z1, double y, const double flux[3], double scale) {
    return guard([&] {  // XZRectLight::new, light.rs:134-146 (scale only feeds the photon power)
        not_committed_only(s);
        REQUIRE(flux, "null flux");
        int m = add_material(*s, MAT_DIFFUSE_LIGHT, add_texture_constant(*s, flux), 0.);
        return mark_light(s, add_rect(*s, 1, x0, z0, x1, z1, y, m), flux, scale);
    });
}
int rt_object_mesh(rt_scene* s, int n_vert, const double* positions, const double* normals, int n_tri, const uint32_t* indices,
                   int material, int synthesize_normals_flag, uint64_t bvh_seed) {
    return guard([&] {
        not_committed_only(s);
        return add_mesh(*s, n_vert, positions, normals, n_tri, indices, material, synthesize_normals_flag != 0, bvh_seed);
    });
}
int rt_object_mesh_obj(rt_scene* s, const char* obj_path, int material, int synthesize_normals_flag, uint64_t bvh_seed) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(obj_path, "null path");
        ObjMesh m = load_obj_file(obj_path);
        return add_mesh(*s, (int)(m.pos.size() / 3), m.pos.data(), m.has_normals ? m.nrm.data() : nullptr, (int)(m.idx.size() / 3),
                        m.idx.data(), material, synthesize_normals_flag != 0, bvh_seed);
    });
}
int rt_object_transform(rt_scene* s, const double rotate_deg[3], const double scale[3], const double translate[3], int object) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(rotate_deg && scale && translate, "null argument");
        return add_transform(*s, rotate_deg, scale, translate, object);
    });
}
int rt_object_transform_matrix(rt_scene* s, const double trans[16], const double* inverse_trans, int object) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(trans, "null matrix");
        return add_transform_matrix(*s, trans, inverse_trans, object);
    });
}
int rt_mesh_data(rt_scene* s, int n_vert, const double* positions, const double* normals) {
    return guard([&] {
        not_committed_only(s);
        return add_mesh_data(*s, n_vert, positions, normals);
    });
}
int rt_object_triangle(rt_scene* s, int mesh, uint32_t a, uint32_t b, uint32_t c, int material) {
    return guard([&] {
        not_committed_only(s);
        return add_triangle(*s, mesh, a, b, c, material);
    });
}
int rt_object_list(rt_scene* s, int n, const int* objects) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(n >= 0 && (n == 0 || objects), "bad list");
        return add_list(*s, n, objects);
    });
}
int rt_object_bvh_node(rt_scene* s, int left, int right) {
    return guard([&] {
        not_committed_only(s);
        check_obj(*s, left);
        check_obj(*s, right);
        return add_bvh_node(*s, left, right);
    });
}
int rt_object_bvh_build(rt_scene* s, int n, const int* objects, uint64_t bvh_seed) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(n > 0 && objects, "BVHNode::new needs a non-empty list");
        return add_bvh_build(*s, std::vector<int>(objects, objects + n), bvh_seed);
    });
}
int rt_object_bounding_box(const rt_scene* s, int object, double out_min_max[6]) {
    return guard([&] {
        REQUIRE(s && out_min_max, "null argument");
        Box b;
        if (!bounding_box(*s, object, b)) throw RtError(RT_ERR_NO_BBOX, "object has no bounding box");
        for (int i = 0; i < 3; i++) {
            out_min_max[i] = b.mn[i];
            out_min_max[3 + i] = b.mx[i];
        }
        return (int)RT_OK;
    });
}
int rt_scene_root(const rt_scene* s) {
    return guard([&] {
        REQUIRE(s, "null scene");
        REQUIRE(s->root >= 0, "scene has no root");
        return s->root;
    });
}
int rt_object_describe(const rt_scene* s, int object, rt_object_desc* out) {
    return guard([&] {
        REQUIRE(s && out, "null argument");
        check_obj(*s, object);
        const ObjectRec& o = s->objects[object];
        static_assert((int)OBJ_SPHERE == RT_OBJ_SPHERE && (int)OBJ_RECT == RT_OBJ_RECT && (int)OBJ_CUBE == RT_OBJ_CUBE &&
                      (int)OBJ_TRIANGLE == RT_OBJ_TRIANGLE && (int)OBJ_MESH == RT_OBJ_MESH && (int)OBJ_TRANSFORM == RT_OBJ_TRANSFORM &&
                      (int)OBJ_LIST == RT_OBJ_LIST && (int)OBJ_BVH == RT_OBJ_BVH && (int)OBJ_MEDIUM == RT_OBJ_MEDIUM &&
                      (int)OBJ_MOVING_SPHERE == RT_OBJ_MOVING_SPHERE, "rt_object_type mirrors ObjType");
        std::memset(out, 0, sizeof(*out));
        out->type = o.type;
        out->material = (o.type == OBJ_SPHERE || o.type == OBJ_RECT || o.type == OBJ_TRIANGLE || o.type == OBJ_MOVING_SPHERE) ? o.material : -1;
        out->n_children = (int32_t)o.children.size();
        if (o.type == OBJ_SPHERE) {
            out->v[0] = o.c[0]; out->v[1] = o.c[1]; out->v[2] = o.c[2]; out->v[3] = o.r;
        } else if (o.type == OBJ_MOVING_SPHERE) {
            out->v[0] = o.c[0]; out->v[1] = o.c[1]; out->v[2] = o.c[2]; out->v[3] = o.r;
            out->v[4] = o.c1[0]; out->v[5] = o.c1[1]; out->v[6] = o.c1[2];
        } else if (o.type == OBJ_RECT) {
            out->axis = o.axis;
            out->v[0] = o.a0; out->v[1] = o.b0; out->v[2] = o.a1; out->v[3] = o.b1; out->v[4] = o.k;
        } else if (o.type == OBJ_TRIANGLE) {
            out->v[0] = (double)o.ia; out->v[1] = (double)o.ib; out->v[2] = (double)o.ic;
        } else if (o.type == OBJ_MEDIUM) {
            out->material = o.material;
            out->v[0] = o.density;
        }
        return (int)RT_OK;
    });
}
int rt_object_children(const rt_scene* s, int object, int capacity, int* out) {
    return guard([&] {
        REQUIRE(s && (out || capacity <= 0), "null argument");
        check_obj(*s, object);
        const ObjectRec& o = s->objects[object];
        for (int i = 0; i < capacity && i < (int)o.children.size(); i++) out[i] = o.children[i];
        return (int)o.children.size();
    });
}
int rt_world_new(rt_scene* s, int n, const int* objects, uint64_t bvh_seed) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(n > 0 && objects, "World::new needs a non-empty list");
        s->root = add_bvh_build(*s, std::vector<int>(objects, objects + n), bvh_seed);
        return s->root;
    });
}
int rt_scene_set_lights(rt_scene* s, int n, const int* objects) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(n >= 0 && (n == 0 || objects), "bad light list");
        std::vector<int> v;
        for (int i = 0; i < n; i++) {
            check_obj(*s, objects[i]);
            const ObjectRec& o = s->objects[objects[i]];
            if (!(o.type == OBJ_SPHERE || (o.type == OBJ_RECT && o.axis == 1)))
                throw RtError(RT_ERR_ARG, "a light must be a sphere or an XZ rectangle (light.rs:67-86,127-146)");
            v.push_back(objects[i]);
        }
        s->lights = v;
        return (int)RT_OK;
    });
}
int rt_scene_set_area_lights(rt_scene* s, int n, const int* objects) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(n >= 0 && (n == 0 || objects), "bad area light list");
        for (int i = 0; i < n; i++) check_area_light(*s, objects[i]);
        s->area_lights.assign(objects, objects + n);
        return (int)RT_OK;
    });
}
int rt_scene_area_light_tris(const rt_scene* s, int capacity, rt_area_tri* out) {
    return guard([&] {
        REQUIRE(s && (out || capacity <= 0), "null argument");
        require_committed(*s);
        const std::vector<rt_area_tri>& t = s->flat.area_tris;
        for (int i = 0; i < capacity && i < (int)t.size(); i++) out[i] = t[i];
        return (int)t.size();
    });
}
int rt_scene_set_background(rt_scene* s, const rt_background* bg) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(bg, "null background");
        REQUIRE(bg->kind >= 0 && bg->kind <= 3, "background kind must be 0 (none), 1 (constant), 2 (vertical gradient) or 3 (texture)");
        bool ok = std::isfinite(bg->scale) && bg->scale >= 0.;
        for (int c = 0; c < 3; c++) ok = ok && std::isfinite(bg->color0[c]) && bg->color0[c] >= 0. && std::isfinite(bg->color1[c]) && bg->color1[c] >= 0.;
        REQUIRE(ok, "background colours and scale must be finite and >= 0");
        if (bg->kind == 3)
            REQUIRE(bg->texture >= 0 && bg->texture < (int)s->textures.size(), "background kind 3 needs a texture id of this scene");
        s->background = *bg;
        return (int)RT_OK;
    });
}
int rt_scene_get_background(const rt_scene* s, rt_background* out) {
    return guard([&] {
        REQUIRE(s && out, "null argument");
        *out = s->background;
        return (int)RT_OK;
    });
}
int rt_scene_set_env_sampling(rt_scene* s, const rt_env_sampling* cfg) {
    return guard([&] {
        not_committed_only(s);
        REQUIRE(cfg, "null env sampling config");
        REQUIRE(cfg->enabled == 0 || cfg->enabled == 1, "env sampling: enabled must be 0 or 1");
        REQUIRE(cfg->width >= 0 && cfg->height >= 0, "env sampling: the table size must not be negative");
        REQUIRE((cfg->width == 0) == (cfg->height == 0), "env sampling: width and height are both 0 (automatic) or both set");
        REQUIRE(cfg->width <= ENV_MAX_DIM && cfg->height <= ENV_MAX_DIM, "env sampling: the table is at most 8192 x 8192");
        s->env_sampling = *cfg;
        return (int)RT_OK;
    });
}
int rt_scene_get_env_sampling(const rt_scene* s, rt_env_sampling* out) {
    return guard([&] {
        REQUIRE(s && out, "null argument");
        *out = s->env_sampling;
        return (int)RT_OK;
    });
}
int rt_scene_set_root(rt_scene* s, int object) {
    return guard([&] {
        not_committed_only(s);
        check_obj(*s, object);
        s->root = object;
        return (int)RT_OK;
    });
}
int rt_scene_cornell_box(rt_scene* s, const char* cube_obj_path, double aspect_ratio, uint64_t bvh_seed, rt_camera* cam_out) {
    return guard([&] {  // scene.rs:16-112, numbers verbatim
        not_committed_only(s);
        REQUIRE(cube_obj_path, "null path");
        auto ctex = [&](double r, double g, double b) {
            const double c[3] = {r, g, b};
            return add_texture_constant(*s, c);
        };
        int red = add_material(*s, MAT_LAMBERTIAN, ctex(0.75, 0.25, 0.25), 0.);
        int white = add_material(*s, MAT_LAMBERTIAN, ctex(0.75, 0.75, 0.75), 0.);
        int blue = add_material(*s, MAT_LAMBERTIAN, ctex(0.25, 0.25, 0.75), 0.);
        int light = add_material(*s, MAT_DIFFUSE_LIGHT, ctex(1., 1., 1.), 0.);  // XZRectLight::new(.., flux (1,1,1), 1e6)
        std::vector<int> items;
        items.push_back(add_rect(*s, 0, 0.0, 0.0, 555.0, 555.0, 555., red));
        items.push_back(add_rect(*s, 0, 0., 0., 555., 555., 0., blue));
        items.push_back(add_rect(*s, 1, 0., 0., 555., 555., 0., white));
        items.push_back(add_rect(*s, 1, 0., 0., 555., 555., 555., white));
        items.push_back(add_rect(*s, 2, 0., 0., 555., 555., 555., white));
        const double c1[3] = {140., 100., 240.}, c2[3] = {400., 100., 360.};
        items.push_back(add_sphere(*s, c1, 100., add_material(*s, MAT_DIELECTRIC, ctex(0.999, 0.999, 0.999), 1.5)));
        items.push_back(add_sphere(*s, c2, 100., add_material(*s, MAT_METAL, ctex(0.999, 0.999, 0.999), 0.)));
        const int light_obj = add_rect(*s, 1, 213., 227., 343., 332., 554., light);
        const double one[3] = {1., 1., 1.};
        mark_light(s, light_obj, one, 1000000.);  // XZRectLight::new((213,227),(343,332),554, flux (1,1,1), scale 1e6), scene.rs:26-32
        items.push_back(light_obj);
        s->lights = {light_obj};  // scene.rs:110 vec![Arc::new(light)]
        ObjMesh m = load_obj_file(cube_obj_path);
        if (!m.has_normals) throw RtError(RT_ERR_NO_NORMALS, "cube.obj without normals");
        int mesh = add_mesh(*s, (int)(m.pos.size() / 3), m.pos.data(), m.nrm.data(), (int)(m.idx.size() / 3), m.idx.data(), white, false,
                            bvh_seed);
        const double rot[3] = {0., 0., 0.}, sc[3] = {1. * 50., 1. * 50., 1. * 50.}, tr[3] = {100., 50., 100.};
        items.push_back(add_transform(*s, rot, sc, tr, mesh));
        const double bmin[3] = {300., 0., 100.}, bmax[3] = {380., 100., 180.};
        items.push_back(add_cube(*s, bmin, bmax, white));
        s->root = add_bvh_build(*s, items, bvh_seed);
        if (cam_out) {
            rt_camera c = {{278., 278., -800.}, {278., 278., 278.}, {0., 1., 0.}, 50., aspect_ratio, 0.0, 10.0};
            *cam_out = c;
        }
        return (int)RT_OK;
    });
}
int rt_scene_load_file(const char* path, rt_scene** out, rt_camera* cam_out) {
    return guard([&] {
        REQUIRE(path && out, "null argument");
        *out = load_scene_file(path, cam_out);
        return (int)RT_OK;
    });
}
int rt_scene_parse_file(const char* path, rt_scene** out, rt_camera* cam_out) {
    return guard([&] {
        REQUIRE(path && out, "null argument");
        *out = load_scene_file(path, cam_out, false);
        return (int)RT_OK;
    });
}
int rt_scene_commit(rt_scene* s) {
    return guard([&] {
        REQUIRE(s, "null scene");
        if (s->committed) return (int)RT_OK;
        flatten(*s);
        return (int)RT_OK;
    });
}
uint64_t rt_scene_fingerprint(const rt_scene* s) {
    if (!s || !s->committed) return 0;
    uint64_t h = 1469598103934665603ull;  // FNV-1a, 64 bit
    for (unsigned char c : s->flat.blob) {
        h ^= (uint64_t)c;
        h *= 1099511628211ull;
    }
    return h ? h : 1;
}
// bumped whenever an image's bits may change for unchanged inputs (round 5: near ties go to the reference-order walk; rng-3 since round 4)
const char* rt_spec_version(void) { return "rtamd-image-5 rng-3 ln-1 sin-1"; }
int rt_scene_info_get(const rt_scene* s, rt_scene_info* out) {
    return guard([&] {
        REQUIRE(s && out, "null argument");
        *out = s->flat.info;
        out->committed = s->committed ? 1 : 0;
        return (int)RT_OK;
    });
}

// ---- render (the frame driver: host/frame.h) --------------------------------
int64_t rt_tiles_total(const rt_params* p) {
    if (!p || p->width <= 0 || p->height <= 0) return RT_ERR_ARG;
    return tiles_total(p->width, p->height);
}
int64_t rt_tiles_owned(const rt_params* p) {
    if (!p || p->width <= 0 || p->height <= 0 || p->world < 1 || p->rank < 0 || p->rank >= p->world) return RT_ERR_ARG;
    return tiles_owned(tiles_total(p->width, p->height), p->rank, p->world);
}

int rt_render_tiles_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, double* d_tiles, void* hip_stream,
                           rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && d_tiles, "null argument");
        require_committed(*s);
        require_device();
        const CallClock clock;
        const RenderPlan pl = make_plan(p);
        DeviceScope dev_scope(p->device);  // (d_tiles and hip_stream must belong to it; the caller's current device is restored)
        const CameraDev cd = make_camera(*cam);
        if (stats) std::memset(stats, 0, sizeof(*stats));
        render_tiles(*s, cd, pl, d_tiles, hip_stream, stats);
        clock.stamp(stats, pixels_in_image(pl) * (uint64_t)pl.spp);
        return (int)RT_OK;
    });
}

int rt_render_accumulate_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, int32_t sample_begin, int32_t sample_end,
                                double* d_accum, void* hip_stream, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && d_accum, "null argument");
        accumulate_device(*s, *cam, *p, sample_begin, sample_end, d_accum, hip_stream, stats);
        return (int)RT_OK;
    });
}
int rt_accum_finalize_device(const rt_params* p, const double* d_accum, double* d_tiles, void* hip_stream) {
    return guard([&] {
        REQUIRE(p && d_accum && d_tiles, "null argument");
        require_device();
        const RenderPlan pl = make_plan(p);
        DeviceScope dev_scope(p->device);
        finalize_tiles(pl, d_accum, d_tiles, hip_stream);
        return (int)RT_OK;
    });
}

int64_t rt_accum_state_doubles(const rt_params* p) {
    const int64_t n = rt_tiles_owned(p);
    return n < 0 ? n : (int64_t)row_doubles(n);
}
int rt_render_accumulate(const rt_scene* s, const rt_camera* cam, const rt_params* p, int32_t sample_begin, int32_t sample_end,
                         double* accum_state, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && accum_state, "null argument");
        accumulate_host(*s, *cam, *p, sample_begin, sample_end, accum_state, stats);
        return (int)RT_OK;
    });
}
int rt_accum_finalize(const rt_params* p, const double* accum_state, double* out_rgb) {
    return guard([&] {
        REQUIRE(p && accum_state && out_rgb, "null argument");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_accum_finalize stitches a whole frame: rank / world must be 0 / 1");
        finalize_host(*p, accum_state, out_rgb);
        return (int)RT_OK;
    });
}

// ---- tile-adaptive sampling (the kernels between the passes: device/adaptive.inc) ----
static const double kAdaptiveThreshold = 0.002;  // rt_default_adaptive_config (how it was chosen)
void rt_default_adaptive_config(rt_adaptive_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->min_spp = 16;
    c->threshold = kAdaptiveThreshold;
}
int rt_render_adaptive(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_adaptive_config* cfg, double* out_rgb,
                       int32_t* out_tile_spp, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && cfg && out_rgb, "null argument");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_render_adaptive renders whole frames: world must be 1 and rank 0");
        REQUIRE(p->spp > 0, "spp must be positive");
        REQUIRE(cfg->min_spp >= 2 && cfg->min_spp % 2 == 0 && cfg->min_spp <= p->spp, "min_spp must be even, >= 2 and <= spp");
        REQUIRE(!std::isnan(cfg->threshold) && cfg->threshold >= 0., "threshold must be >= 0 (not NaN)");
        if (p->kernel == 6 || p->integrator == 2)
            throw RtError(RT_ERR_UNSUPPORTED, "rt_render_adaptive runs with kernels 0 / 1 / 2 / 5 and integrators 0 / 1");
        render_adaptive(*s, *cam, *p, *cfg, out_rgb, out_tile_spp, stats);
        return (int)RT_OK;
    });
}

// ---- pixel regions of a frame (the driver: host/frame.cpp render_regions, the crop: device/region.inc) ----
int64_t rt_region_doubles(const rt_params* p, int n_regions, const rt_region* regions) {
    int64_t n = 0;
    const int rc = guard([&] {
        check_regions(p, n_regions, regions);
        n = 3 * region_pixels(n_regions, regions);
        return (int)RT_OK;
    });
    return rc < 0 ? rc : n;
}
int64_t rt_region_tiles(const rt_params* p, int n_regions, const rt_region* regions, int64_t capacity, int32_t* out_tiles) {
    int64_t n = 0;
    const int rc = guard([&] {
        const RenderPlan full = check_regions(p, n_regions, regions);
        REQUIRE(capacity >= 0 && (out_tiles || capacity == 0), "out_tiles may be null only with capacity 0 (capacity must be >= 0)");
        const std::vector<int32_t> tiles = region_tile_list(full, n_regions, regions);
        n = (int64_t)tiles.size();
        if (std::min(capacity, n) > 0) std::memcpy(out_tiles, tiles.data(), (size_t)std::min(capacity, n) * sizeof(int32_t));
        return (int)RT_OK;
    });
    return rc < 0 ? rc : n;
}
int rt_region_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, int n_regions, const rt_region* regions, double* out_rgb,
                     rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && regions && out_rgb, "null argument");
        check_regions(p, n_regions, regions);
        render_regions(*s, *cam, *p, n_regions, regions, out_rgb, false, nullptr, stats);
        return (int)RT_OK;
    });
}
int rt_region_render_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, int n_regions, const rt_region* regions,
                            double* d_out_rgb, void* hip_stream, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && regions && d_out_rgb, "null argument");
        check_regions(p, n_regions, regions);
        render_regions(*s, *cam, *p, n_regions, regions, d_out_rgb, true, hip_stream, stats);
        return (int)RT_OK;
    });
}

int rt_render_sppm_tiles_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_sppm_config* cfg, double* d_tiles,
                                void* hip_stream, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && cfg && d_tiles, "null argument");
        REQUIRE(p->spp > 0, "spp must be positive");
        require_committed(*s);
        require_device();
        const CallClock clock;
        const RenderPlan pl = make_sppm_plan(*p);
        DeviceScope dev_scope(p->device);
        const CameraDev cd = make_camera(*cam);
        rt_stats st{};
        render_sppm(*s, cd, pl, *cfg, d_tiles, nullptr, hip_stream, &st, nullptr);
        clock.finish(stats, st);
        return (int)RT_OK;
    });
}

int rt_assemble_frame_device(const rt_params* p, const double* d_gathered, int64_t tiles_per_rank_stride, double* d_frame,
                             void* hip_stream) {
    return guard([&] {
        REQUIRE(d_gathered && d_frame, "null argument");
        RenderPlan pl = make_plan(p);
        assemble_frame(pl, d_gathered, tiles_per_rank_stride, d_frame, hip_stream);
        return (int)RT_OK;
    });
}

static CameraDev camera_from_frame(const rt_camera_frame& f) {
    CameraDev d;
    for (int i = 0; i < 3; i++) {
        d.origin[i] = f.origin[i]; d.llc[i] = f.lower_left_corner[i]; d.horizontal[i] = f.horizontal[i];
        d.vertical[i] = f.vertical[i]; d.u[i] = f.u[i]; d.v[i] = f.v[i]; d.w[i] = f.w[i];
    }
    d.lens_radius = f.lens_radius;
    return d;
}
int rt_camera_frame_from(const rt_camera* cam, rt_camera_frame* out) {
    return guard([&] {
        REQUIRE(cam && out, "null argument");
        const CameraDev d = make_camera(*cam);
        for (int i = 0; i < 3; i++) {
            out->origin[i] = d.origin[i]; out->lower_left_corner[i] = d.llc[i]; out->horizontal[i] = d.horizontal[i];
            out->vertical[i] = d.vertical[i]; out->u[i] = d.u[i]; out->v[i] = d.v[i]; out->w[i] = d.w[i];
        }
        out->lens_radius = d.lens_radius;
        return (int)RT_OK;
    });
}
static void require_finite(const rt_camera_frame& f) {
    for (const double* v : {f.origin, f.lower_left_corner, f.horizontal, f.vertical, f.u, f.v, f.w})
        for (int i = 0; i < 3; i++) REQUIRE(std::isfinite(v[i]), "camera frame must be finite");
    REQUIRE(std::isfinite(f.lens_radius), "camera frame must be finite");
}
int rt_render_camera_frame(const rt_scene* s, const rt_camera_frame* frame, const rt_params* p, double* out_rgb, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && frame && p && out_rgb, "null argument");
        require_finite(*frame);
        render_frame(*s, camera_from_frame(*frame), *p, out_rgb, stats);
        return (int)RT_OK;
    });
}
int rt_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, double* out_rgb, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && out_rgb, "null argument");
        render_frame(*s, make_camera(*cam), *p, out_rgb, stats);
        return (int)RT_OK;
    });
}

// ---- the frame across the GPUs of one node (host/frame.cpp: render_fanout) ----
int rt_render_multi(const rt_scene* s, const rt_camera* cam, const rt_params* p, int n_devices, const int* device_ids, double* out_rgb,
                    rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam, "null argument");
        require_committed(*s);
        render_fanout(*s, make_camera(*cam), nullptr, p, n_devices, device_ids, out_rgb, stats);
        return (int)RT_OK;
    });
}
int rt_render_multi_camera_frame(const rt_scene* s, const rt_camera_frame* frame, const rt_params* p, int n_devices, const int* device_ids,
                                 double* out_rgb, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && frame, "null argument");
        require_finite(*frame);
        require_committed(*s);
        render_fanout(*s, camera_from_frame(*frame), nullptr, p, n_devices, device_ids, out_rgb, stats);
        return (int)RT_OK;
    });
}
int rt_render_sppm_multi(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_sppm_config* cfg, int n_devices,
                         const int* device_ids, double* out_rgb, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && cfg && p, "null argument");
        REQUIRE(p->spp > 0, "spp must be positive");
        require_committed(*s);
        render_fanout(*s, make_camera(*cam), cfg, p, n_devices, device_ids, out_rgb, stats);
        return (int)RT_OK;
    });
}
int rt_rccl_version(void) { return exchange_library_version(); }

void rt_default_sppm_config(rt_sppm_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->iterations = 50;            // photon_mapper.rs:148
    c->photons_per_iter = 500000;  // photon_mapper.rs:149
    c->k_global = 100;             // GLOBAL_INIT_PHOTONS
    c->k_caustic = 50;             // CAUSTIC_INIT_PHOTONS
    c->max_bounces = 4096;
    c->alpha = 0.7;                // ALPHA
}
int rt_render_sppm(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_sppm_config* cfg, double* out_rgb, double* stats_out,
                   uint64_t photons_stored[2], rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && cfg, "null argument");
        REQUIRE(p->spp == 0 || out_rgb, "null output buffer");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_render_sppm renders the whole frame on one GPU (world must be 1); "
                                               "the tile-partitioned form is rt_render_sppm_tiles_device");
        render_sppm_frame(*s, *cam, *p, *cfg, out_rgb, stats_out, photons_stored, stats);
        return (int)RT_OK;
    });
}
// ---- guide buffers and the a-trous filter (device/aov.inc, device/denoise.hip through the weak declarations of device/denoise.h) ----
int rt_render_aov(const rt_scene* s, const rt_camera* cam, const rt_params* p, int32_t aov_spp, double* out_aov, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && out_aov, "null argument");
        REQUIRE(p->width > 0 && p->height > 0, "width/height must be positive");
        REQUIRE(aov_spp > 0, "aov_spp must be positive");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_render_aov renders whole frames: rank / world must be 0 / 1");
        REQUIRE(p->kernel >= 0 && p->kernel <= 2, "rt_render_aov walks with kernel 0 (auto), 1 or 2");
        require_committed(*s);
        require_device(render_aov != nullptr);
        const CallClock clock;
        DeviceScope dev_scope(p->device);
        rt_stats st{};
        render_aov(*s, make_camera(*cam), p->width, p->height, p->seed, p->t_min, p->kernel, aov_spp, out_aov, &st);
        clock.finish(stats, st);
        return (int)RT_OK;
    });
}
// ---- ambient occlusion (device/ao.inc through the weak declarations of device/ao.h) ----
void rt_default_ao_config(rt_ao_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->ao_spp = 4;
    c->rays_per_hit = 4;
    c->max_distance = INFINITY;
}
// every refusal that needs no device comes before RT_ERR_NO_DEVICE
static int ao_render_entry(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_ao_config* cfg, double* out, bool on_device, void* hip_stream,
                           rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && cfg && out, "null argument");
        REQUIRE(p->width > 0 && p->height > 0, "width/height must be positive");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_ao_render renders whole frames: rank / world must be 0 / 1");
        REQUIRE(cfg->ao_spp >= 1 && cfg->ao_spp <= 4096, "ao_spp must be 1..4096");
        REQUIRE(cfg->rays_per_hit >= 1 && cfg->rays_per_hit <= 256, "rays_per_hit must be 1..256");
        REQUIRE(cfg->max_distance > 0., "max_distance must be > 0 (+inf: no limit)");
        for (int32_t r : cfg->reserved) REQUIRE(r == 0, "rt_ao_config.reserved must be 0");
        REQUIRE(p->kernel >= 0 && p->kernel <= 2, "rt_ao_render walks with kernel 0 (auto), 1 or 2");
        const CameraDev cd = make_camera(*cam);
        choose_pixel_walk(*s, cd, p->t_min, p->kernel, AO_LDS_MAX);  // (the refusals; the launch picks the walk again with its device's LDS)
        require_device(render_ao != nullptr && render_ao_device != nullptr);
        const CallClock clock;
        DeviceScope dev_scope(p->device);
        rt_stats st{};
        if (on_device)
            render_ao_device(*s, cd, p->width, p->height, p->seed, p->t_min, p->kernel, *cfg, out, hip_stream, &st);
        else
            render_ao(*s, cd, p->width, p->height, p->seed, p->t_min, p->kernel, *cfg, out, &st);
        clock.finish(stats, st);
        return (int)RT_OK;
    });
}
int rt_ao_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_ao_config* cfg, double* out_ao, rt_stats* stats) {
    return ao_render_entry(s, cam, p, cfg, out_ao, false, nullptr, stats);
}
int rt_ao_render_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_ao_config* cfg, double* d_out_ao, void* hip_stream,
                        rt_stats* stats) {
    return ao_render_entry(s, cam, p, cfg, d_out_ao, true, hip_stream, stats);
}
void rt_default_denoise_config(rt_denoise_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->iterations = 5;
    c->normal_power_log2 = 7;
    c->sigma_depth = 1.0;
    c->sigma_albedo = 0.1;
    c->sigma_luma = 4.0;
    c->eps = 1e-10;
    c->guides = 7;
}
static void check_denoise_config(const rt_denoise_config* cfg) {
    REQUIRE(cfg->iterations >= 1 && cfg->iterations <= 8, "iterations must be 1..8");
    REQUIRE(cfg->normal_power_log2 >= 0 && cfg->normal_power_log2 <= 16, "normal_power_log2 must be 0..16");
    for (double v : {cfg->sigma_depth, cfg->sigma_albedo, cfg->sigma_luma, cfg->eps})
        REQUIRE(std::isfinite(v) && v > 0., "sigma_depth, sigma_albedo, sigma_luma and eps must be finite and positive");
    REQUIRE(cfg->guides >= 0 && cfg->guides <= 7, "guides is a mask of bits 0 (normal), 1 (depth), 2 (albedo)");
    for (int32_t r : cfg->reserved) REQUIRE(r == 0, "reserved fields of rt_denoise_config must be 0");
}
static void check_denoise_args(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* rgb, const double* variance,
                               const double* aov, const double* out_rgb, const double* out_variance) {
    REQUIRE(cfg && rgb && out_rgb, "null argument");
    REQUIRE(width > 0 && height > 0 && (int64_t)width * height <= (int64_t(1) << 31), "width/height must be positive (at most 2^31 pixels)");
    check_denoise_config(cfg);
    REQUIRE(!out_variance || variance, "out_variance needs a variance input");
    for (const double* o : {out_rgb, out_variance})
        REQUIRE(!o || (o != rgb && o != variance && o != aov), "outputs must not be inputs");
    REQUIRE(!out_variance || out_variance != out_rgb, "out_rgb and out_variance must differ");
}
int rt_denoise(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* rgb, const double* variance, const double* aov,
               double* out_rgb, double* out_variance) {
    return guard([&] {
        check_denoise_args(cfg, width, height, rgb, variance, aov, out_rgb, out_variance);
        require_device(denoise_host != nullptr);
        denoise_host(*cfg, width, height, rgb, variance, aov, out_rgb, out_variance);
        return (int)RT_OK;
    });
}
int rt_denoise_device(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* d_rgb, const double* d_variance,
                      const double* d_aov, double* d_out_rgb, double* d_out_variance, void* hip_stream) {
    return guard([&] {
        check_denoise_args(cfg, width, height, d_rgb, d_variance, d_aov, d_out_rgb, d_out_variance);
        require_device(denoise_device != nullptr);
        denoise_device(*cfg, width, height, d_rgb, d_variance, d_aov, d_out_rgb, d_out_variance, hip_stream);
        return (int)RT_OK;
    });
}
// the symmetric luminance stop: rt_denoise's checks, and a variance (without one the call would be rt_denoise)
int rt_denoise_sym(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* rgb, const double* variance, const double* aov,
                   double* out_rgb, double* out_variance) {
    return guard([&] {
        check_denoise_args(cfg, width, height, rgb, variance, aov, out_rgb, out_variance);
        REQUIRE(variance, "rt_denoise_sym needs a variance: without one the filter is rt_denoise's");
        require_device(denoise_sym_host != nullptr);
        denoise_sym_host(*cfg, width, height, rgb, variance, aov, out_rgb, out_variance);
        return (int)RT_OK;
    });
}
int rt_denoise_sym_device(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* d_rgb, const double* d_variance,
                          const double* d_aov, double* d_out_rgb, double* d_out_variance, void* hip_stream) {
    return guard([&] {
        check_denoise_args(cfg, width, height, d_rgb, d_variance, d_aov, d_out_rgb, d_out_variance);
        REQUIRE(d_variance, "rt_denoise_sym_device needs a variance: without one the filter is rt_denoise_device's");
        require_device(denoise_sym_device != nullptr);
        denoise_sym_device(*cfg, width, height, d_rgb, d_variance, d_aov, d_out_rgb, d_out_variance, hip_stream);
        return (int)RT_OK;
    });
}

// ---- one call from scene to clean frame (the driver: host/frame.cpp render_denoised) ----
static int render_denoised_entry(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* cfg, int32_t luma_mode,
                                 int32_t aov_spp, double* out_rgb, double* out_noisy, double* out_variance, double* out_aov, bool on_device,
                                 void* hip_stream, rt_stats* stats) {
    return guard([&] {
        REQUIRE(s && cam && p && out_rgb, "null argument");
        REQUIRE(p->spp >= 2 && p->spp % 2 == 0, "rt_denoised_render needs an even spp >= 2 (two half-frames)");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_denoised_render renders whole frames: world must be 1 and rank 0");
        REQUIRE(luma_mode == 0 || luma_mode == 1, "luma_mode must be 0 (rt_denoise's luminance stop) or 1 (rt_denoise_sym's)");
        REQUIRE(aov_spp >= 0, "aov_spp must be >= 0 (0: no guides)");
        REQUIRE(aov_spp > 0 || !out_aov, "out_aov must be NULL when aov_spp is 0 (no guides are rendered)");
        rt_denoise_config dc;
        if (cfg) dc = *cfg;
        else rt_default_denoise_config(&dc);
        check_denoise_config(&dc);
        REQUIRE(p->width > 0 && p->height > 0 && (int64_t)p->width * p->height <= (int64_t(1) << 31), "width/height must be positive (at most 2^31 pixels)");
        for (const double* o : {out_noisy, out_variance, out_aov})
            REQUIRE(!o || o != out_rgb, "the outputs must be distinct buffers");
        REQUIRE(!out_noisy || (out_noisy != out_variance && out_noisy != out_aov), "the outputs must be distinct buffers");
        REQUIRE(!out_variance || out_variance != out_aov, "the outputs must be distinct buffers");
        render_denoised(*s, *cam, *p, dc, luma_mode, aov_spp, out_rgb, out_noisy, out_variance, out_aov, on_device, hip_stream, stats);
        return (int)RT_OK;
    });
}
int rt_denoised_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* cfg, int32_t luma_mode,
                       int32_t aov_spp, double* out_rgb, double* out_noisy, double* out_variance, double* out_aov, rt_stats* stats) {
    return render_denoised_entry(s, cam, p, cfg, luma_mode, aov_spp, out_rgb, out_noisy, out_variance, out_aov, false, nullptr, stats);
}
int rt_denoised_render_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* cfg, int32_t luma_mode,
                              int32_t aov_spp, double* d_out_rgb, double* d_out_noisy, double* d_out_variance, double* d_out_aov,
                              void* hip_stream, rt_stats* stats) {
    return render_denoised_entry(s, cam, p, cfg, luma_mode, aov_spp, d_out_rgb, d_out_noisy, d_out_variance, d_out_aov, true, hip_stream, stats);
}

// ---- temporal accumulation (device/temporal.hip through the weak declarations of device/temporal.h; the driver: host/frame.cpp sequence_frame) ----
void rt_default_temporal_config(rt_temporal_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->alpha = 0.2;
    c->plane_tolerance = 0.02;
    c->normal_min = 0.9;
    c->albedo_tolerance = 0.25;
    c->min_weight = 0.25;
    c->max_history = 32;
}
// (every comparison is written so that a NaN fails it)
static void check_temporal_config(const rt_temporal_config* cfg) {
    REQUIRE(cfg->alpha >= 0. && cfg->alpha <= 1., "alpha must be 0..1");
    REQUIRE(cfg->plane_tolerance > 0., "plane_tolerance must be > 0");
    REQUIRE(cfg->normal_min >= -1. && cfg->normal_min <= 1., "normal_min must be -1..1");
    REQUIRE(cfg->albedo_tolerance >= 0., "albedo_tolerance must be >= 0 (+inf: no albedo test)");
    REQUIRE(cfg->min_weight > 0. && cfg->min_weight <= 1., "min_weight must be > 0 and <= 1");
    REQUIRE(cfg->max_history >= 1 && cfg->max_history <= 65536, "max_history must be 1..65536");
    for (int32_t r : cfg->reserved) REQUIRE(r == 0, "reserved fields of rt_temporal_config must be 0");
}
static void check_temporal_size(int32_t width, int32_t height) {
    REQUIRE(width >= 2 && height >= 2 && (int64_t)width * height <= (int64_t(1) << 31), "width and height must be at least 2 (at most 2^31 pixels)");
}
static void check_temporal_args(const rt_temporal_config* cfg, int32_t width, int32_t height, const rt_camera_frame* cam_prev,
                                const rt_camera_frame* cam_cur, const double* rgb, const double* aov, const double* variance,
                                const double* prev_history, const double* prev_aov, const double* out_history, const double* out_variance) {
    REQUIRE(cfg && cam_cur && rgb && aov && out_history, "null argument");
    check_temporal_size(width, height);
    check_temporal_config(cfg);
    REQUIRE((cam_prev && prev_history && prev_aov) || (!cam_prev && !prev_history && !prev_aov),
            "cam_prev, prev_history and prev_aov are given together, or all NULL on a first frame");
    for (const double* o : {out_history, out_variance})
        REQUIRE(!o || (o != rgb && o != aov && o != variance && o != prev_history && o != prev_aov), "outputs must not be inputs");
    REQUIRE(out_variance != out_history, "out_history and out_variance must differ");
}
int rt_temporal_accumulate(const rt_temporal_config* cfg, int32_t width, int32_t height, const rt_camera_frame* cam_prev,
                           const rt_camera_frame* cam_cur, const double* rgb, const double* aov, const double* variance,
                           const double* prev_history, const double* prev_aov, double* out_history, double* out_variance) {
    return guard([&] {
        check_temporal_args(cfg, width, height, cam_prev, cam_cur, rgb, aov, variance, prev_history, prev_aov, out_history, out_variance);
        require_device(temporal_host != nullptr);
        temporal_host(*cfg, width, height, cam_prev, *cam_cur, rgb, aov, variance, prev_history, prev_aov, out_history, out_variance);
        return (int)RT_OK;
    });
}
int rt_temporal_accumulate_device(const rt_temporal_config* cfg, int32_t width, int32_t height, const rt_camera_frame* cam_prev,
                                  const rt_camera_frame* cam_cur, const double* d_rgb, const double* d_aov, const double* d_variance,
                                  const double* d_prev_history, const double* d_prev_aov, double* d_out_history, double* d_out_variance,
                                  void* hip_stream) {
    return guard([&] {
        check_temporal_args(cfg, width, height, cam_prev, cam_cur, d_rgb, d_aov, d_variance, d_prev_history, d_prev_aov, d_out_history, d_out_variance);
        require_device(temporal_device != nullptr);
        temporal_device(*cfg, width, height, cam_prev, *cam_cur, d_rgb, d_aov, d_variance, d_prev_history, d_prev_aov, d_out_history, d_out_variance,
                        hip_stream);
        return (int)RT_OK;
    });
}

int rt_sequence_create(int32_t width, int32_t height, int32_t device, const rt_temporal_config* cfg, rt_sequence** out) {
    return guard([&] {
        REQUIRE(out, "null argument");
        *out = nullptr;
        check_temporal_size(width, height);
        REQUIRE(device >= -1, "device must be a HIP device ordinal or -1 (the device current at the first frame)");
        rt_temporal_config tc;
        if (cfg) tc = *cfg;
        else rt_default_temporal_config(&tc);
        check_temporal_config(&tc);
        rt_sequence* q = new rt_sequence();
        q->width = width;
        q->height = height;
        q->device = device;
        q->cfg = tc;
        *out = q;
        return (int)RT_OK;
    });
}
void rt_sequence_destroy(rt_sequence* q) { delete q; }
int rt_sequence_reset(rt_sequence* q) {
    return guard([&] {
        REQUIRE(q, "null sequence");
        q->frames = 0;
        return (int)RT_OK;
    });
}
int rt_sequence_frames(const rt_sequence* q) {
    return guard([&] {
        REQUIRE(q, "null sequence");
        return q->frames;
    });
}
int rt_sequence_frame(rt_sequence* q, const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* dn, int32_t luma_mode,
                      int32_t aov_spp, double* out_rgb, double* out_accum, double* out_history, double* out_variance, rt_stats* stats) {
    return guard([&] {
        REQUIRE(q && s && cam && p && out_rgb, "null argument");
        REQUIRE(p->width == q->width && p->height == q->height, "width / height differ from the sequence's (a sequence has one frame size)");
        REQUIRE(p->spp >= 2 && p->spp % 2 == 0, "rt_sequence_frame needs an even spp >= 2 (two half-frames)");
        REQUIRE(p->world == 1 && p->rank == 0, "rt_sequence_frame renders whole frames: world must be 1 and rank 0");
        REQUIRE(luma_mode >= -1 && luma_mode <= 1, "luma_mode must be -1 (no filter), 0 (rt_denoise) or 1 (rt_denoise_sym)");
        REQUIRE(aov_spp >= 1, "aov_spp must be >= 1: the temporal step needs guides");
        rt_denoise_config dc;
        if (dn) dc = *dn;
        else rt_default_denoise_config(&dc);
        check_denoise_config(&dc);
        const double* outs[4] = {out_rgb, out_accum, out_history, out_variance};
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < i; j++) REQUIRE(!outs[i] || outs[i] != outs[j], "the outputs must be distinct buffers");
        sequence_frame(*q, *s, *cam, *p, dc, luma_mode, aov_spp, out_rgb, out_accum, out_history, out_variance, stats);
        return (int)RT_OK;
    });
}

int rt_tonemap_u8(const double* rgb, size_t n_channels, uint8_t* out) {
    return guard([&] {
        REQUIRE((rgb && out) || n_channels == 0, "null argument");
        for (size_t i = 0; i < n_channels; i++) out[i] = tonemap_channel(rgb[i]);
        return (int)RT_OK;
    });
}
int rt_write_png(const char* path, int width, int height, const uint8_t* rgb) {
    return guard([&] {
        REQUIRE(path, "null path");
        write_png(path, width, height, rgb);
        return (int)RT_OK;
    });
}

int rt_debug_rng_device(uint64_t seed, uint64_t pixel, uint64_t sample, int n, uint64_t* out_host) {
    return guard([&] {
        REQUIRE(n > 0 && out_host, "bad argument");
        if (device_count() < 1) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        debug_rng_device(seed, pixel, sample, n, out_host);
        return (int)RT_OK;
    });
}
int rt_debug_rng_host(uint64_t seed, uint64_t pixel, uint64_t sample, int n, uint64_t* out_host) {
    return guard([&] {
        REQUIRE(n > 0 && out_host, "bad argument");
        Rng r;
        r.seed_stream(seed, pixel, sample);
        for (int i = 0; i < n; i++) out_host[i] = r.next_u64();
        return (int)RT_OK;
    });
}
int rt_debug_rng_floats(uint64_t seed, uint64_t pixel, uint64_t sample, int n, double lo, double hi, int on_device, double* out_gen,
                        double* out_range) {
    return guard([&] {
        REQUIRE(n > 0 && out_gen && out_range && lo < hi && std::isfinite(hi - lo), "bad argument");
        if (on_device) {
            if (device_count() < 1) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
            debug_rng_floats_device(seed, pixel, sample, n, lo, hi, out_gen, out_range);
            return (int)RT_OK;
        }
        Rng r;
        r.seed_stream(seed, pixel, sample);
        for (int i = 0; i < n; i++) out_gen[i] = r.gen_f64();
        r.seed_stream(seed, pixel, sample);
        for (int i = 0; i < n; i++) out_range[i] = (lo == -1. && hi == 1.) ? r.gen_range_pm1() : (lo == 0. && hi == 1.) ? r.gen_range_01() : r.gen_range(lo, hi);
        return (int)RT_OK;
    });
}
int rt_debug_math_device(int op, size_t n, const double* a_host, const double* b_host, double* out_host) {
    return guard([&] {
        REQUIRE(n > 0 && a_host && out_host && (op == 0 || op == 2 || op == 3 || op == 4 || (op == 1 && b_host)), "bad argument");
        if (device_count() < 1) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        debug_math_device(op, n, a_host, b_host, out_host);
        return (int)RT_OK;
    });
}
int rt_debug_hit_device(const rt_scene* s, int kernel, size_t n, const double* rays_host, double t_min, double t_max, double* out_host) {
    return guard([&] {
        REQUIRE(s && n > 0 && rays_host && out_host && (kernel == 1 || kernel == 2 || kernel == 3 || kernel == 5 || kernel == 6 || kernel == 7 || kernel == 8), "bad argument");
        if (device_count() < 1) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        debug_hit_device(*s, kernel, n, rays_host, t_min, t_max, out_host);
        return (int)RT_OK;
    });
}
// the three env sampling diagnostics run on `device` and leave the caller's current device as it was
static int env_debug(const rt_scene* s, int device, const std::function<void()>& f) {
    return guard([&] {
        REQUIRE(s, "null scene");
        const int n_dev = device_count();
        if (n_dev < 1 || !env_debug_linked()) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        REQUIRE(device >= 0 && device < n_dev, "no such device");
        DeviceScope dev_scope(device);
        f();
        return (int)RT_OK;
    });
}
int rt_debug_env_table_device(const rt_scene* s, int device, int* w, int* h, uint32_t* q_host) {
    return env_debug(s, device, [&] { debug_env_table_device(*s, w, h, q_host); });
}
int rt_debug_env_sample_device(const rt_scene* s, int device, size_t n, const double* xi4_host, double* out_host) {
    return env_debug(s, device, [&] {
        REQUIRE(n > 0 && xi4_host && out_host, "bad argument");
        debug_env_eval_device(*s, 0, n, xi4_host, out_host);
    });
}
int rt_debug_env_pdf_device(const rt_scene* s, int device, size_t n, const double* dirs_host, double* pdf_host) {
    return env_debug(s, device, [&] {
        REQUIRE(n > 0 && dirs_host && pdf_host, "bad argument");
        debug_env_eval_device(*s, 1, n, dirs_host, pdf_host);
    });
}
int rt_debug_area_sample_device(const rt_scene* s, int device, size_t n, const double* in_host, double* out_host) {
    return env_debug(s, device, [&] {
        REQUIRE(n > 0 && in_host && out_host, "bad argument");
        if (&rtamd::debug_area_eval_device == nullptr) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        debug_area_eval_device(*s, 0, n, in_host, out_host);
    });
}
int rt_debug_area_pdf_device(const rt_scene* s, int device, size_t n, const double* rays_host, double* pdf_host) {
    return env_debug(s, device, [&] {
        REQUIRE(n > 0 && rays_host && pdf_host, "bad argument");
        if (&rtamd::debug_area_eval_device == nullptr) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        debug_area_eval_device(*s, 1, n, rays_host, pdf_host);
    });
}
// the shading and object-light diagnostics check their arguments on the host, before they ask for a device
static void index_column(const double* in, size_t n, size_t stride, size_t col, size_t count, const char* what) {
    for (size_t k = 0; k < n; k++) {
        const double v = in[stride * k + col];
        if (!(v >= 0. && v < (double)count && v == std::floor(v))) throw RtError(RT_ERR_ARG, what);
    }
}
static int shade_debug(const rt_scene* s, int device, bool linked, const std::function<void()>& check, const std::function<void()>& f) {
    return guard([&] {
        REQUIRE(s, "null scene");
        check();
        const int n_dev = device_count();
        if (n_dev < 1 || !linked) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        REQUIRE(device >= 0 && device < n_dev, "no such device");
        DeviceScope dev_scope(device);
        f();
        return (int)RT_OK;
    });
}
static void object_lights_only(const rt_scene& s) {
    if (!s.committed) throw RtError(RT_ERR_NOT_COMMITTED, "scene not committed");
    if (s.flat.view.n_lights == 0u) throw RtError(RT_ERR_ARG, "the scene has no object lights (rt_scene_set_lights)");
}
int rt_debug_shade_device(const rt_scene* s, int device, size_t n, const double* in_host, const uint64_t* keys_host, double* out_host) {
    return shade_debug(s, device, &rtamd::debug_shade_device != nullptr, [&] {
        REQUIRE(n > 0 && in_host && keys_host && out_host, "bad argument");
        if (!s->committed) throw RtError(RT_ERR_NOT_COMMITTED, "scene not committed");
        index_column(in_host, n, 17, 0, s->materials.size(), "rt_debug_shade_device: no such material");
        bool mix = false;
        for (size_t k = 0; k < n; k++) mix |= in_host[17 * k + 1] != 0.;
        if (!mix) return;
        object_lights_only(*s);
        if (s->flat.view.off_env != 0u || s->flat.view.off_area != 0u)
            throw RtError(RT_ERR_ARG, "rt_debug_shade_device takes the plain mixture step: object lights only, no env sampling, no area lights");
    }, [&] { debug_shade_device(*s, n, in_host, keys_host, out_host); });
}
int rt_debug_light_sample_device(const rt_scene* s, int device, size_t n, const double* in_host, const uint64_t* keys_host, double* out_host) {
    return shade_debug(s, device, &rtamd::debug_light_eval_device != nullptr, [&] {
        REQUIRE(n > 0 && in_host && keys_host && out_host, "bad argument");
        object_lights_only(*s);
        index_column(in_host, n, 4, 3, s->flat.view.n_lights, "rt_debug_light_sample_device: no such light");
    }, [&] { debug_light_eval_device(*s, 0, n, in_host, keys_host, out_host); });
}
int rt_debug_light_pdf_device(const rt_scene* s, int device, size_t n, const double* rays_host, double* pdf_host) {
    return shade_debug(s, device, &rtamd::debug_light_eval_device != nullptr, [&] {
        REQUIRE(n > 0 && rays_host && pdf_host, "bad argument");
        object_lights_only(*s);
    }, [&] { debug_light_eval_device(*s, 1, n, rays_host, nullptr, pdf_host); });
}
// the walk diagnostic likewise: every refusal that needs no device comes before RT_ERR_NO_DEVICE
int rt_debug_walk_device(const rt_scene* s, int device, int kernel, size_t n, const double* rays_host, const uint64_t* keys_host, double t_min, double* out_host) {
    bool unit_zero = false;
    const int rc = shade_debug(s, device, &rtamd::debug_walk_device != nullptr, [&] {
        REQUIRE(n > 0 && rays_host && keys_host && out_host, "bad argument");
        REQUIRE(kernel >= 1 && kernel <= 3, "rt_debug_walk_device: kernel 1, 2 or 3");
        if (!s->committed) throw RtError(RT_ERR_NOT_COMMITTED, "scene not committed");
        const FlatView& v = s->flat.view;
        if (kernel != 1 && !v.accel_ok) throw RtError(RT_ERR_UNSUPPORTED, "no accel for this scene");
        if (kernel != 1 && !(t_min >= 0.)) throw RtError(RT_ERR_UNSUPPORTED, "kernels 2 and 3 need t_min >= 0 (box32)");
        if (debug_walk_lds_bytes(v, kernel) > DEBUG_WALK_LDS_MAX)
            throw RtError(RT_ERR_UNSUPPORTED, kernel == 3 ? "the NodeW table of this scene does not fit in LDS" : "the walk stacks of this scene do not fit in LDS");
        const bool moving = (v.kinds_mask & (1u << NK_MSPHERE)) != 0;
        for (size_t k = 0; k < n; k++) {
            const double tm = rays_host[7 * k + 6];
            REQUIRE(std::isfinite(tm), "rt_debug_walk_device: a ray time is not finite");
            // the shutter rule of a render: a moving sphere's box covers its positions between ITS time0 and time1 only
            if (moving && !(tm >= s->flat.msph_t0_max && tm <= s->flat.msph_t1_min))
                throw RtError(RT_ERR_ARG, "rt_debug_walk_device: ray time " + std::to_string(tm) + " lies outside [time0, time1] of a moving sphere ([" +
                                              std::to_string(s->flat.msph_t0_max) + ", " + std::to_string(s->flat.msph_t1_min) + "] for this scene)");
        }
    }, [&] { unit_zero = debug_walk_device(*s, kernel, n, rays_host, keys_host, t_min, out_host); });
    if (rc == RT_OK && unit_zero) {
        g_err = "unitizing zero vector (device, walk diagnostic)";
        return RT_ERR_UNIT_ZERO;
    }
    return rc;
}
// the any-hit diagnostic likewise (the rays' origins are the caller's: the origin bound is stated in rtamd.h, not checked)
int rt_debug_occluded_device(const rt_scene* s, int device, int kernel, size_t n, const double* rays_host, double t_min, double* out_host) {
    return shade_debug(s, device, rtamd::debug_occluded_device != nullptr, [&] {
        REQUIRE(n > 0 && rays_host && out_host, "bad argument");
        REQUIRE(kernel == 1 || kernel == 2, "rt_debug_occluded_device: kernel 1 or 2");
        aov_refuse(*s);
        if (kernel == 2 && !accel2_usable(s->flat.view, 0., t_min, 64, AO_LDS_MAX))
            throw RtError(RT_ERR_UNSUPPORTED, "kernel 2 needs an accel, t_min >= 0 (box32) and walk stacks that fit in LDS");
    }, [&] { debug_occluded_device(*s, kernel, n, rays_host, t_min, out_host); });
}
// the SPPM gather diagnostic checks its arguments on the host, before it asks for a device (as shade_debug does)
int rt_debug_sppm_gather_device(int device, rt_debug_sppm_gather* io) {
    bool unit_zero = false;
    const int rc = guard([&] {
        REQUIRE(io, "null argument");
        REQUIRE(io->points && io->stats && io->estimates && (io->global || io->n_global == 0) && (io->caustic || io->n_caustic == 0), "null pointer");
        REQUIRE(io->m > 0 && io->m <= 0x7FFFFFFFull, "m must be 1 .. 2^31 - 1");
        REQUIRE(io->n_global <= 0x40000000ull && io->n_caustic <= 0x40000000ull, "photon map too large");
        REQUIRE(io->k_global >= 1 && io->k_caustic >= 1, "k must be >= 1");
        REQUIRE(io->alpha > 0., "alpha must be > 0");
        REQUIRE(io->shift >= 0 && io->shift <= 60, "S must be 0 .. 60");
        const int n_dev = device_count();
        if (n_dev < 1 || &rtamd::debug_sppm_gather_device == nullptr) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        REQUIRE(device >= 0 && device < n_dev, "no such device");
        DeviceScope dev_scope(device);
        unit_zero = debug_sppm_gather_device(*io);
        return (int)RT_OK;
    });
    if (rc == RT_OK && unit_zero) {
        g_err = "unitizing zero vector (device, SPPM gather)";
        return RT_ERR_UNIT_ZERO;
    }
    return rc;
}
// the SPPM trace diagnostic likewise: its own argument checks, then the refusals of a render (sppm_refuse, device.h), then the device
int rt_debug_sppm_trace_device(const rt_scene* s, const rt_camera* cam, int device, rt_debug_sppm_trace* io) {
    bool unit_zero = false;
    const int rc = guard([&] {
        REQUIRE(s && cam && io, "null argument");
        REQUIRE(io->width >= 2 && io->height >= 2, "width and height must be >= 2 (the eye pass divides by width - 1 and height - 1)");
        REQUIRE((uint64_t)io->width * (uint64_t)io->height <= 0x7FFFFFFFull, "too many pixels");
        REQUIRE(io->iteration >= 0, "iteration must be >= 0");
        REQUIRE(io->photons_per_iter >= 1 && io->max_bounces >= 1, "photons_per_iter and max_bounces must be >= 1");
        REQUIRE(io->capacity_global <= 0x40000000u && io->capacity_caustic <= 0x40000000u, "capacity above 2^30 photons");
        REQUIRE((io->global || io->global_rows == 0) && (io->caustic || io->caustic_rows == 0), "rows without a buffer");
        sppm_refuse(*s, false);
        const int n_dev = device_count();
        if (n_dev < 1 || &rtamd::debug_sppm_trace_device == nullptr) throw RtError(RT_ERR_NO_DEVICE, "no HIP device");
        REQUIRE(device >= 0 && device < n_dev, "no such device");
        DeviceScope dev_scope(device);
        const CameraDev cd = make_camera(*cam);
        unit_zero = debug_sppm_trace_device(*s, cd, *io);
        return (int)RT_OK;
    });
    if (rc == RT_OK && unit_zero) {
        g_err = "unitizing zero vector (device, SPPM trace)";
        return RT_ERR_UNIT_ZERO;
    }
    return rc;
}
int rt_debug_grid_shape(const double* lo3, const double* hi3, uint64_t n, double* cell, int32_t* dim3) {
    return guard([&] {
        REQUIRE(lo3 && hi3 && cell && dim3, "null argument");
        int dim[3];
        if (!grid_shape(lo3, hi3, (size_t)n, cell, dim)) throw RtError(RT_ERR_UNSUPPORTED, "the bounding box is not finite");
        for (int a = 0; a < 3; a++) dim3[a] = dim[a];
        return (int)RT_OK;
    });
}
int rt_debug_schedule(int64_t tiles_owned, int n_waves, int s_begin, int s_end, int sub_spp, int job_units, int* out25) {
    int rounds = 0;
    const int rc = guard([&] {
        REQUIRE(tiles_owned > 0 && n_waves > 0 && s_begin >= 0 && s_end > s_begin && sub_spp >= 1 && sub_spp <= 8 && job_units >= 1 && out25, "bad argument");
        Schedule sch;
        rounds = make_schedule(sch, (int)std::min<int64_t>(tiles_owned, 0x7fffffff), n_waves, s_begin, s_end, sub_spp, job_units);
        for (int i = 0; i < 25; i++) out25[i] = sch.lvl[i / 5][i % 5];
        return (int)RT_OK;
    });
    return rc < 0 ? rc : rounds;
}

}  // extern "C"
