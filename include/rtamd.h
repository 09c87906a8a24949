/*
 * rtamd.h -- C ABI of the MI355X-native radiance path (librtamd.so).
 *
 * Drop-in boundary for ONE hot path of BlackCloud37/rust-raytracer: the
 * per-pixel radiance loop  Camera::capture_image -> Integrator::sample_ray ->
 * World::hit -> {BVHNode,AABB,Sphere,Rect,Triangle,Transform}::hit ->
 * Material::{emitted,scatter}.  The reference has no FFI of its own (SURVEY.md
 * s8b), so every entry point below names the Rust item it stands in for
 * (paths relative to /root/reference/raytracer/src).  The cut is at
 * capture_image granularity: the host walks its Hitable/Material/Texture graph
 * once through the rt_texture_* / rt_material_* / rt_object_* builders (one per
 * reference constructor), commits, and calls rt_render.
 *
 * Conventions
 *   - plain C, pointers + sizes only; no C++/torch types cross this boundary.
 *   - every function returns RT_OK (0) / a non-negative id, or a negative
 *     rt_status; rt_last_error() gives the message (thread-local).  Nothing
 *     aborts or unwinds across the boundary (the reference's panic sites map
 *     to error codes, listed per function).
 *   - the library owns what it copies at build/commit; the caller owns every
 *     buffer it passes in.  An rt_scene is immutable after rt_scene_commit and
 *     may then be rendered from several host threads concurrently.
 *   - all geometry and radiance is f64, as in the reference (vec3.rs:15-19).
 *   - there is NO CPU fallback: without a HIP device the render entry points
 *     fail with RT_ERR_NO_DEVICE.
 */
#ifndef RTAMD_H
#define RTAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTAMD_ABI_VERSION 2   /* 2 (round 5): rt_stats grew by five f64 fields behind reserved[] */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_ARG = -1,          /* bad argument / unknown id */
    RT_ERR_UNIT_ZERO = -2,    /* Vec3::unit of a zero vector      (vec3.rs:88 panic)      */
    RT_ERR_NO_BBOX = -3,      /* "No bounding box in bvh_node constructor" (bvh.rs:43,57) */
    RT_ERR_SINGULAR = -4,     /* "Invalid transform matrix"       (transform.rs:146)      */
    RT_ERR_IO = -5,           /* file cannot be read ("Failed to load OBJ file", mesh.rs:158) */
    RT_ERR_SCHEMA = -6,       /* scene file does not follow the schema of data/ (.json/.yaml) */
    RT_ERR_NO_NORMALS = -7,   /* mesh without vertex normals      (mesh.rs:62 index panic) */
    RT_ERR_NOT_COMMITTED = -8,
    RT_ERR_NO_DEVICE = -9,    /* no HIP device / HIP runtime error: there is no CPU fallback */
    RT_ERR_UNSUPPORTED = -10,
    RT_ERR_HIP = -11,
    RT_ERR_INTERNAL = -12     /* a device-side invariant failed (an instance below an instance reached the serving waves; a request ring overran) */
} rt_status;

typedef struct rt_scene rt_scene; /* opaque: World's object graph + its flattened device form */

/* Camera::new arguments (camera.rs:24-32); data/<scene>.json "camera" block. */
typedef struct rt_camera {
    double look_from[3];
    double look_at[3];
    double vup[3];
    double vfov;       /* degrees */
    double aspect;     /* CONFIGS.aspect_ratio (main.rs:35) */
    double aperture;
    double focus_dist;
} rt_camera;

/* The Camera struct as the reference STORES it (camera.rs:12-21: the derived frame, not the constructor arguments): a host
 * that already owns a `Camera` hands these eight fields over as they are. */
typedef struct rt_camera_frame {
    double origin[3];
    double lower_left_corner[3];
    double horizontal[3];
    double vertical[3];
    double u[3], v[3], w[3];
    double lens_radius;
} rt_camera_frame;

/* capture_image's compile-time constants made run-time (SURVEY.md s5 "Config / flags"). */
typedef struct rt_params {
    int32_t width;       /* CONFIGS.width  (main.rs:34) default 800 */
    int32_t height;      /* CONFIGS.height (main.rs:45) default 800 */
    int32_t spp;         /* sample_per_pixel (camera.rs:73) default 256 */
    int32_t max_depth;   /* photon_mapper.rs:334 default 50 */
    double t_min;        /* photon_mapper.rs:335 default 0.001 */
    uint64_t seed;       /* rtamd-rng-3 stream seed (replaces thread_rng) */
    int32_t rank;        /* image-tile partition: this call renders tiles t with t % world == rank */
    int32_t world;       /* 1 = whole image */
    int32_t spp_chunk;   /* samples per pixel per kernel launch; 0 = all in one launch */
    int32_t kernel;      /* 0 = auto; 1 = reference-order stackless traversal; 2 = SAH-BVH2 accel traversal (auto whenever the
                            scene has a usable accel); 5 = kernel 2's BVH with the cooperative instance service: the walks
                            through mesh instances are queued per workgroup and served by full waves (auto when an
                            instance's object-space BVH has >= 64 nodes; needs 1..64 instances, at least one of f32-vertex triangles);
                            6 = the same service across the whole GPU and across launches (parked paths in HBM pools, a
                            dedicated walk launch per cycle; 1..64 instances, at least one of f32-vertex triangles, as kernel 5; by request only -- it is slower than
                            kernel 5; workspace within rt_tuning.wf_workspace_mb, default 1.9 GB).
                            All give bit-identical images (same f64 primitive tests, same tie rule: when two objects share the
                            closest t EXACTLY the later-visited one wins unless the reference's own BVHNode box test would have
                            culled it -- bvh.rs:88, aabb.rs:28-30 -- in every kernel). */
    int32_t device;      /* HIP device ordinal; -1 = current */
    int32_t integrator;  /* 0 = sample_ray as the reference structures it (BSDF sampling only; default);
                            1 = light importance sampling: on Diffuse hits the direction is drawn from the
                                0.5*lights + 0.5*cosine mixture pdf (book-3 MixturePDF semantics; needs rt_scene_set_lights);
                            2 = the reference's SPPM sample_ray (only through rt_render_sppm) */
    double time0, time1; /* book-2 extension (the reference has no code for it: its Ray has no time, ray.rs:3-6): the camera's shutter.
                            With time1 > time0 every sample draws a time in [time0, time1] (gen_range's product may round up to time1) right after its lens sample and moving spheres
                            (rt_object_moving_sphere) are where they are at that time; default 0, 0 = no draw */
} rt_params;

typedef struct rt_stats {
    double seconds;          /* wall time of the call (host clock) */
    double kernel_ms;        /* sum of path-trace kernel launch durations (HIP events on the launch stream) */
    double reduce_ms;        /* 0: the ordered reduction happens inside the path-trace kernel */
    uint64_t samples;        /* pixel-samples traced by this call (this rank) */
    int32_t launches;        /* path-trace kernel launches */
    int32_t kernel_used;     /* which kernel ran */
    int32_t scene_in_lds;    /* 1 if the flattened scene was staged into LDS */
    int32_t block_threads;
    int32_t grid_blocks;
    int32_t spp_chunk;
    uint64_t scene_bytes;    /* flattened scene size */
    uint64_t reserved[4];    /* [0] SPPM pre-pass microseconds, [1] render workspace bytes on the device; rt_render_multi, entry 0: [2] microseconds from
                                the last rank's finish until every row had arrived on the root device (the exchange proper: no stitch, no host copy),
                                [3] rows that travelled through RCCL */
    /* ABI version 2: */
    double upload_ms;        /* copying the scene to this call's device (0 when a copy was already there: uploads happen once per scene and device) */
    double posted_ms;        /* rt_render_multi, entry i: when rank i's rows were handed to the exchange, ms after the call began (its own finish time;
                                0 for rows rendered in place on the root device) */
    double stitch_copy_ms;   /* rt_render_multi, entry 0: the stitch on the root device and the copy of the frame to out_rgb */
    double comm_init_ms;     /* rt_render_multi, entry 0: creating the RCCL communicators of this device list (0 when they were cached) */
    double exchange_ms;      /* rt_render_multi, entry 0: reserved[2] in ms */
} rt_stats;

/* ---- library ------------------------------------------------------------ */
int rt_abi_version(void);
const char* rt_last_error(void);
void rt_default_params(rt_params* p);           /* the reference's constants, see rt_params */
int rt_device_count(void);                      /* HIP devices visible; 0 without a GPU */

/* Measurement and test hooks.  The library reads NO environment variable: everything that changes how (never what) it
 * renders is set here, process-wide, before the calls it should affect.  0 / negative = automatic (the default). */
typedef struct rt_tuning {
    int32_t no_lds;                /* 1: keep scene tables in global memory even when they fit LDS (A/B runs)            */
    int32_t top_nodes;             /* >= 0: cap on the BVH nodes cached in LDS when the scene lives in L2/HBM; -1 auto  */
    int32_t sub_spp;               /* 1..8: sample indices per work unit (a wave's pool = 64 px x sub_spp); 0 auto      */
    int32_t coop_pool;             /* 1..1024: parked-path slots per workgroup in kernel 5 (small values force its in-lane fallback); 0 auto */
    int32_t max_leaf;              /* 1..4: accel builder, items per leaf; 0 auto (read at rt_scene_commit)             */
    int32_t sppm_photon_capacity;  /* > 0: initial photon-buffer capacity (forces the grow-and-retry path); 0 auto      */
    int32_t sppm_knn_candidates;   /* >= 0: k-nearest candidates kept in LDS (0 forces the out-of-LDS selection); -1 auto */
    int32_t multi_force_rccl;      /* 1: rt_render_multi sends EVERY rank's rows through the RCCL communicator, also those that already sit on
                                      the root device (a rank then sends to itself): exercises the exchange on a one-GPU box; 0 auto      */
    int32_t wf_workspace_mb;       /* > 0: kernel 6's workspace budget in MB (unit buffers + record pools; default 1900); 8600 = what round 3 took */
    int32_t reserved;
    double sah_box_cost;           /* > 0: accel builder, SAH cost of a box-pair test relative to 2.0 per primitive; 0 auto */
} rt_tuning;
void rt_tuning_default(rt_tuning* t);
int rt_tuning_set(const rt_tuning* t);
/* The render entry points keep a workspace per device for the life of the process (unit rings of the resident waves, ~0.3 GB,
 * accumulator, tickets: no hipMalloc on the hot path), rt_render_multi also its RCCL communicators and its frame-sized buffers (gathered
 * rows, stitched frame, the ranks' rows: up to 4 idle ones per device and size and at most 1 GiB of idle buffers in all -- beyond that
 * the least recently returned ones are freed).  This frees the idle ones;
 * returns the bytes released. */
int64_t rt_release_workspaces(void);

/* ---- scene graph builders (one per reference constructor) ---------------- */
int rt_scene_create(rt_scene** out);
void rt_scene_destroy(rt_scene* s);

/* material.rs:48-50  ConstantTexture(Vec3) / CheckerTexture(t0,t1) / ImageTexture(rgb8, row-major, top row first) */
int rt_texture_constant(rt_scene* s, const double color[3]);
int rt_texture_checker(rt_scene* s, int t0, int t1);
int rt_texture_image(rt_scene* s, int width, int height, const uint8_t* rgb);
/* Book-2 extension, no reference counterpart (BASELINE config C5 names it): noise_texture(scale), the marble texture
 * 0.5 (1 + sin(scale p.z + 10 turb(p))) over Perlin noise with 7 octaves of turbulence; the 256 gradient vectors and the three
 * permutations come from the RNG stream (seed, "perlin" key, 0); sin is the deterministic rtamd-sin-1 (csrc/common/detsin.h).
 * The lattice index of an octave's coordinate x is floor(x) mod 256 of the mathematical integer (0..255) for every finite x -- so 0 for
 * every |x| >= 2^60 -- and 0 for a non-finite x: defined at every coordinate a scene can hold (see "diagnostics", Noise).
 * A scene that holds a noise texture -- on a material or as its background -- is a book-2 scene, as one with moving spheres or an open
 * shutter: it renders with kernels 1 and 2 and integrator 0; integrator 1 and kernels 5 / 6 are RT_ERR_UNSUPPORTED. */
int rt_texture_noise(rt_scene* s, double scale, uint64_t seed);
/* material.rs:88-212  Lambertian::new / Metal::new / Dielectric::new / DiffuseLight::new */
int rt_material_lambertian(rt_scene* s, int albedo_tex);
int rt_material_metal(rt_scene* s, int albedo_tex, double fuzz);
int rt_material_dielectric(rt_scene* s, double ir, int albedo_tex);
int rt_material_diffuse_light(rt_scene* s, int emit_tex);
/* material.rs:213-231  Isotropic::new(albedo) -- commented out in the reference; the phase function of a ConstantMedium:
 * scatter = (albedo, Ray(p, random_in_unit_sphere())); treated as a pass-through (Specular) interaction by every integrator */
int rt_material_isotropic(rt_scene* s, int albedo_tex);

/* objects/sphere.rs:9-13 */
int rt_object_sphere(rt_scene* s, const double center[3], double radius, int material);
/* Book-2 extension, no reference counterpart: moving_sphere(center0, center1, time0, time1, radius, material) -- Sphere::hit around
 * the centre center0 + (center1 - center0) (ray.time - time0) / (time1 - time0); box = the union of the boxes at both times.
 * Rendered by kernels 1 and 2 with integrator 0 (integrator 1 and kernels 5 / 6 are RT_ERR_UNSUPPORTED, also for any scene rendered with
 * an open shutter); needs rt_params.time1 > rt_params.time0 to move.  The shutter [rt_params.time0,
 * rt_params.time1] must lie inside [time0, time1] of every moving sphere of the scene (their boxes are the union of the boxes at those two
 * times): a render with a shutter outside that range is refused with RT_ERR_ARG */
int rt_object_moving_sphere(rt_scene* s, const double center0[3], const double center1[3], double time0, double time1, double radius, int material);
/* objects/rectangle.rs:7-12,44-49,82-87 : {a0,b0}=xy0|xz0|yz0, {a1,b1}=xy1|xz1|yz1, k = z|y|x */
int rt_object_rect_xy(rt_scene* s, double x0, double y0, double x1, double y1, double z, int material);
int rt_object_rect_xz(rt_scene* s, double x0, double z0, double x1, double z1, double y, int material);
int rt_object_rect_yz(rt_scene* s, double y0, double z0, double y1, double z1, double x, int material);
/* objects/cube.rs:16 Cube::new(box_min, box_max, mat) */
int rt_object_cube(rt_scene* s, const double box_min[3], const double box_max[3], int material);
/* SphereDiffuseLight::new(center, radius, flux, scale) light.rs:74-86 / XZRectLight::new(xz0, xz1, y, flux, scale)
 * light.rs:134-146 : as a Hitable the light is its primitive + DiffuseLight(ConstantTexture(flux)); `scale` only feeds
 * the photon power (flux * scale) of the SPPM pre-pass */
int rt_object_sphere_light(rt_scene* s, const double center[3], double radius, const double flux[3], double scale);
int rt_object_xz_rect_light(rt_scene* s, double x0, double z0, double x1, double z1, double y, const double flux[3], double scale);
/* objects/medium.rs:16 ConstantMedium::new(d, boundary, phase_function): constant-density participating medium inside
 * `boundary` (any Hitable with a box, not itself a medium).  Its hit() draws a random number (medium.rs:37-38) from the path's
 * stream, in the reference's visit order: kernels 1 and 2 render such scenes with integrator 0, and rt_render_sppm* with all three
 * passes (a volume event is a pass-through interaction: no photon, no gather point); integrator 1, kernels 5 / 6, a medium inside a
 * medium's boundary and, under SPPM, a light inside a medium's boundary are refused with RT_ERR_UNSUPPORTED.  Under a background
 * (rt_scene_set_background) such scenes render with kernels 1 and 2 and integrator 0; SPPM refuses every scene with a background.  The
 * logarithm is the deterministic rtamd-ln-1 (csrc/common/detlog.h, < 1 ulp from libm). */
int rt_object_constant_medium(rt_scene* s, double density, int boundary, int phase_material);
/* objects/mesh.rs:149 Mesh::load_obj given parsed arrays: positions/normals n_vert*3, indices n_tri*3.
 * normals == NULL -> RT_ERR_NO_NORMALS unless synthesize_normals != 0 (area-weighted smooth normals). */
int rt_object_mesh(rt_scene* s, int n_vert, const double* positions, const double* normals, int n_tri, const uint32_t* indices,
                   int material, int synthesize_normals, uint64_t bvh_seed);
/* Mesh::load_obj(path, material): tobj{single_index, triangulate} semantics, models[0] */
int rt_object_mesh_obj(rt_scene* s, const char* obj_path, int material, int synthesize_normals, uint64_t bvh_seed);
/* objects/transform.rs:17 Transform::new(rotate_in_degree, scale, translate, obj): M = T*S*Rx*Ry*Rz
 * Transforms may nest (a Transform whose object is, or contains, another Transform) up to 8 levels; rt_scene_commit refuses a deeper
 * chain with RT_ERR_UNSUPPORTED.  A scene that nests renders through kernels 1 and 2 (the automatic choice is kernel 2) with every
 * integrator; kernels 5 / 6 refuse it with RT_ERR_UNSUPPORTED (rt_scene_info.accel_compact = 0).  A light of rt_scene_set_lights under a Transform is refused
 * at commit (an area light, rt_scene_set_area_lights, may lie under Transforms); a ConstantMedium under a Transform, at any depth, renders through kernel 1 only, as at depth 1. */
int rt_object_transform(rt_scene* s, const double rotate_deg[3], const double scale[3], const double translate[3], int object);
/* Transform as the reference stores it (transform.rs:9-14: obj, trans, inverse_trans; row-major 4x4).  inverse_trans may be
 * NULL (computed as try_inverse does; RT_ERR_SINGULAR if there is none). */
int rt_object_transform_matrix(rt_scene* s, const double trans[16], const double* inverse_trans, int object);
/* Triangle::new on shared vertex arrays (mesh.rs:8-53: a, b, c index Arc<Vec<Vec3>> positions / normals): rt_mesh_data registers
 * the arrays once (returns a mesh id, not an object id), rt_object_triangle one triangle; the host keeps its own BVHNode tree
 * over them (rt_object_bvh_node), e.g. Mesh.bvh as BVHNode::new really built it. */
int rt_mesh_data(rt_scene* s, int n_vert, const double* positions, const double* normals);
int rt_object_triangle(rt_scene* s, int mesh, uint32_t a, uint32_t b, uint32_t c, int material);
/* impl Hitable for Vec<Arc<dyn Hitable>> (objects/hit.rs:56-93) */
int rt_object_list(rt_scene* s, int n, const int* objects);
/* BVHNode::construct(left,right) (bvh.rs:47-58) and BVHNode::new(src_objects) (bvh.rs:60-83; split axes from
 * the seeded rtamd-rng-3 "bvh" stream instead of thread_rng) */
int rt_object_bvh_node(rt_scene* s, int left, int right);
int rt_object_bvh_build(rt_scene* s, int n, const int* objects, uint64_t bvh_seed);
/* Hitable::bounding_box (objects/hit.rs:53): out = min[3], max[3]; RT_ERR_NO_BBOX for None */
int rt_object_bounding_box(const rt_scene* s, int object, double out_min_max[6]);

/* Introspection of the host-side object graph (the walk a `Describe` visitor of the reference's trait objects does the
 * other way round): what an object id stands for, its parameters and its children.
 *   sphere:    v = {center[3], radius}                      (objects/sphere.rs:9-13)
 *   moving sphere: v = {center0[3], radius, center1[3]} (its times are not reported)
 *   rect:      v = {a0, b0, a1, b1, k}, axis = constant axis (0: YZRectangle x=k, 1: XZRectangle y=k, 2: XYRectangle z=k)
 *   triangle:  v = {ia, ib, ic} vertex indices of its mesh  (objects/mesh.rs:8-14)
 *   medium:    v = {density}, material = phase function, children = {boundary}   (objects/medium.rs:9-13)
 *   cube / list / mesh / transform / bvh: children only (cube: its 6 sides; mesh: its inner BVHNode; bvh: {left, right}) */
typedef enum rt_object_type {
    RT_OBJ_SPHERE = 0, RT_OBJ_RECT = 1, RT_OBJ_CUBE = 2, RT_OBJ_TRIANGLE = 3, RT_OBJ_MESH = 4, RT_OBJ_TRANSFORM = 5,
    RT_OBJ_LIST = 6, RT_OBJ_BVH = 7, RT_OBJ_MEDIUM = 8, RT_OBJ_MOVING_SPHERE = 9
} rt_object_type;
typedef struct rt_object_desc {
    int32_t type;        /* rt_object_type */
    int32_t material;    /* material id, -1 for containers */
    int32_t n_children;
    int32_t axis;        /* rect only */
    double v[8];
} rt_object_desc;
int rt_scene_root(const rt_scene* s);            /* object id of the root (World.bvh / the file's top-level list), RT_ERR_ARG if unset */
int rt_object_describe(const rt_scene* s, int object, rt_object_desc* out);
int rt_object_children(const rt_scene* s, int object, int capacity, int* out);  /* writes min(capacity, n) ids, returns n */

/* World::new(hitable_list, cam, lights) (world.rs:15-25): root = BVHNode::new(list) */
int rt_world_new(rt_scene* s, int n, const int* objects, uint64_t bvh_seed);
/* World::new's `lights: Vec<Arc<dyn Light>>` (world.rs:18; scene.rs:110 passes the XZRectLight): the objects that the
 * mixture-pdf integrator samples.  Each must be a sphere or an XZ rectangle in world space (the reference's two Light
 * impls, light.rs:67-86,127-146); RT_ERR_UNSUPPORTED for lights under a Transform.  Every other emissive shape -- an XY or YZ
 * rectangle, a cube, triangles and meshes, any of them under Transforms -- goes to rt_scene_set_area_lights below.  A background (rt_scene_set_background) is a
 * light of integrator 1 only where the scene switched env sampling on (rt_scene_set_env_sampling below): then it is one more strategy
 * of the light half of the mixture, and a scene lit by nothing else needs no object lights.  Without that switch integrator 1 reaches
 * the background by the BSDF and light-sampled directions of the mixture only.  rt_render_sppm* refuses a scene with a background
 * either way (the photon pass has no environment emitter). */
int rt_scene_set_lights(rt_scene* s, int n, const int* objects);
/* root = an existing object (e.g. the HitableList of a scene file) */
int rt_scene_set_root(rt_scene* s, int object);
/* ---- background (no reference counterpart: a miss ends sample_ray with what it has, photon_mapper.rs:335,364) ----
 * What a ray that leaves the scene sees.  A ray that the segment loop traces and that hits nothing adds beta (x) B(d) to L (per
 * channel: L_c + beta_c * B_c), then the path ends.  A hit at depth == 0 still ends the path without a background (Q12 unchanged).
 * With u = unit(d) (the kernels' unit(): sqrt(sqlen) followed by a division), in f64 without contraction:
 *   kind 0: none -- black, the default; the scene keeps the flattened blob and the fingerprint it had without this call.
 *   kind 1: B = scale * color0, per channel.
 *   kind 2: t = 0.5 * (u.y + 1.0), c = (1.0 - t) * color0 + t * color1, B = scale * c.  color0 is the colour straight down
 *           (u.y = -1), color1 straight up; book 1's sky is color0 = (1, 1, 1), color1 = (0.5, 0.7, 1.0).
 *   kind 3: B = scale * tex_color(texture, rec) with rec.p = u and (rec.u, rec.v) = Sphere::get_uv(u) (sphere.rs:16-20, the
 *           deterministic acos / atan2 of D10): an ImageTexture is an equirectangular map with its top row up; checker and noise
 *           textures work too.
 * Set before rt_scene_commit, like every builder.  RT_ERR_ARG: a kind outside 0..3, a texture that is not one of this scene's for
 * kind 3, a non-finite or negative colour component or scale, a call after commit.  The background is part of the flattened scene, so
 * rt_scene_fingerprint tells scenes with different backgrounds apart.  It reaches every render entry point that runs kernels 1 / 2
 * (rt_render, rt_render_camera_frame, rt_render_tiles_device, rt_render_accumulate(_device), rt_render_adaptive, rt_render_multi*)
 * with integrators 0 and 1; kernels 5 / 6 requested explicitly and rt_render_sppm* are RT_ERR_UNSUPPORTED for a scene with a
 * background (kind != 0), and the automatic choice is kernel 2 (kernel 1 without an accel).  rt_render_aov and rt_denoise are
 * unchanged: their guides are first-hit data. */
typedef struct rt_background {
    int32_t kind;      /* 0 none (black, the default); 1 constant colour; 2 vertical gradient; 3 texture by direction */
    int32_t texture;   /* kind 3: any texture id of this scene */
    double color0[3];  /* kind 1: the colour; kind 2: the colour straight down (unit(d).y = -1) */
    double color1[3];  /* kind 2: the colour straight up (unit(d).y = +1) */
    double scale;      /* multiplies the colour; finite, >= 0 */
} rt_background;
int rt_scene_set_background(rt_scene* s, const rt_background* bg);
int rt_scene_get_background(const rt_scene* s, rt_background* out);
/* ---- env sampling: the background as a light of integrator 1 (no reference counterpart) ----
 * Off by default; a scene that leaves it off keeps its blob, its fingerprint, its kernels and every image.  Enabled, every device the
 * scene is uploaded to builds a piecewise-constant distribution over the (u, v) square of Sphere::get_uv from the background B(d) above,
 * W x H cells, cell (i, j) = u in [i/W, (i+1)/W), v in [j/H, (j+1)/H) (v = 0 is straight down; an ImageTexture flips v, so image row r
 * from the top is table row H - 1 - r).  All of it in f64 without contraction; PI = 3.14159265358979323846, sin = rtamd-sin-1 (det_sin),
 * cos x = det_sin(x + PI / 2.0):
 *   weight  theta = PI * ((j + 0.5) / H), phi = (2.0 * PI) * ((i + 0.5) / W), st = det_sin(theta),
 *           d_ij = (-(cos phi * st), -cos theta, sin phi * st), (r, g, b) = B(d_ij) (the very function that shades a miss, which
 *           normalises d_ij once more), w_ij = ((0.2126 r + 0.7152 g) + 0.0722 b) * st.
 *   q_ij    0 where w_ij is not > 0, otherwise max(1, floor((w_ij / w_max) * 4294967295.0)) as uint32, w_max the largest w_ij.  Row
 *           sums, their prefix sums and `total` are uint64, so no order of summation shows.  total == 0 (a black background) switches
 *           the strategy off: the scene renders as if env sampling were not enabled, the refusal of a scene without lights included.
 *   draw    four gen_f64 draws xi1..xi4 in this order: row j = the first row whose inclusive prefix sum of row totals exceeds
 *           min(total - 1, (uint64)(xi1 * (double)total)); column i likewise within row j from xi2 and the row's total;
 *           u = (i + xi3) / W, v = (j + xi4) / H, theta = PI * v, phi = (2.0 * PI) * u, and d by the formula of d_ij.
 *   pdf     of ANY direction d: n = unit(d), (u, v) = get_uv(n) (rtamd-acos-1 / rtamd-atan2-1), i = min(W - 1, (int)floor(W * u)),
 *           j = min(H - 1, (int)floor(H * v)), s2 = 1.0 - n.y * n.y; 0 where s2 is not > 0, otherwise
 *           p = ((((double)q_ij / (double)total) * (double)W) * (double)H) / (((2.0 * PI) * PI) * sqrt(s2)).
 *   mixture with L >= 0 object lights the light half of integrator 1 picks one of L + 1 strategies by (uint32)(gen_f64() * (L + 1))
 *           (clamped to L), index L being the environment, and pdf = 0.5 * ((sum of the light pdfs + p) / (L + 1)) + 0.5 * cosine / PI,
 *           the sum taken lights first.  Weight, termination and what a miss adds are unchanged.  The cosine half reaches every
 *           direction the BSDF scatters into, so the estimator is unbiased whatever the table's resolution.
 * width = height = 0: automatic -- a kind-3 background whose texture is an ImageTexture gets one cell per texel, both axes halved
 * together (integer division, an axis never below 1) while the width exceeds 4096 or the height 2048; every other background 256 x 128.  The table lives in device memory
 * beside the scene's upload, is freed with it and is not part of the blob; the blob gains a 16-byte record {1, W, H}, so
 * rt_scene_fingerprint tells a scene with env sampling from one without and two table sizes apart.
 * RT_ERR_ARG: enabled outside 0 / 1, a negative size, only one of width / height zero, a size above 8192 x 8192, a call after commit;
 * at rt_scene_commit, enabled with a background of kind 0.  Only integrator 1 on kernels 1 / 2 changes; everything integrator 1 refuses
 * without env sampling (media, the book-2 kinds, kernels 5 / 6 under a background) stays refused, and so does rt_render_sppm*. */
typedef struct rt_env_sampling {
    int32_t enabled;        /* 0 (default) / 1 */
    int32_t width, height;  /* table resolution; 0, 0 = automatic */
} rt_env_sampling;
int rt_scene_set_env_sampling(rt_scene* s, const rt_env_sampling* cfg);
int rt_scene_get_env_sampling(const rt_scene* s, rt_env_sampling* out);  /* what was set (0, 0 stays 0, 0) */
/* ---- area lights: emissive rectangles, cubes and meshes as lights of integrator 1 (no reference counterpart) ----
 * A second light list beside rt_scene_set_lights (which keeps its meaning, its refusals and its bits).  An area light is any object whose
 * leaves are rectangles (any axis), cubes or triangles: whole meshes, lists and BVH nodes of such leaves, and any of these under up to 8
 * nested Transforms.  Set before rt_scene_commit; n == 0 clears the list, and a scene with an empty list keeps its blob, its fingerprint,
 * its kernels and every image.  RT_ERR_ARG: an unknown id, a call after commit, a subtree that holds a sphere, a moving sphere or a medium,
 * a leaf whose material is not a DiffuseLight, a Transform chain deeper than 8.
 *   lowering  rt_scene_commit lowers the list to ONE table of world-space triangles, in f64 without contraction, objects in list order:
 *             a rectangle with corners P00, P10, P01, P11 (the first in-plane axis varies first: x for XY and XZ, y for YZ) gives
 *             (P00, P10, P11) and (P00, P11, P01); a cube its six sides in rt_object_children order, each as a rectangle;
 *             rt_object_triangle its three positions; a mesh its triangles in the order of `indices` (not of its inner BVH); a list / BVH
 *             node its children in order; a Transform maps its child's vertices by its stored `trans` (vec3.rs:174-178, w = 1), innermost
 *             first.  Per triangle (a, b, c): e0 = b - a, e1 = c - a, n = cross(e0, e1), area2 = sqrt(sqlen(n)); a triangle whose area2 is
 *             0 or not finite is dropped.  Per light L: q_k = max(1, floor(area2_k / area2_max_L * 4294967295.0)) as uint32, area2_max_L
 *             the light's largest area2; the inclusive prefix sums of q within the light and total_L are uint64.
 *             At commit: more than 1024 triangles over all area lights is RT_ERR_UNSUPPORTED (the pdf below is a linear scan), an area
 *             light with no triangle of non-zero area RT_ERR_ARG.  The table is part of the blob, so rt_scene_fingerprint tells a scene
 *             with area lights from the same scene without them.
 *   draw      from light L at point o, three gen_f64 draws xi1..xi3: triangle k = the first whose inclusive prefix sum exceeds
 *             min(total_L - 1, (uint64)(xi1 * (double)total_L)); u = xi2, v = xi3, and if u + v > 1.0 then u = 1.0 - u, v = 1.0 - v;
 *             p = a + (e0 * u + e1 * v), dir = p - o.
 *   pdf       of (o, d) for light L: the sum, from 0.0 in table order, over the light's triangles that Triangle::hit (mesh.rs:57-102, on
 *             (a, e0, e1), t in [0.001, +inf]) accepts, of (((double)q_k / (double)total_L) * dist2) / (cosine * (0.5 * area2_k)) with
 *             dist2 = (t * t) * sqlen(d) and cosine = fabs(dot(d, n_k) / (sqrt(sqlen(d)) * area2_k)); a term whose cosine is not > 0 is
 *             skipped.  Emission is two-sided (material.rs:209-211 has no face test), hence the fabs.
 *   mixture   with L object lights, M area lights and E in {0, 1} environment strategies (env sampling above) n = L + M + E; the light half
 *             picks (uint32)(gen_f64() * n), clamped to n - 1: [0, L) the object lights, [L, L + M) the area lights, L + M the environment;
 *             pdf = 0.5 * ((the sum of the n pdfs, in that order) / n) + 0.5 * cosine / PI.  Weight, termination and what a miss adds are
 *             unchanged.  A scene with area lights and no object lights renders under integrator 1.
 * Only integrator 1 on kernels 1 / 2 changes (the automatic choice is kernel 2, or 1 without an accel): integrator 0 ignores the list, bit
 * for bit; kernels 5 / 6 under integrator 1 and rt_render_sppm* (the photon pass has no emitter for them) are RT_ERR_UNSUPPORTED for a
 * scene with area lights; media and the book-2 kinds stay refused under integrator 1. */
int rt_scene_set_area_lights(rt_scene* s, int n, const int* objects);
typedef struct rt_area_tri {
    double a[3], e0[3], e1[3], n[3];
    double area2;
    uint32_t q;
    int32_t light;     /* index into the list of rt_scene_set_area_lights */
} rt_area_tri;
/* the lowered table of a committed scene (host only, no device): writes min(capacity, N) records, returns N */
int rt_scene_area_light_tris(const rt_scene* s, int capacity, rt_area_tri* out);
/* scene.rs:16-112 cornell_box_scene(): the reference's only built-in scene, numbers verbatim.
 * cube_obj_path = "data/mesh/cube.obj" of the reference. */
int rt_scene_cornell_box(rt_scene* s, const char* cube_obj_path, double aspect_ratio, uint64_t bvh_seed, rt_camera* cam_out);
/* data/<name>.json|.yaml loader (schema SURVEY.md sA.1; README.md:86-89 Track 5). File BVH topology is kept
 * verbatim, the redundant "bounding_box" is recomputed as BVHNode::construct does. Creates AND commits. */
int rt_scene_load_file(const char* path, rt_scene** out, rt_camera* cam_out);
/* The same scene as rt_scene_load_file, left UNcommitted: builders such as rt_scene_set_background or rt_scene_set_lights still apply,
 * and rt_scene_commit then flattens it to the blob rt_scene_load_file would have made (with the additions). */
int rt_scene_parse_file(const char* path, rt_scene** out, rt_camera* cam_out);
/* flatten the graph into the linear device form (DFS pre-order program, SoA tables) */
int rt_scene_commit(rt_scene* s);

/* introspection of the flattened form (tests, INTEGRATION) */
typedef struct rt_scene_info {
    int32_t n_nodes, n_boxes, n_spheres, n_rects, n_tris, n_xforms, n_materials, n_textures;
    int32_t n_verts, max_depth, committed, n_cubes;   /* a Cube is one record and one node (six sides scanned by the kernel's cube_hit) */
    uint64_t bytes;
    int32_t accel_ok, accel_nodes, accel_items, accel_instances, accel_stack, accel_compact;  /* accel_compact: 1 if the compact object-space copies kernel 5 needs were built */
} rt_scene_info;
int rt_scene_info_get(const rt_scene* s, rt_scene_info* out);
/* What a saved accumulator state (rt_render_accumulate) belongs to, beside its rt_params: a 64-bit fingerprint of the committed scene (FNV-1a
 * over the flattened blob: geometry, materials, textures, BVH wiring; 0 for a scene that is not committed) and the version of everything
 * that decides the bits of an image -- RNG, deterministic ln / sin, sampling order (a string such as "rtamd-image-5 rng-3 ln-1 sin-1").
 * A checkpoint written by another build or for another scene must not be resumed: the host compares both (host_cpp/rtamd.hpp does). */
uint64_t rt_scene_fingerprint(const rt_scene* s);
const char* rt_spec_version(void);

/* ---- the hot path -------------------------------------------------------- */
/* Camera::capture_image (camera.rs:66-128) minus the u8 conversion: linear radiance (sum/spp), f64 RGB,
 * row-major, y down, into caller-owned HOST memory out_rgb[height*width*3].  world > 1 renders only this
 * rank's tiles (others left 0).
 * Where a call meets several of the refusals documented with the builders above, the first of this list answers (p->kernel 0 picks a
 * kernel that steps 1 to 4 accept, so only steps 5 to 7 can refuse it):
 *   1. a background and kernel 5 / 6: RT_ERR_UNSUPPORTED;           2. area lights, integrator 1 and kernel 5 / 6: RT_ERR_UNSUPPORTED;
 *   3. kernel 5 / 6 on a scene they cannot render (a ConstantMedium, a book-2 scene, nested Transforms, no instance of f32-vertex
 *      triangles, more than 64 instances): RT_ERR_UNSUPPORTED;        4. kernel 2 without a usable accel (a ConstantMedium under a
 *      Transform among the reasons): RT_ERR_UNSUPPORTED;
 *   5. integrator 1 on a scene without object lights, area lights and a sampled environment: RT_ERR_ARG;
 *   6. integrator 1 on a book-2 scene: RT_ERR_UNSUPPORTED;           7. integrator 1 on a scene with a ConstantMedium: RT_ERR_UNSUPPORTED. */
int rt_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, double* out_rgb, rt_stats* stats);
/* the same for a host that owns a constructed Camera (its stored frame); rt_camera_frame_from = Camera::new (camera.rs:24-55) */
int rt_render_camera_frame(const rt_scene* s, const rt_camera_frame* frame, const rt_params* p, double* out_rgb, rt_stats* stats);
int rt_camera_frame_from(const rt_camera* cam, rt_camera_frame* out);

/* The reference's main.rs:52-54 as it really is: SPPMIntegrator::new(world) (photon_mapper.rs:139-233: `iterations` x
 * {photons_per_iter photon paths -> global + caustic photon maps; one eye ray per pixel; progressive radius update}) followed
 * by capture_image with SPPMIntegrator::sample_ray (photon_mapper.rs:327-365: the first Diffuse hit adds the pixel's estimates
 * and ends the path).  Needs rt_scene_set_lights with lights made by rt_object_*_light.  One GPU, whole frame:
 * p->world != 1 is RT_ERR_ARG.  Refusals, the first that applies: a background, area lights (RT_ERR_UNSUPPORTED), a scene without object lights: RT_ERR_ARG, the book-2 kinds, a light in a medium; the kernel's own (spp > 0) after the pre-pass.
 * stats_out (optional, HOST, height*width*10 f64): per pixel {global: flux[3], radius2, photons; caustic: flux[3], radius2, photons}.
 * spp == 0 runs the pre-pass only (out_rgb may be NULL).  rt_stats.reserved[0] = pre-pass time in microseconds. */
typedef struct rt_sppm_config {
    int32_t iterations;        /* max_iter_cnt      photon_mapper.rs:148  default 50     */
    int32_t photons_per_iter;  /* photon_per_iter   photon_mapper.rs:149  default 500000 */
    int32_t k_global;          /* GLOBAL_INIT_PHOTONS  :18  default 100 */
    int32_t k_caustic;         /* CAUSTIC_INIT_PHOTONS :19  default 50  */
    int32_t max_bounces;       /* cap on photon / eye path length (the reference loops until absorbed); default 4096 */
    int32_t reserved;
    double alpha;              /* ALPHA :17  default 0.7 */
} rt_sppm_config;
void rt_default_sppm_config(rt_sppm_config* c);
int rt_render_sppm(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_sppm_config* cfg, double* out_rgb,
                   double* stats_out, uint64_t photons_stored[2], rt_stats* stats);

/* Same, device-resident: renders this rank's 8x8 tiles into d_tiles (DEVICE memory,
 * rt_tiles_owned(p)*64*3 f64, tile-major) on `hip_stream` (hipStream_t as void*, NULL = default stream).
 * The call returns after the work has completed on that stream. */
int rt_render_tiles_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, double* d_tiles, void* hip_stream,
                           rt_stats* stats);
/* Resumable / progressive rendering (checkpoint and restart of a long frame).  capture_image adds a pixel's samples in index order
 * and divides once (camera.rs:96-102); here the running sums are the CALLER's: rt_render_accumulate_device traces the sample indices
 * [sample_begin, sample_end) of every pixel of this rank's tiles (0 <= begin < end <= p->spp) and adds them, in index order, to d_accum
 * (DEVICE memory, rt_tiles_owned(p)*64*3 f64; sample_begin == 0 initialises it, no zeroing needed); rt_accum_finalize_device writes
 * d_tiles = d_accum / p->spp (0 outside the image) as rt_render_tiles_device would have.  Calls with consecutive ranges, in order, give
 * that function's result bit for bit however the range is cut (the additions are the same sequence), so the state of an interrupted
 * frame is d_accum and the next sample index -- the RNG is keyed by (seed, pixel, sample) and has no state to save.  p must be the
 * same in every call (spp = the frame's total).  Kernels 1 / 2 / 5, integrators 0 / 1. */
int rt_render_accumulate_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, int32_t sample_begin, int32_t sample_end,
                                double* d_accum, void* hip_stream, rt_stats* stats);
int rt_accum_finalize_device(const rt_params* p, const double* d_accum, double* d_tiles, void* hip_stream);
/* The same for a host that holds no device memory (the reference's Rust host): the running sums travel in `accum_state`, HOST memory,
 * rt_accum_state_doubles(p) f64, opaque to the caller (it is this rank's tile-major accumulator) -- write it to disk to checkpoint, read it
 * back to resume.  rt_accum_finalize turns a complete state (all p->spp samples) into the frame out_rgb[H][W][3] that rt_render would
 * have returned (world == 1), bit for bit.  Each call copies the state to the device and back (24 B per pixel). */
int64_t rt_accum_state_doubles(const rt_params* p);
int rt_render_accumulate(const rt_scene* s, const rt_camera* cam, const rt_params* p, int32_t sample_begin, int32_t sample_end,
                         double* accum_state, rt_stats* stats);
int rt_accum_finalize(const rt_params* p, const double* accum_state, double* out_rgb);
/* SPPM across GPUs: every rank runs the same deterministic pre-pass (photon maps + per-pixel statistics of the WHOLE
 * frame: ~0.13 s for the reference's 50 x 500 000 photons) and renders only its own tiles; the buffers are gathered and
 * stitched exactly like rt_render_tiles_device's.  (The per-pixel pre-pass statistics are only returned by rt_render_sppm.) */
int rt_render_sppm_tiles_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_sppm_config* cfg, double* d_tiles,
                                void* hip_stream, rt_stats* stats);
int64_t rt_tiles_total(const rt_params* p);   /* ceil(W/8)*ceil(H/8) */
int64_t rt_tiles_owned(const rt_params* p);   /* tiles t in [0,total) with t % world == rank */
/* the stitch of camera.rs:115-123: scatter gathered tile-major buffers (rank-major: rank 0's tiles, rank 1's, ...
 * each padded to rt_tiles_owned of rank 0) into a row-major frame; both pointers DEVICE memory. */
int rt_assemble_frame_device(const rt_params* p, const double* d_gathered, int64_t tiles_per_rank_stride, double* d_frame,
                             void* hip_stream);

/* ---- the frame across the GPUs of one node ------------------------------------ */
/* Camera::capture_image as the reference structures it (camera.rs:74-126: the worker pool, the jobs, the channel and the stitch are
 * all INSIDE the call; main.rs:52-54 makes one call): one process, one host thread per logical rank.  The committed scene is
 * replicated on every device; rank i renders the 8x8 tiles t with t % n_devices == i on device_ids[i]; the ranks' tile-major rows
 * are gathered on device_ids[0] -- grouped ncclSend / ncclRecv over a communicator from ncclCommInitAll (RCCL, xGMI), cached per
 * device list for the life of the process; rows of ranks that share the root's device are rendered in place -- stitched there
 * (camera.rs:115-123) and copied once to out_rgb (HOST, height*width*3 f64).  The image is bit-identical to rt_render's for every
 * device list (the RNG is keyed by pixel and sample).
 *   device_ids: HIP ordinals, one per rank; an ordinal may repeat (its ranks share that device).  NULL = 0 .. n_devices-1.
 *   n_devices:  number of ranks; 0 = one per visible device.
 *   p->rank / p->world must be 0 / 1 (the call partitions the frame itself); p->device is ignored.
 *   stats:      NULL or n_devices entries, entry i = rank i's render (kernel_ms, samples, upload_ms, posted_ms ...).  stats[0].seconds = wall
 *               time of the whole call, stats[0].exchange_ms (= reserved[2] in microseconds) = from the last rank's finish until every row
 *               had arrived on the root device, stats[0].stitch_copy_ms = stitch + copy to the host, stats[0].comm_init_ms = creating the
 *               communicators (first call with a device list), stats[0].reserved[3] = number of rows that travelled through RCCL.
 *               A rank's rows are handed to RCCL (ncclSend on its device, the matching ncclRecv on the root's) by the rank's own host thread
 *               the moment its render has finished -- not after all ranks have joined -- so the rows of early ranks travel while the others
 *               still render.
 * Errors of any rank come back as that rank's rt_status (first failing rank wins); nothing aborts. */
int rt_render_multi(const rt_scene* s, const rt_camera* cam, const rt_params* p, int n_devices, const int* device_ids, double* out_rgb,
                    rt_stats* stats);
/* the same for a host that owns a constructed Camera (its stored frame, camera.rs:12-21), as rt_render_camera_frame */
int rt_render_multi_camera_frame(const rt_scene* s, const rt_camera_frame* frame, const rt_params* p, int n_devices, const int* device_ids,
                                 double* out_rgb, rt_stats* stats);
/* main.rs:52-54 as the reference really runs it, across GPUs: every rank repeats the deterministic SPPM pre-pass and renders its own
 * tiles (rt_render_sppm_tiles_device), gathered and stitched as above. */
int rt_render_sppm_multi(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_sppm_config* cfg, int n_devices,
                         const int* device_ids, double* out_rgb, rt_stats* stats);
/* ncclGetVersion of the RCCL the library is linked with (e.g. 22606), 0 if it cannot be asked */
int rt_rccl_version(void);

/* ---- guide buffers and denoising (no reference counterpart) ---------------------------------------------------------- */
/* First-hit guide buffers: for every pixel and sample s in [0, aov_spp) the camera ray rt_render draws -- stream (p->seed, pixel, s),
 * the same jitter and lens draws -- and its first hit World::hit(ray, p->t_min, +inf).  Averaged over the rays that hit, summed in
 * sample order in f64: out_aov[height][width][8] (HOST) = {normal[3] (the hit record's front-facing normal), t, albedo[3], coverage}.
 * The albedo is the material's texture value at (u, v, p): Lambertian / Metal albedo, Dielectric's texture, DiffuseLight's emit;
 * coverage = hits / aov_spp; a pixel without a hit is all zeros.  p->kernel 0 / 1 / 2 picks the walk as rt_render does (0: kernel 2's
 * when the scene has a usable accel); p->spp, max_depth, integrator and the shutter are not used.  Whole frames only: p->world > 1 or
 * p->rank != 0 is RT_ERR_ARG.  Scenes with a ConstantMedium (the first hit needs the path's stream) or moving spheres (no ray time) are
 * RT_ERR_UNSUPPORTED.  stats: seconds, kernel_ms, samples (= rays), kernel_used. */
int rt_render_aov(const rt_scene* s, const rt_camera* cam, const rt_params* p, int32_t aov_spp, double* out_aov, rt_stats* stats);

/* Edge-aware a-trous wavelet filter: `iterations` passes of the 5x5 B3 kernel H = {3/8, 1/4, 1/16} at step 2^i, f64, one thread per
 * pixel.  For tap q = p + step (dx, dy) (dy, then dx, from -2 to 2; taps outside the image skipped), h = H[|dx|] H[|dy|], w = h at q == p
 * and otherwise w = h * wn * wz * wa * wl, left to right, a factor 1 when its guide is absent:
 *   wn = fmax(0, (nx nx' + ny ny') + nz nz') squared normal_power_log2 times        (guide: aov normal, guides bit 0)
 *   wz = 1 / (1 + |z_p - z_q| / (sigma_depth * step))                                (guide: aov t, guides bit 1)
 *   wa = 1 / (1 + ((|dr| + |dg|) + |db|) / sigma_albedo)                              (guide: aov albedo, guides bit 2)
 *   wl = 1 / (1 + |l_p - l_q| / (sigma_luma * sqrt(v_p) + eps)), l = (0.2126 r + 0.7152 g) + 0.0722 b   (guide: variance)
 * W += w, C += w c_q, V += (w w) v_q; c'_p = C / W, v'_p = V / (W W).  Only + - * / sqrt fmax: the result is restated bit for bit by
 * tests/denoise_ref.py.  Every value of a bad config is RT_ERR_ARG. */
typedef struct rt_denoise_config {
    int32_t iterations;         /* passes, 1..8; default 5 */
    int32_t normal_power_log2;  /* wn = max(0, n.n')^(2^k), 0..16; default 7 */
    double sigma_depth;         /* > 0; default 1 (scene units per pixel of step) */
    double sigma_albedo;        /* > 0; default 0.1 */
    double sigma_luma;          /* > 0; default 4 (standard deviations of the pixel's mean luminance) */
    double eps;                 /* > 0; default 1e-10 */
    int32_t guides;             /* which aov guides weigh the taps: bit 0 normal, 1 depth, 2 albedo; default 7 (all); unused without aov */
    int32_t reserved[5];        /* must be 0 */
} rt_denoise_config;
void rt_default_denoise_config(rt_denoise_config* c);
/* rgb[height][width][3]; variance[height][width] (NULL: wl = 1): the variance of each pixel's mean luminance; aov[height][width][8] as
 * rt_render_aov writes it (NULL: no guides); out_rgb[height][width][3]; out_variance[height][width] (NULL: not returned; needs
 * variance).  HOST memory; outputs must not be inputs. */
int rt_denoise(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* rgb, const double* variance, const double* aov,
               double* out_rgb, double* out_variance);
/* the same on DEVICE memory of the current device, queued on `hip_stream` (hipStream_t as void*, NULL = default stream); returns after
 * the work has completed on that stream */
int rt_denoise_device(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* d_rgb, const double* d_variance,
                      const double* d_aov, double* d_out_rgb, double* d_out_variance, void* hip_stream);
/* The energy-preserving mode: rt_denoise / rt_denoise_device with a SYMMETRIC luminance stop.  Same arguments, same rt_denoise_config;
 * one term differs.  For a tap q != p
 *   wl = 1 / (1 + |l_p - l_q| / (sigma_luma * sqrt(v_p + v_q) + eps))
 * with v_p and v_q the variance input of THIS pass at the centre and at the tap (the caller's on the first pass, the propagated
 * V / (W W) afterwards).  Everything else is rt_denoise's bit for bit (tap order, h, wn, wz, wa, the product h * wn * wz * wa * wl, W, C,
 * V += (w w) v_q, the divisions, the ping-pong frames); tests/denoise_sym_ref.py restates it.  The weight p gives q is the weight q gives
 * p, so a bright pixel among dark ones with v = 0 is neither averaged down by them nor rejected by them, and the frame keeps its mean
 * (DESIGN.md s4e has the measurements).  variance == NULL is RT_ERR_ARG (without a variance the call would be rt_denoise); all of
 * rt_denoise's other argument errors are kept. */
int rt_denoise_sym(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* rgb, const double* variance, const double* aov,
                   double* out_rgb, double* out_variance);
int rt_denoise_sym_device(const rt_denoise_config* cfg, int32_t width, int32_t height, const double* d_rgb, const double* d_variance,
                          const double* d_aov, double* d_out_rgb, double* d_out_variance, void* hip_stream);

/* One call from scene to clean frame, on one device (p->world 1, p->rank 0, p->device picks it); nothing but the requested outputs
 * leaves the device.  p->spp must be even and >= 2.
 *   noisy     the samples [0, spp/2) and [spp/2, spp) go into ONE accumulator through the resumable path (rt_render_accumulate_device), so
 *             out_noisy is rt_render's frame bit for bit;
 *   variance  with h = spp / 2, S_h the sums after the first range and S the sums after both: per channel A = S_h / h, B = (S - S_h) / h,
 *             l = (0.2126 r + 0.7152 g) + 0.0722 b, variance = ((l_A - l_B) * (l_A - l_B)) / 4.0 -- of the pixel's mean luminance;
 *   guides    aov_spp > 0: rt_render_aov with p's seed and t_min; the walk is p->kernel when that is 1 or 2, otherwise automatic.
 *             aov_spp == 0: no guides, the filter runs on colour and variance alone (scenes with media or moving spheres);
 *   filter    rt_denoise (luma_mode 0) or rt_denoise_sym (luma_mode 1) over noisy, variance and the guides, under cfg (NULL =
 *             rt_default_denoise_config).
 * out_rgb[H][W][3] (required) = the filtered frame; out_noisy[H][W][3], out_variance[H][W], out_aov[H][W][8] may be NULL; HOST memory.
 * RT_ERR_ARG, before the device is touched: a null s, cam, p or out_rgb; spp odd or below 2; p->world != 1 or p->rank != 0; luma_mode
 * outside 0..1; aov_spp < 0; out_aov with aov_spp == 0; a config rt_denoise refuses; params rt_render refuses.  After that the call
 * returns what rt_render_accumulate_device and rt_render_aov return: kernel 6 and integrator 2 are RT_ERR_UNSUPPORTED, and so is
 * aov_spp > 0 on a scene with media or moving spheres.  stats: seconds = the call's wall time; kernel_ms, launches and samples summed
 * over the two render ranges; the rest from the first range. */
int rt_denoised_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* cfg, int32_t luma_mode,
                       int32_t aov_spp, double* out_rgb, double* out_noisy, double* out_variance, double* out_aov, rt_stats* stats);
/* the same with the outputs in DEVICE memory of the call's device, the work queued on `hip_stream` (hipStream_t as void*, NULL = default
 * stream); returns after the work has completed on that stream */
int rt_denoised_render_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* cfg, int32_t luma_mode,
                              int32_t aov_spp, double* d_out_rgb, double* d_out_noisy, double* d_out_variance, double* d_out_aov,
                              void* hip_stream, rt_stats* stats);

/* ---- ambient occlusion (no reference counterpart) -------------------------------------------------------------------- */
/* Ambient occlusion / sky visibility, a bent normal and the ambient term lit by the scene's background, on one device (p->world 1,
 * p->rank 0, p->device picks it); the pass generates its own rays.  Read from p: width, height, seed, t_min, kernel (0 / 1 / 2, as
 * rt_render_aov), device; everything else in p is ignored.  All arithmetic is f64 without contraction.
 *   camera ray   for pixel pix = y * width + x and sample s in [0, ao_spp): rt_render's sample s -- stream (p->seed, pix, s), the same
 *                jitter and lens draws -- and its first hit World::hit(ray, p->t_min, +inf).  A miss contributes nothing; a hit gives
 *                its point P and the record's front-facing normal n.
 *   occlusion    for each hit and k in [0, K), K = rays_per_hit: a fresh stream (p->seed XOR 0x9E3779B97F4A7C15, pix, s * K + k);
 *                u = unit(random_in_unit_sphere(stream)) as a Lambertian scatters; v = n + u, v = n where near_zero(v); d = unit(v)
 *                (cosine-distributed around n).  The ray is OCCLUDED iff World::hit(Ray(P, d), p->t_min, max_distance) returns a hit:
 *                every surface occludes (lights, glass, emitters); an occluder farther than max_distance does not count.
 *   sums         in (s, k) order from 0.0; hits = camera rays that hit, N = hits * K.
 * out_ao[height][width][8] (HOST) = {visibility = unoccluded / N, bent[3] = (sum over unoccluded rays of d) / N (not renormalised: its
 * length tells how open the cone is), ambient[3] = (sum over unoccluded rays of B(d)) / N with B what shades a miss (rt_scene_set_background;
 * exactly 0 where the scene has none), coverage = hits / ao_spp}; a pixel without a hit is eight zeros.  The result does not depend on
 * the walk or the launch shape; tests/ao_ref.py restates it over the oracle.
 * Checked before the device is touched: RT_ERR_ARG (a null s, cam, p, cfg or output; width / height < 1; p->world != 1 or p->rank != 0; a
 * kernel outside 0..2; a config value outside its range; reserved != 0), RT_ERR_NOT_COMMITTED, RT_ERR_UNSUPPORTED (a scene with a
 * ConstantMedium or moving spheres, as rt_render_aov; kernel 2 without a usable accel: no accel, t_min < 0, the camera farther from the
 * origin than the scene's origin bound, stacks larger than LDS) -- then RT_ERR_NO_DEVICE without a GPU.
 * stats: seconds, kernel_ms, launches (1), upload_ms, samples (= width * height * ao_spp), kernel_used (1 or 2), block_threads,
 * grid_blocks, scene_bytes. */
typedef struct rt_ao_config {
    int32_t ao_spp;        /* camera rays per pixel, 1..4096; default 4 */
    int32_t rays_per_hit;  /* K: occlusion rays per camera-ray hit, 1..256; default 4 */
    double max_distance;   /* > 0, +inf allowed (the default): an occluder farther away does not count */
    int32_t reserved[4];   /* must be 0 */
} rt_ao_config;
void rt_default_ao_config(rt_ao_config* c);
int rt_ao_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_ao_config* cfg, double* out_ao, rt_stats* stats);
/* the same with d_out_ao in DEVICE memory of the call's device, the kernel launched on `hip_stream` (hipStream_t as void*, NULL =
 * default stream); returns after the work has completed on that stream */
int rt_ao_render_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_ao_config* cfg, double* d_out_ao,
                        void* hip_stream, rt_stats* stats);

/* ---- tile-adaptive sampling (no reference counterpart) ------------------------------------------------------------ */
/* A whole frame on one device (p->world 1, p->rank 0, p->device picks it) in which every 8x8 tile T gets its own sample count n_T.  With
 * h = min_spp / 2 the passes trace the sample ranges [0, h), [h, 2h), [2h, 4h), [4h, 8h), ..., each capped at p->spp (the last one is
 * [n, p->spp)), over the tiles still active, all of them over the same range (the resumable path: the RNG is keyed by (seed, pixel,
 * sample)).  After a pass that ends at n = 2m < p->spp every active tile is tested: with S its running sums and S^m their snapshot at m,
 * the two-buffer error of Dammertz et al. (WSCG 2009) is, in f64 without contraction, for each in-image pixel of the tile in pixel index
 * order (row-major inside the tile):
 *   I_c = S_c / n, A_c = S^m_c / m (finalize's divisions), s = (I_r + I_g) + I_b,
 *   e_p = s > 0 ? ((|I_r - A_r| + |I_g - A_g|) + |I_b - A_b|) / sqrt(s) : 0,
 * e_T = the e_p added one at a time in that order from 0.0, divided by the tile's in-image pixel count.  The tile stops (n_T = n, for
 * good) when e_T < threshold -- a NaN error never stops a tile -- so n_T is one of {2h, 4h, ..., p->spp}.  out_rgb (HOST, [H][W][3]) =
 * S / n_T (0 outside the image); every tile is rt_render's frame at spp = n_T on that tile, bit for bit, and threshold 0 gives
 * rt_render's frame.  The result depends on no schedule knob (sub_spp, spp_chunk, job size).  out_tile_spp (HOST, [tiles_y][tiles_x],
 * or NULL) receives n_T.  Kernels 0 / 1 / 2 / 5 and integrators 0 / 1 (those of rt_render_accumulate_device); kernel 6 and integrator 2
 * are RT_ERR_UNSUPPORTED.  A bad config (min_spp odd, below 2 or above p->spp; threshold negative or NaN) or p->world != 1 is RT_ERR_ARG,
 * checked before the device.  stats: seconds; kernel_ms and launches summed over the passes; samples = the in-image pixel-samples
 * actually traced (the sum over tiles of n_T x in-image pixels); the rest from the first pass. */
typedef struct rt_adaptive_config {
    int32_t min_spp;   /* even, 2 <= min_spp <= p->spp: samples every tile gets before it may stop; default 16 */
    int32_t reserved;
    double threshold;  /* >= 0, not NaN: a tile stops once e_T < threshold; 0 = never stop (the frame is rt_render's); default 0.002 */
} rt_adaptive_config;
void rt_default_adaptive_config(rt_adaptive_config* c);
int rt_render_adaptive(const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_adaptive_config* cfg, double* out_rgb,
                       int32_t* out_tile_spp, rt_stats* stats);

/* ---- pixel regions of a frame (no reference counterpart: capture_image renders whole frames) ------------------------- */
/* A region is the pixel rectangle [x0, x1) x [y0, y1) of the p->width x p->height frame, y down.  rt_region_render traces all p->spp
 * samples of every pixel of every region and writes each region's linear radiance -- the running sum divided by spp exactly as rt_render
 * divides -- packed: region i is [y1 - y0][x1 - x0][3] f64, row-major, and starts behind regions 0 .. i-1; rt_region_doubles gives the
 * total, 3 x the sum of the areas.  Every value equals the same pixel of rt_render's frame for the same scene, camera and params, bit for bit
 * (the RNG is keyed by (seed, pixel, sample), the samples of a pixel are added in index order whatever else the launch renders).  Regions
 * may overlap, repeat, share tiles and come in any order: each gets its own copy of its pixels.
 *   cost      whole 8x8 tiles are traced: a call costs the tiles its regions touch (each once, however many regions touch it), in ONE launch
 *             over the sorted, unique list of those tiles (rt_region_tiles), so the launch depends on the SET of pixels asked for, not on
 *             how the caller cut it.  A pixel-exact lane mask is out of scope: a one-pixel region traces its tile's 64 pixels.
 *   supports  what rt_render_accumulate_device supports: kernels 0 / 1 / 2 / 5 and integrators 0 / 1, with rt_render's kernel choice, refusals
 *             and messages for media, the book-2 kinds, backgrounds, env sampling, area lights and nested Transforms; kernel 6 and
 *             integrator 2 are RT_ERR_UNSUPPORTED.
 *   errors    RT_ERR_ARG, before anything else: a null argument, params that rt_render refuses (size, spp, depth, kernel / integrator id,
 *             shutter), p->world != 1 or p->rank != 0, n_regions outside 1..65536, a region that breaks 0 <= x0 < x1 <= width or
 *             0 <= y0 < y1 <= height.  Then RT_ERR_UNSUPPORTED (kernel 6, integrator 2), RT_ERR_NOT_COMMITTED, RT_ERR_NO_DEVICE.
 *   stats     seconds = wall time of the call; samples = in-image pixels of the touched tiles x spp (what was really traced); kernel_ms,
 *             launches, kernel_used, scene_in_lds and the rest as rt_render reports them for its launch.
 * rt_region_doubles and rt_region_tiles are host only (no device needed) and check p and the regions as above; a bad argument returns a
 * negative rt_status.  rt_region_tiles lowers the regions to the launch's tile list -- image tiles ty * tiles_x + tx, ascending, unique --
 * writes min(capacity, N) ids and returns N; out_tiles may be NULL when capacity is 0.
 * rt_region_render writes HOST memory; rt_region_render_device DEVICE memory of the call's device (p->device, -1 = current), with the work
 * queued on `hip_stream` (hipStream_t as void*, NULL = default stream), and returns after it has completed there. */
typedef struct rt_region { int32_t x0, y0, x1, y1; } rt_region;
int64_t rt_region_doubles(const rt_params* p, int n_regions, const rt_region* regions);
int64_t rt_region_tiles(const rt_params* p, int n_regions, const rt_region* regions, int64_t capacity, int32_t* out_tiles);
int rt_region_render(const rt_scene* s, const rt_camera* cam, const rt_params* p, int n_regions, const rt_region* regions,
                     double* out_rgb, rt_stats* stats);
int rt_region_render_device(const rt_scene* s, const rt_camera* cam, const rt_params* p, int n_regions, const rt_region* regions,
                            double* d_out_rgb, void* hip_stream, rt_stats* stats);

/* From<Vec3> for Rgb<u8> (vec3.rs:223-231): floor(clamp(sqrt(c),0,1)*255), NaN -> 0.  Host buffers. */
int rt_tonemap_u8(const double* rgb, size_t n_channels, uint8_t* out);
/* RgbImage::save("output/test.png") (main.rs:55): 8-bit RGB PNG */
int rt_write_png(const char* path, int width, int height, const uint8_t* rgb);

/* ---- diagnostics used by the parity tests ------------------------------- */
/* rtamd-rng-3 (csrc/common/rng.h): first n u64 draws of stream (seed, pixel, sample) computed ON THE DEVICE */
int rt_debug_rng_device(uint64_t seed, uint64_t pixel, uint64_t sample, int n, uint64_t* out_host);
/* host-side restatement of the same stream (used by BVHNode::new's axis draws) */
int rt_debug_rng_host(uint64_t seed, uint64_t pixel, uint64_t sample, int n, uint64_t* out_host);
/* the float conversions of the spec (rand 0.8.4's): out_gen[i] = the i-th gen::<f64>() of a fresh stream (seed, pixel, sample),
 * out_range[i] = the i-th gen_range(lo..hi) of another fresh stream of the same key; on_device != 0 computes them in a kernel */
int rt_debug_rng_floats(uint64_t seed, uint64_t pixel, uint64_t sample, int n, double lo, double hi, int on_device, double* out_gen,
                        double* out_range);
/* device f64 sqrt / divide / rtamd-ln-1 / rtamd-sin-1, element-wise: op 0 = sqrt(a), 1 = a/b, 2 = det_ln(a), 3 = det_sin(a), 4 = sqrt_hot(a) (the item step's sqrt, 64 consecutive elements a wave; op 0's bits) */
int rt_debug_math_device(int op, size_t n, const double* a_host, const double* b_host, double* out_host);
/* closest hit of explicit world-space rays through device traversal `kernel` (1, 2, or 3 = kernel 2's LDS node table "NodeW" with
 * its own box test, which pt_kernel uses when the scene is LDS-resident; 5 / 6 = the walks of the instance service in one lane: the
 * world-space walk with the large instances deferred, then their object-space walks over the Node2 / item records (5: the in-lane
 * fallback of kernel 5) or over the compact NodeQ / Tri32 copies (6: what the serving waves of kernels 5 / 6 walk), with the exact-tie rule;
 * 7 = 3 with the table's boxes tightened as a render tightens them, for the origin bound 2 * max(scene extent, largest |origin coordinate| of
 * this batch); a scene with instances keeps the stored boxes, as in a render; 8 = 3 begun at the root's dominant leaf child where csrc/common/walk_start.h finds one, as pt_kernel's sphere-only LDS variants begin, RT_ERR_UNSUPPORTED with nested Transforms): rays n*6 (orig,dir);
 * out n*12 = {hit, t, p[3], normal[3], front_face, u, v, leaf index in the reference-order program}.
 * RT_ERR_UNSUPPORTED: a scene with moving spheres or a ConstantMedium (rt_debug_walk_device asks those); a kernel other than 1 on a scene
 * without an accel; kernels 5 / 6 on a scene without 1..64 instances of which one holds only f32-vertex triangles (so on every scene with
 * nested Transforms). */
int rt_debug_hit_device(const rt_scene* s, int kernel, size_t n, const double* rays_host, double t_min, double t_max, double* out_host);
/* the per-tile job sequence of one launch over samples [s_begin, s_end) for a rank that owns `tiles_owned` tiles on a GPU with `n_waves`
 * resident waves (host logic only, no device needed): out[25] = 5 rows {first round, first unit, first sample, samples per unit, units per
 * job}, one per level of decreasing unit / job size, the row behind the last level = {rounds, units, s_end, 0, 0}.  Every tile's samples
 * are cut the same way; jobs are dealt round by round, so the small jobs of the last levels are what runs when the queue runs dry.
 * Returns the number of rounds (jobs per tile) or a negative rt_status. */
int rt_debug_schedule(int64_t tiles_owned, int n_waves, int s_begin, int s_end, int sub_spp, int job_units, int* out25);
/* env sampling diagnostics on HIP device `device` (a committed scene with env sampling enabled; RT_ERR_NO_DEVICE without a GPU).
 * table: the resolved size and, where q_host is not NULL, the h*w quantised weights q (row j = v cell j) as that device built them.
 * sample: n draws from xi4_host (n*4: xi1..xi4) -> out_host n*4 = {d[3], pdf(d)}.  pdf: n directions (n*3) -> n pdfs.  A table whose
 * total is 0 returns zeros from both. */
int rt_debug_env_table_device(const rt_scene* s, int device, int* w, int* h, uint32_t* q_host);
int rt_debug_env_sample_device(const rt_scene* s, int device, size_t n, const double* xi4_host, double* out_host);
int rt_debug_env_pdf_device(const rt_scene* s, int device, size_t n, const double* dirs_host, double* pdf_host);
/* area light diagnostics on HIP device `device` (a committed scene with area lights; RT_ERR_NO_DEVICE without a GPU).
 * sample: in_host n*7 = {o[3], xi0, xi1, xi2, xi3}: xi0 picks one of the M area lights by the mixture's clamped product (uint32)(xi0 * M),
 * xi1..xi3 are the three draws -> out_host n*4 = {dir[3], pdf}.  pdf: rays_host n*6 = {o[3], d[3]} -> n pdfs.  Both pdfs are the sum of the
 * pdfs of all M area lights, in list order from 0.0 (not divided by M). */
int rt_debug_area_sample_device(const rt_scene* s, int device, size_t n, const double* in_host, double* out_host);
int rt_debug_area_pdf_device(const rt_scene* s, int device, size_t n, const double* rays_host, double* pdf_host);
/* shading and object-light diagnostics on HIP device `device`: what a path does after its hit, on explicit inputs, through the very
 * functions the render kernels call.  The arguments are checked on the host first -- RT_ERR_ARG (a null pointer, n == 0, a material or
 * light index that is not an integer of the scene's range), RT_ERR_NOT_COMMITTED -- then RT_ERR_NO_DEVICE without a GPU.  Every row has
 * its own random stream, keys_host n*3 = {seed, pixel, sample} as uint64, and its own unit-zero status (1.0: some unit() met a vector of
 * length 0; the row's other outputs are then what the arithmetic gave).  "next draw" = the two 32-bit halves {upper, lower} of the
 * stream's next u64 after the call, as exact doubles: its index in rt_debug_rng_host's stream is the number of draws the call consumed.
 * shade: emitted + scatter of material `mat` at an explicit hit record, texture lookup included (the noise-texture form where the scene
 *   has a noise texture, as a render chooses).  in_host n*17 = {mat, mix, ray origin[3], ray direction[3], p[3], normal[3], front_face, u, v}
 *   (the ray origin is carried for the oracle's Ray and not read); out_host n*22 = {scattered (0: Absorb), diffuse, out_dir[3], att[3],
 *   emitted[3], mixed, continued, beta[3], dir[3], unit-zero status, next draw[2]}.  Where mix != 0 and the interaction is Diffuse, the
 *   plain mixture step of integrator 1 follows (mixed = 1): continued = its weight is > 0, beta = the weight times att started from
 *   (1, 1, 1) (left at that where not continued), dir = the direction it settled on; elsewhere mixed = continued = 0, beta = (1, 1, 1),
 *   dir = out_dir.  out_dir is (0, 0, 0) on Absorb.  mix needs object lights and a scene without env sampling and area lights (RT_ERR_ARG).
 * light sample: light_random of object light `light` (index into rt_scene_set_lights' list) seen from o: in_host n*4 = {o[3], light};
 *   out_host n*6 = {dir[3], unit-zero status, next draw[2]}.
 * light pdf: rays_host n*6 = {o[3], d[3]} -> pdf_host n*L: the pdf of EACH of the scene's L object lights for the ray, in list order
 *   (the mixture adds them in that order from 0.0 and divides by L).
 * Noise: the lattice index of a Perlin octave is floor(x) mod 256 of the mathematical integer, 0..255, for every finite coordinate x
 * (computed as fx - 256 floor(fx / 256), exact in f64: no conversion leaves the range of int; every |x| >= 2^60 has index 0); a
 * non-finite coordinate has index 0 (and the texture's value is then 0.5, through rtamd-sin-1 of a NaN). */
int rt_debug_shade_device(const rt_scene* s, int device, size_t n, const double* in_host, const uint64_t* keys_host, double* out_host);
int rt_debug_light_sample_device(const rt_scene* s, int device, size_t n, const double* in_host, const uint64_t* keys_host, double* out_host);
int rt_debug_light_pdf_device(const rt_scene* s, int device, size_t n, const double* rays_host, double* pdf_host);
/* closest hit of explicit rays that carry what a path's segment carries: a ray time and a random stream.  This is the closest-hit
 * diagnostic for scenes with a ConstantMedium (whose hit draws from the path's stream) or a moving sphere (whose centre depends on the
 * ray's time), both of which rt_debug_hit_device refuses; any other committed scene is accepted too and then draws nothing.
 *   rays_host n*7 = {origin[3], direction[3], time}; keys_host n*3 = {seed, pixel, sample} as uint64: row i walks with a fresh stream of
 *   its own key.  t_max is +inf, as in a render.
 *   kernel 1: the reference-order program (traverse), 2: the accel walk over the node array in global memory, 3: the same walk over the
 *   LDS node table "NodeW" with the stored pads (rt_debug_hit_device's mode 3).  The GENERAL / MEDIA variant of each walk is the one a
 *   render with integrator 0 and a closed shutter launches for the scene (spheres only, general, book 2, nested chains).
 *   out_host n*14 = rt_debug_hit_device's 12 fields {hit, t, p[3], normal[3], front_face, u, v, leaf index in the reference-order
 *   program}, all zero on a miss, then "next draw" = the two 32-bit halves {upper, lower} of the stream's next u64 after the walk, as
 *   exact doubles (as rt_debug_shade_device reports it): its index in rt_debug_rng_host's stream is the number of draws the walk
 *   consumed -- at most one per ConstantMedium the ray crosses, none in a scene without media.  A medium's hit is materialised as a
 *   render's: outward normal (1, 0, 0), u = v = 0, leaf index = the medium's closing node.
 * Checked on the host first: RT_ERR_ARG (a null pointer, n == 0, a kernel outside 1..3, a time that is not finite, a time outside
 * [time0, time1] of any moving sphere of the scene -- the rule of a render's shutter: their boxes are built for that range),
 * RT_ERR_NOT_COMMITTED, RT_ERR_UNSUPPORTED (kernel 2 or 3 on a scene without an accel or with t_min < 0; stacks or a NodeW table that
 * do not fit in LDS) -- then RT_ERR_NO_DEVICE without a GPU.  Returns RT_ERR_UNIT_ZERO where the record of some row took unit() of a vector of
 * length 0 (as a render of that hit would); every output is then still written, with what the arithmetic gave.  The accel walks are exact for origins within the scene's origin bound, as
 * in a render (64 times its extent). */
int rt_debug_walk_device(const rt_scene* s, int device, int kernel, size_t n, const double* rays_host, const uint64_t* keys_host, double t_min,
                         double* out_host);
/* any-hit of explicit rays, through the device function rt_ao_render's occlusion rays take: "would World::hit(ray, t_min, t_max) return
 * a hit", answered at the first primitive whose own test accepts a t in the range (no record, no tie rule); an acceptance at an end of the
 * range, where World::hit's own box tests may cull the primitive (t_max = the distance of a cube face), is settled by the reference-order walk.
 *   rays_host n*7 = {origin[3], direction[3], t_max} (every row its own t_max, +inf allowed); out_host n doubles, 1.0 = occluded, 0.0 = not.
 *   kernel 1: the reference-order program, 2: the accel walk over the node array in global memory (nested chains where the scene has any).
 * Checked on the host first: RT_ERR_ARG (a null pointer, n == 0, a kernel outside 1..2), RT_ERR_NOT_COMMITTED, RT_ERR_UNSUPPORTED (a
 * scene with a ConstantMedium or moving spheres; kernel 2 on a scene without an accel, with t_min < 0 or with stacks that do not fit in
 * LDS) -- then RT_ERR_NO_DEVICE without a GPU.  The accel walk is exact for origins within the scene's origin bound, as in a render (64
 * times its extent). */
int rt_debug_occluded_device(const rt_scene* s, int device, int kernel, size_t n, const double* rays_host, double t_min, double* out_host);
/* SPPM photon gather diagnostics: ONE iteration of the render's own gather on explicit inputs (host buffers throughout) -- the grid
 * build and the sort of both photon maps, gather_kernel (four waves per block, one gather point per wave, caustic map first, then
 * global) and estimate_kernel, launched as rt_render_sppm launches them.  No scene is involved.
 *   global / caustic: the two photon maps, n * 9 doubles {position[3], power[3], norm[3]} each; either n may be 0 (its pointer is then
 *     not read).  At most 2^30 photons per map.
 *   points: m * 7 doubles {valid, p[3], bsdf[3]}; a row with valid == 0 is skipped and its statistics stay as they came.
 *   stats: m * 10 doubles {global[5], caustic[5]}, each map {flux[3], radius2, photons} -- IN: the state before this iteration (all zeros
 *     before the first), OUT: the state after it.  The caller carries it from call to call, each with that iteration's photon maps.
 *   k_global, k_caustic, alpha: as in rt_sppm_config.  shift: the S of the 2^-S fixed-point flux accumulators, 0..60.  CONTRACT: every
 *     photon's term bsdf * power * (1 - disk factor) has |term| * 2^S < 2^52 per channel (rt_render_sppm chooses S from the lights'
 *     power so that this holds), and the int64 sum of one query's terms does not overflow.  term * 2^S is rounded to the nearest
 *     integer, ties to even.
 *   n_emitted: the N of flux / (pi * radius2 * N).  estimates: OUT m * 6 doubles {caustic[3], global[3]} for EVERY row (0 / 0 = NaN where
 *     radius2 == 0).
 *   grid_global, grid_caustic: OUT what the grid over each map came out as.  Where cell_start / index are not NULL they receive the
 *     dim[0] * dim[1] * dim[2] + 1 cell offsets (cell c = (z * dim[1] + y) * dim[0] + x holds index[cell_start[c] .. cell_start[c + 1]))
 *     and the n photon indices grouped by cell; *_capacity are the entries the buffers hold (RT_ERR_ARG where that is too few:
 *     rt_debug_grid_shape gives the number of cells beforehand).  A map with n == 0 has no grid: lo = 0, cell = 1, dim = 1, no buffer written.
 * Honours rt_tuning.sppm_knn_candidates as rt_render_sppm does.  The arguments are checked on the host first -- RT_ERR_ARG for a null
 * pointer, m == 0, k < 1, !(alpha > 0), S outside 0..60 -- then RT_ERR_NO_DEVICE without a GPU.  A photon position that is not finite
 * is RT_ERR_UNSUPPORTED.  Returns RT_ERR_UNIT_ZERO where some gather point lies exactly on a photon it visits (as rt_render_sppm does);
 * every output is then still written, with what the arithmetic gave. */
typedef struct rt_debug_grid {
    double lo[3];               /* the grid's origin: the least photon coordinate per axis */
    double cell;                /* the edge of a cell */
    int32_t dim[3];             /* cells per axis, 1..161 */
    int32_t reserved;
    uint32_t* cell_start;       /* NULL, or cell_start_capacity entries */
    uint32_t* index;            /* NULL, or index_capacity entries */
    uint64_t cell_start_capacity, index_capacity;
} rt_debug_grid;
typedef struct rt_debug_sppm_gather {
    uint64_t n_global, n_caustic, m;
    const double* global;
    const double* caustic;
    const double* points;
    double* stats;
    double* estimates;
    int32_t k_global, k_caustic;
    double alpha;
    int32_t shift;                 /* S */
    int32_t reserved;
    double n_emitted;
    rt_debug_grid grid_global, grid_caustic;
} rt_debug_sppm_gather;
int rt_debug_sppm_gather_device(int device, rt_debug_sppm_gather* io);
/* SPPM trace diagnostics: the photon pass and the eye pass of ONE iteration of rt_render_sppm's pre-pass on a committed scene, and what
 * they wrote (host buffers throughout).  The entry goes through the code rt_render_sppm itself runs for the light table (cumulative
 * weights, flux, scale, S), for the choice of the compiled photon / eye kernel and its launch shape, for the launches and for the
 * grow-and-retry of the photon stores; only the two-stream overlap of iterations is the render's alone.  The gather is not run
 * (rt_debug_sppm_gather_device takes what this entry returns).
 *   IN   width, height (each >= 2: the eye pass divides by width - 1 and height - 1), seed (rt_params.seed), iteration >= 0 (photon i of
 *        the pass is photon iteration * photons_per_iter + i of the run, a 64-bit index; the eye stream of a pixel is keyed by the
 *        iteration), photons_per_iter >= 1, max_bounces >= 1 (rt_sppm_config's).
 *        capacity_global, capacity_caustic: the photons the two DEVICE stores hold at the first launch, 0 = the render's 8 P + 1024 and
 *        2 P + 1024; a non-zero rt_tuning.sppm_photon_capacity overrides both, as in a render.  A store that overflows is grown to
 *        max(photons + 1024, 2 x capacity) and the pass repeated (it is deterministic).
 *        global, caustic: NULL, or host buffers of global_rows / caustic_rows rows of 9 doubles.  The photon pass runs unless BOTH are
 *        NULL; a map whose pointer is NULL is counted and not copied.  points: NULL (the eye pass is skipped), or width * height * 7 doubles.
 *   OUT  the two maps as n * 9 doubles {position[3], power[3], norm[3]} (rt_debug_sppm_gather's layout) in the order the device stored
 *        them, which is arbitrary; n_global, n_caustic: their photons -- also written where a host buffer holds fewer rows, which is
 *        RT_ERR_ARG with neither map copied, so that a second call can be sized.
 *        points: per pixel y * width + x {valid, p[3], bsdf[3]}; the device buffer is zeroed before the eye kernel runs, so a row with
 *        valid == 0 is all zeros (the kernel writes only its first word there).
 *        shift: the S of the fixed-point flux accumulators, as the render takes it from the lights.  photon_launches: how often the
 *        photon pass was launched (1 + the retries; 0 where it was skipped).  variant: bit 0 the accel walk, bit 1 the accel's hot tables
 *        staged in LDS (photon pass only), bit 2 the chain walk of nested Transforms, bit 3 the MEDIA kernels -- photon_kernel<ACCEL, LDS>,
 *        photon_kernel_nest, eye_kernel<ACCEL>, eye_kernel_nest and their _media twins.
 * Checked on the host first: RT_ERR_ARG (a null argument, a size, count, cap or iteration out of range, rows without a buffer),
 * then what rt_render_sppm refuses, with its codes: RT_ERR_NOT_COMMITTED, RT_ERR_UNSUPPORTED (a background, area lights, moving spheres, noise
 * textures, a light inside a ConstantMedium), RT_ERR_ARG (no lights) -- then RT_ERR_NO_DEVICE without a GPU.  Honours rt_tuning.no_lds.
 * Returns RT_ERR_UNIT_ZERO where a unit() of either pass met a zero vector (as rt_render_sppm does); every output is then still written,
 * with what the arithmetic gave (the photon pass is not repeated after it: a store that overflowed in the same launch is cut at its capacity). */
typedef struct rt_debug_sppm_trace {
    int32_t width, height;
    int32_t iteration, photons_per_iter, max_bounces;
    int32_t reserved;
    uint64_t seed;
    uint32_t capacity_global, capacity_caustic;
    double* global;
    double* caustic;
    uint64_t global_rows, caustic_rows;
    double* points;
    uint64_t n_global, n_caustic;     /* OUT */
    int32_t shift;                    /* OUT: S */
    int32_t photon_launches;          /* OUT */
    uint32_t variant;                 /* OUT */
    uint32_t reserved2;
} rt_debug_sppm_trace;
int rt_debug_sppm_trace_device(const rt_scene* s, const rt_camera* cam, int device, rt_debug_sppm_trace* io);
/* the shape build_grid gives the uniform grid over n photons whose bounding box is [lo3, hi3] (host logic only, no device needed):
 * cell = 2 * sqrt(area / n) of the box's surface area, not below longest extent / 160; dim = floor(extent / cell) + 1 per axis, 1..161.
 * Fallbacks: a box without area (a line or a point) takes cell = its longest extent, a point cell = 1; n == 0 gives cell = 1, dim = 1.
 * RT_ERR_UNSUPPORTED where an extent is negative or not finite. */
int rt_debug_grid_shape(const double* lo3, const double* hi3, uint64_t n, double* cell, int32_t* dim3);

/* ---- temporal accumulation across camera frames (no reference counterpart) ------------------------------------------- */
/* One step of temporal accumulation with reprojection: the current frame is blended into a history that the previous frame left, each
 * pixel fetching its history from where its first hit was on screen under the previous camera.  A scene is immutable after
 * rt_scene_commit, so only the camera moves between frames and the reprojection of a diffuse surface is exact.  f64, one thread per
 * pixel, no contraction; only + - * / floor fmin fmax fabs and comparisons, in the order written here: tests/temporal_ref.py restates
 * the step bit for bit.
 *   buffers  rgb[H][W][3]; aov[H][W][8] as rt_render_aov writes it = {normal[3], t, albedo[3], coverage}; variance[H][W] = the variance
 *            of the pixel's mean luminance as rt_denoised_render returns it (may be NULL); history[H][W][6] = {r, g, b, m1, m2, n}: the
 *            accumulated colour, the first and second moment of the luminance, the history length (an integer-valued double);
 *            out_variance[H][W] (may be NULL).  prev_history, prev_aov and cam_prev are all given or all NULL (the first frame).
 *            Outputs must not be inputs.
 *   helpers  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);
 *            l = (0.2126 r + 0.7152 g) + 0.0722 b; centre(cam, x, y, t): u = ((double)x + 0.5) / (double)(W - 1),
 *            v = ((double)y + 0.5) / (double)(H - 1), st = 1.0 - v, d = ((llc + hor u) + ver st) - origin, P = origin + d t.  Of an
 *            rt_camera_frame only origin, lower_left_corner, horizontal and vertical are read: the lens is ignored (t is the guides'
 *            mean parameter along the pixel's rays).
 *   rule     per pixel (x, y); "reset" means out = {rgb, l, l l, 1.0}:
 *   1. reset when there is no previous frame or aov.coverage is not > 0 (pixels that see the background restart);
 *   2. P = centre(cur, x, y, aov.t), q = P - origin_prev, D0 = llc_prev - origin_prev, N0 = cross(hor_prev, ver_prev),
 *      s = dot(q, N0) / dot(D0, N0); reset unless s > 0 (a point behind the previous camera, NaN);
 *   3. r = q / s - D0, u' = dot(r, hor_prev) / dot(hor_prev, hor_prev), st' = dot(r, ver_prev) / dot(ver_prev, ver_prev),
 *      fx = u' (double)(W - 1) - 0.5, fy = (1.0 - st') (double)(H - 1) - 0.5; reset unless fx > -1.0 && fx < (double)W && fy > -1.0 &&
 *      fy < (double)H; only then x0 = floor(fx), y0 = floor(fy) become integers (in [-1, W - 1] and [-1, H - 1]);
 *   4. wx = fx - x0, wy = fy - y0, reach2 = dot(P - origin_cur, P - origin_cur).  The four bilinear taps (j, i) = (0,0), (0,1), (1,0),
 *      (1,1) at pixel (x0 + i, y0 + j) have the weight b = (i ? wx : 1.0 - wx) * (j ? wy : 1.0 - wy).  A tap is valid iff it lies inside
 *      the image, b > 0, its history n > 0, its prev_aov.coverage > 0, dn dn <= (plane_tolerance plane_tolerance) reach2 with
 *      Pq = centre(prev, xq, yq, prev_aov.t), e = Pq - P, dn = dot(e, normal_cur) (the tap's point lies near the pixel's tangent
 *      plane), dot(normal_cur, normal_q) >= normal_min and (|dr| + |dg|) + |db| <= albedo_tolerance of the guide albedos.  Valid taps
 *      add Wsum += b and A_c += b h_c for c = r, g, b, m1, m2, from 0.0 in tap order; nmin is the least n of the valid taps;
 *   5. reset unless Wsum >= min_weight; otherwise h = A / Wsum, n = fmin(nmin + 1.0, (double)max_history), a = fmax(alpha, 1.0 / n),
 *      out_c = (1.0 - a) h_c + a rgb_c, m1 = (1.0 - a) h_m1 + a l, m2 = (1.0 - a) h_m2 + a (l l);
 *   6. out_variance = Vf a (a = 1.0 on a reset), the variance of the accumulated mean luminance: Vf = variance[pix] where n < 4.0 and a
 *      variance was given (a short history has no temporal estimate), otherwise Vf = fmax(0.0, m2 - m1 m1).
 * Limits: background pixels restart; specular and glass surfaces reproject by their first hit; the lens is ignored; nothing in a scene
 * moves.  RT_ERR_ARG, before any device is touched: a null cfg, cam_cur, rgb, aov or out_history; width or height < 2; a config value
 * out of its range or NaN; reserved != 0; only some of cam_prev, prev_history, prev_aov; an output that is an input.  Then
 * RT_ERR_NO_DEVICE. */
typedef struct rt_temporal_config {
    double alpha;            /* 0..1: least weight of the new frame; 0 = plain running mean up to max_history; default 0.2 */
    double plane_tolerance;  /* > 0: a tap's point may lie this far from the pixel's tangent plane, relative to the pixel's distance from the camera; default 0.02 */
    double normal_min;       /* -1..1: least dot product of the two guide normals; default 0.9 */
    double albedo_tolerance; /* >= 0, +inf allowed: largest (|dr| + |dg|) + |db| of the guide albedos; default 0.25 */
    double min_weight;       /* > 0, <= 1: least sum of valid bilinear weights for a pixel to keep its history; default 0.25 */
    int32_t max_history;     /* 1..65536: cap of the history length; default 32 */
    int32_t reserved[5];     /* must be 0 */
} rt_temporal_config;
void rt_default_temporal_config(rt_temporal_config* c);
/* HOST memory */
int rt_temporal_accumulate(const rt_temporal_config* cfg, int32_t width, int32_t height, const rt_camera_frame* cam_prev,
                           const rt_camera_frame* cam_cur, const double* rgb, const double* aov, const double* variance,
                           const double* prev_history, const double* prev_aov, double* out_history, double* out_variance);
/* the same on DEVICE memory of the current device, queued on `hip_stream` (hipStream_t as void*, NULL = default stream); returns after
 * the work has completed on that stream */
int rt_temporal_accumulate_device(const rt_temporal_config* cfg, int32_t width, int32_t height, const rt_camera_frame* cam_prev,
                                  const rt_camera_frame* cam_cur, const double* d_rgb, const double* d_aov, const double* d_variance,
                                  const double* d_prev_history, const double* d_prev_aov, double* d_out_history, double* d_out_variance,
                                  void* hip_stream);

/* A device-resident sequence of frames of one width x height on one device (-1: the device current at the sequence's first frame): the history,
 * the previous frame's guides and the previous camera stay on the device between frames.  cfg NULL = rt_default_temporal_config.  One
 * thread uses a sequence at a time.  rt_sequence_frame renders one frame:
 *   A  rt_denoised_render's first three stages, unchanged: the noisy frame (rt_render's bits), the two-half variance, the guides;
 *   B  rt_temporal_accumulate with stage A's variance against the sequence's history (the first frame after a reset resets every pixel);
 *   C  luma_mode -1: out_rgb is the accumulated colour; 0 / 1: rt_denoise / rt_denoise_sym over (accumulated colour, stage B's variance,
 *      guides) under dn (NULL = rt_default_denoise_config).  The history keeps the unfiltered accumulation.
 * out_rgb[H][W][3] (required), out_accum[H][W][3], out_history[H][W][6], out_variance[H][W] (stage B's) may be NULL; HOST memory;
 * nothing else leaves the device.  p->seed is used as it is: a host that passes one seed for every frame repeats its noise (the bindings
 * default to base seed + frame index).  The sequence remembers rt_scene_fingerprint(s): a frame of another scene resets first.
 * RT_ERR_ARG, before the device: a null q, s, cam, p or out_rgb; p->width / p->height other than the sequence's; aov_spp < 1 (the step
 * needs guides); luma_mode outside -1..1; everything rt_denoised_render refuses as an argument.  Then what rt_denoised_render returns
 * for the scene (media and moving spheres: RT_ERR_UNSUPPORTED).  p->device is not read: the sequence's device is used.  stats as
 * rt_denoised_render's.  rt_sequence_create: RT_ERR_ARG for a null out, width or height < 2 or beyond 2^31 pixels, device < -1, a config
 * rt_temporal_accumulate refuses; no device is touched before the first frame. */
typedef struct rt_sequence rt_sequence;
int rt_sequence_create(int32_t width, int32_t height, int32_t device, const rt_temporal_config* cfg, rt_sequence** out);
void rt_sequence_destroy(rt_sequence* q);
int rt_sequence_reset(rt_sequence* q);          /* the next frame resets every pixel */
int rt_sequence_frames(const rt_sequence* q);   /* frames since the last reset; RT_ERR_ARG for NULL */
int rt_sequence_frame(rt_sequence* q, const rt_scene* s, const rt_camera* cam, const rt_params* p, const rt_denoise_config* dn,
                      int32_t luma_mode, int32_t aov_spp, double* out_rgb, double* out_accum, double* out_history, double* out_variance,
                      rt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* RTAMD_H */
