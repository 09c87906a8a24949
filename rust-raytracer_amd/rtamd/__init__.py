"""rtamd -- Python host binding of librtamd.so (the C ABI in include/rtamd.h).

Mirrors the reference's host-side interface for the radiance path (names follow
/root/reference/raytracer/src): World / Hitable constructors (Sphere, XYRectangle,
..., BVHNode, Transform, Mesh, Cube), Material / Texture constructors, Camera and
Camera.capture_image.  Everything here is plumbing over ctypes; all intersection
and shading happens in the HIP kernels.  There is no CPU fallback: rendering
without the built library or without a HIP device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("RTAMD_LIB") or os.path.join(_ROOT, "librtamd.so")  # RTAMD_LIB: A/B builds only

RT_OK = 0
ERR_NAMES = {
    -1: "RT_ERR_ARG", -2: "RT_ERR_UNIT_ZERO", -3: "RT_ERR_NO_BBOX", -4: "RT_ERR_SINGULAR", -5: "RT_ERR_IO",
    -6: "RT_ERR_SCHEMA", -7: "RT_ERR_NO_NORMALS", -8: "RT_ERR_NOT_COMMITTED", -9: "RT_ERR_NO_DEVICE",
    -10: "RT_ERR_UNSUPPORTED", -11: "RT_ERR_HIP", -12: "RT_ERR_INTERNAL",
}


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "RT_ERR"), code, msg))
        self.code = code


class rt_camera(C.Structure):
    _fields_ = [("look_from", C.c_double * 3), ("look_at", C.c_double * 3), ("vup", C.c_double * 3), ("vfov", C.c_double),
                ("aspect", C.c_double), ("aperture", C.c_double), ("focus_dist", C.c_double)]


class rt_camera_frame(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("lower_left_corner", C.c_double * 3), ("horizontal", C.c_double * 3),
                ("vertical", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3), ("w", C.c_double * 3), ("lens_radius", C.c_double)]


class rt_params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32), ("t_min", C.c_double),
                ("seed", C.c_uint64), ("rank", C.c_int32), ("world", C.c_int32), ("spp_chunk", C.c_int32), ("kernel", C.c_int32),
                ("device", C.c_int32), ("integrator", C.c_int32), ("time0", C.c_double), ("time1", C.c_double)]


class rt_stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("kernel_ms", C.c_double), ("reduce_ms", C.c_double), ("samples", C.c_uint64),
                ("launches", C.c_int32), ("kernel_used", C.c_int32), ("scene_in_lds", C.c_int32), ("block_threads", C.c_int32),
                ("grid_blocks", C.c_int32), ("spp_chunk", C.c_int32), ("scene_bytes", C.c_uint64), ("reserved", C.c_uint64 * 4),
                ("upload_ms", C.c_double), ("posted_ms", C.c_double), ("stitch_copy_ms", C.c_double), ("comm_init_ms", C.c_double),
                ("exchange_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["workspace_bytes"] = int(self.reserved[1])
        # rt_render on one device: how far kernel 2 moved the planes of its LDS node table inward for this render's ray origins (the f32's
        # bits; 0: the stored boxes).  rt_render_multi's entry 0 keeps its row count in the same word: read that as rows_through_rccl.
        d["box_shrink"] = float(np.uint32(self.reserved[3] & 0xFFFFFFFF).view(np.float32))
        return d


class rt_sppm_config(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("photons_per_iter", C.c_int32), ("k_global", C.c_int32), ("k_caustic", C.c_int32),
                ("max_bounces", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_double)]


class rt_debug_grid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("cell", C.c_double), ("dim", C.c_int32 * 3), ("reserved", C.c_int32),
                ("cell_start", C.POINTER(C.c_uint32)), ("index", C.POINTER(C.c_uint32)), ("cell_start_capacity", C.c_uint64),
                ("index_capacity", C.c_uint64)]


class rt_debug_sppm_gather(C.Structure):
    _fields_ = [("n_global", C.c_uint64), ("n_caustic", C.c_uint64), ("m", C.c_uint64), ("global_", C.POINTER(C.c_double)),
                ("caustic", C.POINTER(C.c_double)), ("points", C.POINTER(C.c_double)), ("stats", C.POINTER(C.c_double)),
                ("estimates", C.POINTER(C.c_double)), ("k_global", C.c_int32), ("k_caustic", C.c_int32), ("alpha", C.c_double),
                ("shift", C.c_int32), ("reserved", C.c_int32), ("n_emitted", C.c_double), ("grid_global", rt_debug_grid),
                ("grid_caustic", rt_debug_grid)]


class rt_debug_sppm_trace(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iteration", C.c_int32), ("photons_per_iter", C.c_int32),
                ("max_bounces", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("capacity_global", C.c_uint32),
                ("capacity_caustic", C.c_uint32), ("global_", C.POINTER(C.c_double)), ("caustic", C.POINTER(C.c_double)),
                ("global_rows", C.c_uint64), ("caustic_rows", C.c_uint64), ("points", C.POINTER(C.c_double)), ("n_global", C.c_uint64),
                ("n_caustic", C.c_uint64), ("shift", C.c_int32), ("photon_launches", C.c_int32), ("variant", C.c_uint32),
                ("reserved2", C.c_uint32)]


class rt_denoise_config(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double),
                ("sigma_luma", C.c_double), ("eps", C.c_double), ("guides", C.c_int32), ("reserved", C.c_int32 * 5)]


class rt_temporal_config(C.Structure):
    _fields_ = [("alpha", C.c_double), ("plane_tolerance", C.c_double), ("normal_min", C.c_double), ("albedo_tolerance", C.c_double),
                ("min_weight", C.c_double), ("max_history", C.c_int32), ("reserved", C.c_int32 * 5)]


class rt_ao_config(C.Structure):
    _fields_ = [("ao_spp", C.c_int32), ("rays_per_hit", C.c_int32), ("max_distance", C.c_double), ("reserved", C.c_int32 * 4)]


class rt_adaptive_config(C.Structure):
    _fields_ = [("min_spp", C.c_int32), ("reserved", C.c_int32), ("threshold", C.c_double)]


class rt_region(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32)]


class rt_background(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("color0", C.c_double * 3), ("color1", C.c_double * 3), ("scale", C.c_double)]


class rt_env_sampling(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class rt_area_tri(C.Structure):
    _fields_ = [("a", C.c_double * 3), ("e0", C.c_double * 3), ("e1", C.c_double * 3), ("n", C.c_double * 3), ("area2", C.c_double),
                ("q", C.c_uint32), ("light", C.c_int32)]


BACKGROUND_KINDS = ("none", "constant", "gradient", "texture")
SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))  # book 1's ray_color: white straight down, (0.5, 0.7, 1.0) straight up


class rt_tuning(C.Structure):
    _fields_ = [("no_lds", C.c_int32), ("top_nodes", C.c_int32), ("sub_spp", C.c_int32), ("coop_pool", C.c_int32),
                ("max_leaf", C.c_int32), ("sppm_photon_capacity", C.c_int32), ("sppm_knn_candidates", C.c_int32),
                ("multi_force_rccl", C.c_int32), ("wf_workspace_mb", C.c_int32), ("reserved", C.c_int32), ("sah_box_cost", C.c_double)]


class rt_object_desc(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_int32), ("n_children", C.c_int32), ("axis", C.c_int32), ("v", C.c_double * 8)]


OBJECT_TYPES = ("Sphere", "Rect", "Cube", "Triangle", "Mesh", "Transform", "HitableList", "BVHNode", "ConstantMedium", "MovingSphere")


class rt_scene_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_boxes", "n_spheres", "n_rects", "n_tris", "n_xforms", "n_materials",
                                         "n_textures", "n_verts", "max_depth", "committed", "n_cubes")] + [("bytes", C.c_uint64)] + \
               [(n, C.c_int32) for n in ("accel_ok", "accel_nodes", "accel_items", "accel_instances", "accel_stack", "accel_compact")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


_d3 = C.c_double * 3
_dp = C.POINTER(C.c_double)
_LIB = None

# every symbol include/rtamd.h declares: (name, restype, argtypes)
_SIGS = [
    ("rt_abi_version", C.c_int, []),
    ("rt_last_error", C.c_char_p, []),
    ("rt_default_params", None, [C.POINTER(rt_params)]),
    ("rt_device_count", C.c_int, []),
    ("rt_tuning_default", None, [C.POINTER(rt_tuning)]),
    ("rt_tuning_set", C.c_int, [C.POINTER(rt_tuning)]),
    ("rt_release_workspaces", C.c_int64, []),
    ("rt_scene_create", C.c_int, [C.POINTER(C.c_void_p)]),
    ("rt_scene_destroy", None, [C.c_void_p]),
    ("rt_texture_constant", C.c_int, [C.c_void_p, _d3]),
    ("rt_texture_checker", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("rt_texture_image", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    ("rt_texture_noise", C.c_int, [C.c_void_p, C.c_double, C.c_uint64]),
    ("rt_material_lambertian", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_material_metal", C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    ("rt_material_dielectric", C.c_int, [C.c_void_p, C.c_double, C.c_int]),
    ("rt_material_diffuse_light", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_material_isotropic", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_object_constant_medium", C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int]),
    ("rt_object_sphere", C.c_int, [C.c_void_p, _d3, C.c_double, C.c_int]),
    ("rt_object_moving_sphere", C.c_int, [C.c_void_p, _d3, _d3, C.c_double, C.c_double, C.c_double, C.c_int]),
    ("rt_object_rect_xy", C.c_int, [C.c_void_p] + [C.c_double] * 5 + [C.c_int]),
    ("rt_object_rect_xz", C.c_int, [C.c_void_p] + [C.c_double] * 5 + [C.c_int]),
    ("rt_object_rect_yz", C.c_int, [C.c_void_p] + [C.c_double] * 5 + [C.c_int]),
    ("rt_object_cube", C.c_int, [C.c_void_p, _d3, _d3, C.c_int]),
    ("rt_object_sphere_light", C.c_int, [C.c_void_p, _d3, C.c_double, _d3, C.c_double]),
    ("rt_object_xz_rect_light", C.c_int, [C.c_void_p] + [C.c_double] * 5 + [_d3, C.c_double]),
    ("rt_object_mesh", C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_uint64]),
    ("rt_object_mesh_obj", C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64]),
    ("rt_object_transform", C.c_int, [C.c_void_p, _d3, _d3, _d3, C.c_int]),
    ("rt_object_transform_matrix", C.c_int, [C.c_void_p, C.c_double * 16, C.POINTER(C.c_double), C.c_int]),
    ("rt_mesh_data", C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    ("rt_object_triangle", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    ("rt_object_list", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    ("rt_object_bvh_node", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("rt_object_bvh_build", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_uint64]),
    ("rt_object_bounding_box", C.c_int, [C.c_void_p, C.c_int, C.c_double * 6]),
    ("rt_scene_root", C.c_int, [C.c_void_p]),
    ("rt_object_describe", C.c_int, [C.c_void_p, C.c_int, C.POINTER(rt_object_desc)]),
    ("rt_object_children", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("rt_world_new", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_uint64]),
    ("rt_scene_set_root", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_scene_set_lights", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    ("rt_scene_set_background", C.c_int, [C.c_void_p, C.POINTER(rt_background)]),
    ("rt_scene_get_background", C.c_int, [C.c_void_p, C.POINTER(rt_background)]),
    ("rt_scene_set_area_lights", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    ("rt_scene_area_light_tris", C.c_int, [C.c_void_p, C.c_int, C.POINTER(rt_area_tri)]),
    ("rt_scene_set_env_sampling", C.c_int, [C.c_void_p, C.POINTER(rt_env_sampling)]),
    ("rt_scene_get_env_sampling", C.c_int, [C.c_void_p, C.POINTER(rt_env_sampling)]),
    ("rt_scene_cornell_box", C.c_int, [C.c_void_p, C.c_char_p, C.c_double, C.c_uint64, C.POINTER(rt_camera)]),
    ("rt_scene_load_file", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(rt_camera)]),
    ("rt_scene_parse_file", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(rt_camera)]),
    ("rt_scene_commit", C.c_int, [C.c_void_p]),
    ("rt_scene_info_get", C.c_int, [C.c_void_p, C.POINTER(rt_scene_info)]),
    ("rt_scene_fingerprint", C.c_uint64, [C.c_void_p]),
    ("rt_spec_version", C.c_char_p, []),
    ("rt_render", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), _dp, C.POINTER(rt_stats)]),
    ("rt_render_camera_frame", C.c_int, [C.c_void_p, C.POINTER(rt_camera_frame), C.POINTER(rt_params), _dp, C.POINTER(rt_stats)]),
    ("rt_camera_frame_from", C.c_int, [C.POINTER(rt_camera), C.POINTER(rt_camera_frame)]),
    ("rt_default_sppm_config", None, [C.POINTER(rt_sppm_config)]),
    ("rt_render_sppm", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_sppm_config), _dp, _dp,
                                 C.POINTER(C.c_uint64), C.POINTER(rt_stats)]),
    ("rt_render_multi", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int, C.POINTER(C.c_int), _dp, C.POINTER(rt_stats)]),
    ("rt_render_multi_camera_frame", C.c_int, [C.c_void_p, C.POINTER(rt_camera_frame), C.POINTER(rt_params), C.c_int, C.POINTER(C.c_int), _dp,
                                      C.POINTER(rt_stats)]),
    ("rt_render_sppm_multi", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_sppm_config), C.c_int, C.POINTER(C.c_int), _dp,
                              C.POINTER(rt_stats)]),
    ("rt_rccl_version", C.c_int, []),
    ("rt_render_aov", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int32, _dp, C.POINTER(rt_stats)]),
    ("rt_default_denoise_config", None, [C.POINTER(rt_denoise_config)]),
    ("rt_denoise", C.c_int, [C.POINTER(rt_denoise_config), C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
    ("rt_denoise_device", C.c_int, [C.POINTER(rt_denoise_config), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    ("rt_denoise_sym", C.c_int, [C.POINTER(rt_denoise_config), C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
    ("rt_denoise_sym_device", C.c_int, [C.POINTER(rt_denoise_config), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    ("rt_denoised_render", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_denoise_config), C.c_int32, C.c_int32,
                                     _dp, _dp, _dp, _dp, C.POINTER(rt_stats)]),
    ("rt_denoised_render_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_denoise_config), C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_stats)]),
    ("rt_default_temporal_config", None, [C.POINTER(rt_temporal_config)]),
    ("rt_temporal_accumulate", C.c_int, [C.POINTER(rt_temporal_config), C.c_int32, C.c_int32, C.POINTER(rt_camera_frame), C.POINTER(rt_camera_frame),
                                         _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("rt_temporal_accumulate_device", C.c_int, [C.POINTER(rt_temporal_config), C.c_int32, C.c_int32, C.POINTER(rt_camera_frame),
                                                C.POINTER(rt_camera_frame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    ("rt_sequence_create", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(rt_temporal_config), C.POINTER(C.c_void_p)]),
    ("rt_sequence_destroy", None, [C.c_void_p]),
    ("rt_sequence_reset", C.c_int, [C.c_void_p]),
    ("rt_sequence_frames", C.c_int, [C.c_void_p]),
    ("rt_sequence_frame", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_denoise_config), C.c_int32,
                                    C.c_int32, _dp, _dp, _dp, _dp, C.POINTER(rt_stats)]),
    ("rt_default_ao_config", None, [C.POINTER(rt_ao_config)]),
    ("rt_ao_render", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_ao_config), _dp, C.POINTER(rt_stats)]),
    ("rt_ao_render_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_ao_config), C.c_void_p, C.c_void_p,
                                      C.POINTER(rt_stats)]),
    ("rt_default_adaptive_config", None, [C.POINTER(rt_adaptive_config)]),
    ("rt_render_adaptive", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_adaptive_config), _dp,
                                     C.POINTER(C.c_int32), C.POINTER(rt_stats)]),
    ("rt_region_doubles", C.c_int64, [C.POINTER(rt_params), C.c_int, C.POINTER(rt_region)]),
    ("rt_region_tiles", C.c_int64, [C.POINTER(rt_params), C.c_int, C.POINTER(rt_region), C.c_int64, C.POINTER(C.c_int32)]),
    ("rt_region_render", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int, C.POINTER(rt_region), _dp,
                                   C.POINTER(rt_stats)]),
    ("rt_region_render_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int, C.POINTER(rt_region), C.c_void_p,
                                          C.c_void_p, C.POINTER(rt_stats)]),
    ("rt_render_tiles_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p, C.c_void_p,
                                         C.POINTER(rt_stats)]),
    ("rt_render_sppm_tiles_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_sppm_config), C.c_void_p,
                                              C.c_void_p, C.POINTER(rt_stats)]),
    ("rt_render_accumulate_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.POINTER(rt_stats)]),
    ("rt_accum_finalize_device", C.c_int, [C.POINTER(rt_params), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_accum_state_doubles", C.c_int64, [C.POINTER(rt_params)]),
    ("rt_render_accumulate", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int32, C.c_int32, _dp, C.POINTER(rt_stats)]),
    ("rt_accum_finalize", C.c_int, [C.POINTER(rt_params), _dp, _dp]),
    ("rt_tiles_total", C.c_int64, [C.POINTER(rt_params)]),
    ("rt_tiles_owned", C.c_int64, [C.POINTER(rt_params)]),
    ("rt_assemble_frame_device", C.c_int, [C.POINTER(rt_params), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("rt_tonemap_u8", C.c_int, [_dp, C.c_size_t, C.POINTER(C.c_uint8)]),
    ("rt_write_png", C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    ("rt_debug_rng_device", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    ("rt_debug_rng_host", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    ("rt_debug_rng_floats", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("rt_debug_math_device", C.c_int, [C.c_int, C.c_size_t, _dp, _dp, _dp]),
    ("rt_debug_hit_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, C.c_double, C.c_double, _dp]),
    ("rt_debug_schedule", C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("rt_debug_env_table_device", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    ("rt_debug_env_sample_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, _dp]),
    ("rt_debug_env_pdf_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, _dp]),
    ("rt_debug_area_sample_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, _dp]),
    ("rt_debug_area_pdf_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, _dp]),
    ("rt_debug_shade_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, C.POINTER(C.c_uint64), _dp]),
    ("rt_debug_light_sample_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, C.POINTER(C.c_uint64), _dp]),
    ("rt_debug_light_pdf_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, _dp, _dp]),
    ("rt_debug_walk_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, _dp, C.POINTER(C.c_uint64), C.c_double, _dp]),
    ("rt_debug_occluded_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, _dp, C.c_double, _dp]),
    ("rt_debug_sppm_gather_device", C.c_int, [C.c_int, C.POINTER(rt_debug_sppm_gather)]),
    ("rt_debug_sppm_trace_device", C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.c_int, C.POINTER(rt_debug_sppm_trace)]),
    ("rt_debug_grid_shape", C.c_int, [_dp, _dp, C.c_uint64, _dp, C.POINTER(C.c_int32)]),
]
ABI_SYMBOLS = [s[0] for s in _SIGS]


def _share_hip_runtime_with_torch():
    """One process must hold ONE HIP/HSA runtime and ONE RCCL.  PyTorch-ROCm bundles its own libamdhip64.so.7 and librccl.so.1
    (same SONAMEs as /opt/rocm's, which librtamd.so names as its dependencies): whichever copy is loaded first serves both.  If torch is
    installed but not imported yet, import it FIRST, so that a later `import torch` in the same process (bench.py, the tests) does not
    find the system's runtime under its own kernels -- "No HIP GPUs are available" -- or the system's RCCL under its `nccl` backend.
    (Pre-loading torch's libraries one by one instead is not safe: with librccl.so loaded before torch's own loader asks for it the
    process ends in `double free or corruption` at exit.)  RTAMD_HIP_RUNTIME=system skips this: /opt/rocm's runtime and RCCL, for hosts
    that never import torch."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("RTAMD_HIP_RUNTIME", "") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None:
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    """Load librtamd.so.  Raises (never falls back) when the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise ImportError("librtamd.so is missing at %s -- run `make -C rust-raytracer_amd` (or __graft_entry__.build()); "
                          "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, res, args in _SIGS:
        fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def _chk(rc):
    if rc < 0:
        raise RtError(rc, lib().rt_last_error().decode("utf-8", "replace"))
    return rc


def device_count():
    return lib().rt_device_count()


def default_params(**kw):
    p = rt_params()
    lib().rt_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _arr3(v):
    return _d3(*[float(x) for x in v])


class Camera:
    """Camera::new (camera.rs:24-55) arguments; capture_image renders through a World."""

    def __init__(self, look_from_to, vup, vfov, aspect_ratio, aperture, focus_dist):
        look_from, look_at = look_from_to
        self.c = rt_camera(_arr3(look_from), _arr3(look_at), _arr3(vup), float(vfov), float(aspect_ratio), float(aperture),
                           float(focus_dist))

    @classmethod
    def from_struct(cls, c):
        self = cls.__new__(cls)
        self.c = c
        return self

    def frame(self):
        """the Camera struct's stored fields (camera.rs:12-21) as an rt_camera_frame: rt_camera_frame_from = Camera::new"""
        f = rt_camera_frame()
        _chk(lib().rt_camera_frame_from(C.byref(self.c), C.byref(f)))
        return f

    def with_aspect(self, aspect):
        c = rt_camera.from_buffer_copy(self.c)
        c.aspect = float(aspect)
        return Camera.from_struct(c)

    def capture_image(self, world, width=800, height=800, sample_per_pixel=256, **kw):
        """Camera::capture_image (camera.rs:66-128): returns an RgbImage as uint8 [H,W,3]."""
        rad, _ = world.render(self, width=width, height=height, spp=sample_per_pixel, **kw)
        return tonemap_u8(rad)


class World:
    """World (world.rs:8-30) + the Hitable/Material/Texture constructors that populate it."""

    def __init__(self, handle=None):
        self.L = lib()
        if handle is None:
            h = C.c_void_p()
            _chk(self.L.rt_scene_create(C.byref(h)))
            handle = h
        self.h = handle

    def __del__(self):
        try:
            if self.h:
                self.L.rt_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # --- textures (material.rs:48-50) ---
    def ConstantTexture(self, color):
        return _chk(self.L.rt_texture_constant(self.h, _arr3(color)))

    def CheckerTexture(self, t0, t1):
        return _chk(self.L.rt_texture_checker(self.h, t0, t1))

    def ImageTexture(self, rgb_u8):
        a = np.ascontiguousarray(rgb_u8, dtype=np.uint8)
        return _chk(self.L.rt_texture_image(self.h, a.shape[1], a.shape[0], a.ctypes.data_as(C.POINTER(C.c_uint8))))

    def NoiseTexture(self, scale, seed=1):
        """book-2 extension (no reference code): Perlin marble texture 0.5 (1 + sin(scale z + 10 turb(p)))"""
        return _chk(self.L.rt_texture_noise(self.h, float(scale), int(seed)))

    # --- materials (material.rs:88-212) ---
    def Lambertian(self, albedo):
        return _chk(self.L.rt_material_lambertian(self.h, albedo))

    def Metal(self, albedo, fuzz):
        return _chk(self.L.rt_material_metal(self.h, albedo, float(fuzz)))

    def Dielectric(self, ir, albedo):
        return _chk(self.L.rt_material_dielectric(self.h, float(ir), albedo))

    def DiffuseLight(self, emit):
        return _chk(self.L.rt_material_diffuse_light(self.h, emit))

    def Isotropic(self, albedo):
        return _chk(self.L.rt_material_isotropic(self.h, albedo))

    # --- hitables (objects/*.rs, light.rs) ---
    def Sphere(self, center, radius, material):
        return _chk(self.L.rt_object_sphere(self.h, _arr3(center), float(radius), material))

    def MovingSphere(self, center0, center1, time0, time1, radius, material):
        """book-2 extension (no reference code): a sphere whose centre moves linearly from center0 at time0 to center1 at time1"""
        return _chk(self.L.rt_object_moving_sphere(self.h, _arr3(center0), _arr3(center1), float(time0), float(time1), float(radius), material))

    def XYRectangle(self, xy0, xy1, z, material):
        return _chk(self.L.rt_object_rect_xy(self.h, float(xy0[0]), float(xy0[1]), float(xy1[0]), float(xy1[1]), float(z), material))

    def XZRectangle(self, xz0, xz1, y, material):
        return _chk(self.L.rt_object_rect_xz(self.h, float(xz0[0]), float(xz0[1]), float(xz1[0]), float(xz1[1]), float(y), material))

    def YZRectangle(self, yz0, yz1, x, material):
        return _chk(self.L.rt_object_rect_yz(self.h, float(yz0[0]), float(yz0[1]), float(yz1[0]), float(yz1[1]), float(x), material))

    def Cube(self, box_min, box_max, material):
        return _chk(self.L.rt_object_cube(self.h, _arr3(box_min), _arr3(box_max), material))

    def SphereDiffuseLight(self, center, radius, flux, scale=1.0):
        return _chk(self.L.rt_object_sphere_light(self.h, _arr3(center), float(radius), _arr3(flux), float(scale)))

    def XZRectLight(self, xz0, xz1, y, flux, scale=1.0):
        return _chk(self.L.rt_object_xz_rect_light(self.h, float(xz0[0]), float(xz0[1]), float(xz1[0]), float(xz1[1]), float(y),
                                                   _arr3(flux), float(scale)))

    def ConstantMedium(self, density, boundary, phase_function):
        return _chk(self.L.rt_object_constant_medium(self.h, float(density), boundary, phase_function))

    def Mesh(self, positions, normals, indices, material, synthesize_normals=False, bvh_seed=1):
        p = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        n_ptr = None
        if normals is not None:
            n = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
            assert n.shape == p.shape
            n_ptr = n.ctypes.data_as(_dp)
        return _chk(self.L.rt_object_mesh(self.h, p.shape[0], p.ctypes.data_as(_dp), n_ptr, i.shape[0],
                                          i.ctypes.data_as(C.POINTER(C.c_uint32)), material, int(synthesize_normals), int(bvh_seed)))

    def Mesh_load_obj(self, obj_file, material, synthesize_normals=False, bvh_seed=1):
        return _chk(self.L.rt_object_mesh_obj(self.h, os.fsencode(obj_file), material, int(synthesize_normals), int(bvh_seed)))

    def Transform(self, rotate_in_degree, scale, translate, obj):
        return _chk(self.L.rt_object_transform(self.h, _arr3(rotate_in_degree), _arr3(scale), _arr3(translate), obj))

    def Transform_from_matrix(self, trans, obj, inverse_trans=None):
        """Transform as the reference stores it: the composed 4x4 (row-major) and optionally its inverse."""
        m = (C.c_double * 16)(*[float(x) for x in np.asarray(trans, dtype=np.float64).reshape(16)])
        inv = None
        if inverse_trans is not None:
            inv = (C.c_double * 16)(*[float(x) for x in np.asarray(inverse_trans, dtype=np.float64).reshape(16)])
        return _chk(self.L.rt_object_transform_matrix(self.h, m, inv, obj))

    def MeshData(self, positions, normals):
        """the shared vertex arrays of a mesh (returns a mesh id for Triangle)"""
        p = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        n = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        assert n.shape == p.shape
        return _chk(self.L.rt_mesh_data(self.h, p.shape[0], p.ctypes.data_as(_dp), n.ctypes.data_as(_dp)))

    def Triangle(self, mesh, a, b, c, material):
        return _chk(self.L.rt_object_triangle(self.h, mesh, int(a), int(b), int(c), material))

    def HitableList(self, objects):
        arr = (C.c_int * len(objects))(*objects)
        return _chk(self.L.rt_object_list(self.h, len(objects), arr))

    def BVHNode_construct(self, left, right):
        return _chk(self.L.rt_object_bvh_node(self.h, left, right))

    def BVHNode_new(self, objects, bvh_seed=1):
        arr = (C.c_int * len(objects))(*objects)
        return _chk(self.L.rt_object_bvh_build(self.h, len(objects), arr, int(bvh_seed)))

    def bounding_box(self, obj):
        out = (C.c_double * 6)()
        _chk(self.L.rt_object_bounding_box(self.h, obj, out))
        return np.array(out[:])

    # --- graph introspection ---
    def root(self):
        return _chk(self.L.rt_scene_root(self.h))

    def describe(self, obj):
        """(type name, dict) of an object id: material, axis, parameters v, children ids."""
        d = rt_object_desc()
        _chk(self.L.rt_object_describe(self.h, obj, C.byref(d)))
        kids = (C.c_int * max(1, d.n_children))()
        _chk(self.L.rt_object_children(self.h, obj, d.n_children, kids))
        return OBJECT_TYPES[d.type], {"material": d.material, "axis": d.axis, "v": list(d.v), "children": list(kids[:d.n_children])}

    # --- World::new / commit ---
    def new(self, hitable_list, lights=(), bvh_seed=1, area_lights=()):
        """World::new(hitable_list, cam, lights) (world.rs:15-25): root = BVHNode::new(hitable_list); then commit.
        area_lights: objects for set_area_lights."""
        arr = (C.c_int * len(hitable_list))(*hitable_list)
        _chk(self.L.rt_world_new(self.h, len(hitable_list), arr, int(bvh_seed)))
        if len(lights):
            self.set_lights(list(lights))
        if len(area_lights):
            self.set_area_lights(list(area_lights))
        return self.commit()

    def set_area_lights(self, objs):
        """rt_scene_set_area_lights (before commit): emissive rectangles, cubes, triangles and meshes -- lists and BVH nodes of them, under
        up to 8 nested Transforms -- that integrator 1 samples beside the object lights; an empty list clears it."""
        arr = (C.c_int * len(objs))(*objs)
        _chk(self.L.rt_scene_set_area_lights(self.h, len(objs), arr))
        return self

    def area_light_tris(self):
        """rt_scene_area_light_tris: the world-space triangles a committed scene's area lights were lowered to, as a numpy record array
        with the fields a, e0, e1, n (f64 [3]), area2 (f64), q (uint32), light (int32)"""
        n = _chk(self.L.rt_scene_area_light_tris(self.h, 0, None))
        out = np.zeros(n, dtype=AREA_TRI_DTYPE)
        if n:
            _chk(self.L.rt_scene_area_light_tris(self.h, n, out.ctypes.data_as(C.POINTER(rt_area_tri))))
        return out

    def set_lights(self, lights):
        arr = (C.c_int * len(lights))(*lights)
        _chk(self.L.rt_scene_set_lights(self.h, len(lights), arr))
        self.n_lights = len(lights)

    def set_background(self, color=None, gradient=None, texture=None, scale=1.0):
        """rt_scene_set_background (before commit): at most one of color=(r, g, b) (kind 1), gradient=((down), (up)) (kind 2) or
        texture=<texture id> (kind 3, sampled by direction; an ImageTexture is an equirectangular map).  None of them: no background."""
        if sum(x is not None for x in (color, gradient, texture)) > 1:
            raise ValueError("set_background takes one of color, gradient, texture")
        bg = rt_background()
        bg.scale = float(scale)
        if color is not None:
            bg.kind = 1
            bg.color0 = _arr3(color)
        elif gradient is not None:
            bg.kind = 2
            bg.color0 = _arr3(gradient[0])
            bg.color1 = _arr3(gradient[1])
        elif texture is not None:
            bg.kind = 3
            bg.texture = int(texture)
        _chk(self.L.rt_scene_set_background(self.h, C.byref(bg)))
        return self

    def set_sky(self, scale=1.0):
        """book 1's sky: the vertical gradient from white (straight down) to (0.5, 0.7, 1.0) (straight up)"""
        return self.set_background(gradient=SKY, scale=scale)

    def background(self):
        """rt_scene_get_background: dict(kind, texture, color0, color1, scale)"""
        bg = rt_background()
        _chk(self.L.rt_scene_get_background(self.h, C.byref(bg)))
        return dict(kind=bg.kind, texture=bg.texture, color0=tuple(bg.color0), color1=tuple(bg.color1), scale=bg.scale)

    def set_env_sampling(self, enabled=True, width=0, height=0):
        """rt_scene_set_env_sampling (before commit): the background becomes one more light of integrator 1, drawn from a width x height
        table over (u, v) that every device builds from the background itself; 0, 0 = automatic (an image map: one cell per texel, halved
        down to 4096 x 2048; anything else 256 x 128)."""
        cfg = rt_env_sampling(1 if enabled else 0, int(width), int(height))
        _chk(self.L.rt_scene_set_env_sampling(self.h, C.byref(cfg)))
        return self

    def env_sampling(self):
        """rt_scene_get_env_sampling: dict(enabled, width, height) as set"""
        cfg = rt_env_sampling()
        _chk(self.L.rt_scene_get_env_sampling(self.h, C.byref(cfg)))
        return dict(enabled=bool(cfg.enabled), width=cfg.width, height=cfg.height)

    def fingerprint(self):
        return int(self.L.rt_scene_fingerprint(self.h))

    def set_root(self, obj):
        _chk(self.L.rt_scene_set_root(self.h, obj))
        return self.commit()

    def commit(self):
        _chk(self.L.rt_scene_commit(self.h))
        return self

    def info(self):
        out = rt_scene_info()
        _chk(self.L.rt_scene_info_get(self.h, C.byref(out)))
        return out.as_dict()

    # --- the hot path ---
    def render(self, camera, width=800, height=800, spp=256, max_depth=50, t_min=1e-3, seed=1, rank=0, world=1, spp_chunk=0,
               kernel=0, device=-1, integrator=0, shutter=(0.0, 0.0)):
        """rt_render: linear radiance f64 [H,W,3] on the host + stats dict.  shutter = (time0, time1): the book-2 camera shutter."""
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, rank=rank, world=world,
                           spp_chunk=spp_chunk, kernel=kernel, device=device, integrator=integrator, time0=float(shutter[0]), time1=float(shutter[1]))
        out = np.zeros((height, width, 3), dtype=np.float64)
        st = rt_stats()
        _chk(self.L.rt_render(self.h, C.byref(camera.c), C.byref(p), out.ctypes.data_as(_dp), C.byref(st)))
        return out, st.as_dict()

    def render_adaptive(self, camera, width, height, spp, min_spp=16, threshold=None, seed=1, kernel=0, integrator=0, max_depth=50,
                        t_min=1e-3, device=-1, spp_chunk=0):
        """rt_render_adaptive: tile-adaptive sampling.  Every 8x8 tile gets min_spp samples, then doubles its count until
        its two-buffer error drops below `threshold` (None: the library's default) or it reaches spp.  Returns (radiance [H,W,3],
        tile_spp int32 [tiles_y, tiles_x] = each tile's final sample count, stats dict)."""
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, kernel=kernel,
                           integrator=integrator, device=device, spp_chunk=spp_chunk)
        cfg = rt_adaptive_config()
        self.L.rt_default_adaptive_config(C.byref(cfg))
        cfg.min_spp = int(min_spp)
        if threshold is not None:
            cfg.threshold = float(threshold)
        out = np.zeros((height, width, 3), dtype=np.float64)
        tile_spp = np.zeros(((height + 7) // 8, (width + 7) // 8), dtype=np.int32)
        st = rt_stats()
        _chk(self.L.rt_render_adaptive(self.h, C.byref(camera.c), C.byref(p), C.byref(cfg), out.ctypes.data_as(_dp),
                                       tile_spp.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st)))
        return out, tile_spp, st.as_dict()

    def render_multi(self, camera, devices=None, gpus=0, width=800, height=800, spp=256, max_depth=50, t_min=1e-3, seed=1, spp_chunk=0,
                     kernel=0, integrator=0, shutter=(0.0, 0.0)):
        """rt_render_multi: the frame across the GPUs of this node in ONE call (one host thread per rank inside the library, rows
        gathered on devices[0] through RCCL).  devices = HIP ordinals, one per rank (may repeat); or gpus = N for devices 0..N-1
        (0 = all visible).  Returns (radiance [H,W,3], [per-rank stats dicts]); stats[0] also carries 'exchange_seconds' and
        'rows_through_rccl'."""
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, spp_chunk=spp_chunk,
                           kernel=kernel, integrator=integrator, time0=float(shutter[0]), time1=float(shutter[1]))
        n = len(devices) if devices is not None else int(gpus)
        ids = (C.c_int * n)(*[int(d) for d in devices]) if devices is not None else None
        n_st = n if n > 0 else max(1, device_count())
        st = (rt_stats * n_st)()
        out = np.zeros((height, width, 3), dtype=np.float64)
        _chk(self.L.rt_render_multi(self.h, C.byref(camera.c), C.byref(p), n, ids, out.ctypes.data_as(_dp), st))
        ds = [s.as_dict() for s in st]
        ds[0]["exchange_seconds"] = st[0].reserved[2] * 1e-6
        ds[0]["rows_through_rccl"] = int(st[0].reserved[3])
        return out, ds

    def render_sppm_multi(self, camera, devices=None, gpus=0, width=800, height=800, spp=256, max_depth=50, t_min=1e-3, seed=1, kernel=0, **sppm):
        """rt_render_sppm_multi: main.rs:52-54 across GPUs (every rank repeats the SPPM pre-pass, renders its tiles)."""
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, kernel=kernel)
        cfg = rt_sppm_config()
        self.L.rt_default_sppm_config(C.byref(cfg))
        for k, v in sppm.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown SPPM setting %r" % k)
            setattr(cfg, k, v)
        n = len(devices) if devices is not None else int(gpus)
        ids = (C.c_int * n)(*[int(d) for d in devices]) if devices is not None else None
        st = (rt_stats * (n if n > 0 else max(1, device_count())))()
        out = np.zeros((height, width, 3), dtype=np.float64)
        _chk(self.L.rt_render_sppm_multi(self.h, C.byref(camera.c), C.byref(p), C.byref(cfg), n, ids, out.ctypes.data_as(_dp), st))
        return out, [s.as_dict() for s in st]

    def render_camera_frame(self, frame, **kw):
        """rt_render_camera_frame: `frame` is an rt_camera_frame (the Camera struct's stored fields)."""
        width, height = kw.get("width", 800), kw.get("height", 800)
        p = default_params(**kw)
        out = np.zeros((height, width, 3), dtype=np.float64)
        st = rt_stats()
        _chk(self.L.rt_render_camera_frame(self.h, C.byref(frame), C.byref(p), out.ctypes.data_as(_dp), C.byref(st)))
        return out, st.as_dict()

    def render_sppm(self, camera, width=800, height=800, spp=256, iterations=50, photons_per_iter=500000, alpha=0.7, k_global=100,
                    k_caustic=50, max_bounces=4096, max_depth=50, t_min=1e-3, seed=1, kernel=0, device=-1):
        """rt_render_sppm = SPPMIntegrator::new + capture_image (main.rs:52-54).
        Returns (radiance [H,W,3], per-pixel stats [H,W,10], (photons in the global maps, in the caustic maps), stats dict)."""
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, kernel=kernel, device=device)
        cfg = rt_sppm_config()
        self.L.rt_default_sppm_config(C.byref(cfg))
        cfg.iterations, cfg.photons_per_iter, cfg.k_global, cfg.k_caustic = iterations, photons_per_iter, k_global, k_caustic
        cfg.max_bounces, cfg.alpha = max_bounces, alpha
        out = np.zeros((height, width, 3), dtype=np.float64)
        stats = np.zeros((height, width, 10), dtype=np.float64)
        tot = (C.c_uint64 * 2)()
        st = rt_stats()
        _chk(self.L.rt_render_sppm(self.h, C.byref(camera.c), C.byref(p), C.byref(cfg), out.ctypes.data_as(_dp), stats.ctypes.data_as(_dp), tot,
                                   C.byref(st)))
        d = st.as_dict()
        d["prepass_seconds"] = st.reserved[0] * 1e-6
        return out, stats, (int(tot[0]), int(tot[1])), d

    def render_regions(self, camera, regions, width=800, height=800, spp=256, max_depth=50, t_min=1e-3, seed=1, rank=0, world=1, spp_chunk=0,
                       kernel=0, device=-1, integrator=0, shutter=(0.0, 0.0)):
        """rt_region_render: the pixel rectangles regions = [(x0, y0, x1, y1), ...] ([x0, x1) x [y0, y1), y down) of the width x height frame
        render() would return, bit for bit, at the cost of the 8x8 tiles they touch.  Returns ([radiance f64
        [y1 - y0, x1 - x0, 3] per region], stats dict)."""
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, rank=rank, world=world,
                           spp_chunk=spp_chunk, kernel=kernel, device=device, integrator=integrator, time0=float(shutter[0]), time1=float(shutter[1]))
        arr, n = _regions(regions)
        out = np.zeros(_chk(self.L.rt_region_doubles(C.byref(p), n, arr)), dtype=np.float64)
        st = rt_stats()
        _chk(self.L.rt_region_render(self.h, C.byref(camera.c), C.byref(p), n, arr, out.ctypes.data_as(_dp), C.byref(st)))
        views, at = [], 0
        for r in arr[:n]:
            h, w = r.y1 - r.y0, r.x1 - r.x0
            views.append(out[at:at + h * w * 3].reshape(h, w, 3))
            at += h * w * 3
        return views, st.as_dict()

    def render_region(self, camera, region, **kw):
        """render_regions for one region (x0, y0, x1, y1): returns (radiance [y1 - y0, x1 - x0, 3], stats dict)"""
        views, st = self.render_regions(camera, [region], **kw)
        return views[0], st

    def render_regions_device(self, camera, params, regions, d_out_ptr, stream_ptr=None):
        """rt_region_render_device: the packed regions (region_doubles(params, regions) f64) into a raw device pointer (e.g. torch tensor
        .data_ptr()), queued on stream_ptr; returns the stats dict after the work has completed on that stream."""
        arr, n = _regions(regions)
        st = rt_stats()
        _chk(self.L.rt_region_render_device(self.h, C.byref(camera.c), C.byref(params), n, arr, C.c_void_p(d_out_ptr),
                                            C.c_void_p(stream_ptr or 0), C.byref(st)))
        return st.as_dict()

    def render_tiles_device(self, camera, params, d_tiles_ptr, stream_ptr=None):
        """rt_render_tiles_device: d_tiles_ptr is a raw device pointer (e.g. torch tensor .data_ptr())."""
        st = rt_stats()
        _chk(self.L.rt_render_tiles_device(self.h, C.byref(camera.c), C.byref(params), C.c_void_p(d_tiles_ptr),
                                           C.c_void_p(stream_ptr or 0), C.byref(st)))
        return st.as_dict()

    def render_accumulate(self, camera, params, sample_begin, sample_end, state=None):
        """rt_render_accumulate: samples [sample_begin, sample_end) added to the host-held accumulator state (numpy f64, created when None);
        returns (state, stats).  accum_finalize(params, state) gives the frame once every sample is in."""
        n = int(lib().rt_accum_state_doubles(C.byref(params)))
        if n <= 0:
            raise RtError(n, "bad image size or partition")
        if state is None:
            state = np.zeros(n, dtype=np.float64)
        assert state.dtype == np.float64 and state.size == n and state.flags["C_CONTIGUOUS"]
        st = rt_stats()
        _chk(self.L.rt_render_accumulate(self.h, C.byref(camera.c), C.byref(params), int(sample_begin), int(sample_end),
                                         state.ctypes.data_as(_dp), C.byref(st)))
        return state, st.as_dict()

    def render_accumulate_device(self, camera, params, sample_begin, sample_end, d_accum_ptr, stream_ptr=None):
        """rt_render_accumulate_device: samples [sample_begin, sample_end) of this rank's tiles are added, in index order, to the caller's
        accumulator (raw device pointer, rt_tiles_owned * 64 * 3 f64; sample_begin == 0 initialises it) -- resumable rendering."""
        st = rt_stats()
        _chk(self.L.rt_render_accumulate_device(self.h, C.byref(camera.c), C.byref(params), int(sample_begin), int(sample_end), C.c_void_p(d_accum_ptr),
                                                C.c_void_p(stream_ptr or 0), C.byref(st)))
        return st.as_dict()

    def render_sppm_tiles_device(self, camera, params, d_tiles_ptr, stream_ptr=None, **sppm):
        """rt_render_sppm_tiles_device: the (replicated, deterministic) SPPM pre-pass, then this rank's tiles of the final pass.
        sppm: iterations, photons_per_iter, alpha, k_global, k_caustic, max_bounces (defaults = the reference's constants)."""
        cfg = rt_sppm_config()
        self.L.rt_default_sppm_config(C.byref(cfg))
        for k, v in sppm.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown SPPM setting %r" % k)
            setattr(cfg, k, v)
        st = rt_stats()
        _chk(self.L.rt_render_sppm_tiles_device(self.h, C.byref(camera.c), C.byref(params), C.byref(cfg), C.c_void_p(d_tiles_ptr),
                                                C.c_void_p(stream_ptr or 0), C.byref(st)))
        d = st.as_dict()
        d["prepass_seconds"] = st.reserved[0] * 1e-6
        return d

    # --- guide buffers and denoising ---
    def render_aov(self, camera, width, height, aov_spp=4, seed=1, kernel=0, t_min=1e-3, device=-1):
        """rt_render_aov: first-hit guide buffers [H, W, 8] = {normal[3], t, albedo[3], coverage}, averaged over the aov_spp camera rays
        render() draws first for each pixel (samples 0 .. aov_spp-1 of stream (seed, pixel, s)); returns (aov, stats dict)."""
        p = default_params(width=width, height=height, seed=seed, kernel=kernel, t_min=t_min, device=device)
        out = np.zeros((height, width, 8), dtype=np.float64)
        st = rt_stats()
        _chk(self.L.rt_render_aov(self.h, C.byref(camera.c), C.byref(p), int(aov_spp), out.ctypes.data_as(_dp), C.byref(st)))
        return out, st.as_dict()

    # --- ambient occlusion ---
    def _ao_config(self, ao_spp, rays_per_hit, max_distance):
        c = rt_ao_config()
        self.L.rt_default_ao_config(C.byref(c))
        c.ao_spp, c.rays_per_hit, c.max_distance = int(ao_spp), int(rays_per_hit), float(max_distance)
        return c

    def render_ao(self, camera, width, height, ao_spp=4, rays_per_hit=4, max_distance=float("inf"), seed=1, kernel=0, t_min=1e-3, device=-1):
        """rt_ao_render: [H, W, 8] = {visibility, bent normal[3], ambient[3], coverage} from ao_spp camera rays per pixel (render()'s
        first samples) and rays_per_hit cosine-distributed occlusion rays per hit, no farther than max_distance; returns (ao, stats dict)."""
        p = default_params(width=width, height=height, seed=seed, kernel=kernel, t_min=t_min, device=device)
        c = self._ao_config(ao_spp, rays_per_hit, max_distance)
        out = np.zeros((height, width, 8), dtype=np.float64)
        st = rt_stats()
        _chk(self.L.rt_ao_render(self.h, C.byref(camera.c), C.byref(p), C.byref(c), out.ctypes.data_as(_dp), C.byref(st)))
        return out, st.as_dict()

    def render_ao_device(self, camera, params, d_out_ptr, ao_spp=4, rays_per_hit=4, max_distance=float("inf"), stream_ptr=None):
        """rt_ao_render_device: the same into DEVICE memory at d_out_ptr ([H, W, 8] f64) on the HIP stream stream_ptr; returns the stats
        dict after the work has completed on that stream."""
        c = self._ao_config(ao_spp, rays_per_hit, max_distance)
        st = rt_stats()
        _chk(self.L.rt_ao_render_device(self.h, C.byref(camera.c), C.byref(params), C.byref(c), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0),
                                        C.byref(st)))
        return st.as_dict()

    def render_denoised(self, camera, width=800, height=800, spp=256, guides=True, aov_spp=4, max_depth=50, t_min=1e-3, seed=1,
                        kernel=0, device=-1, integrator=0, native=False, luma_mode=1, **cfg):
        """A frame, its variance and its guides, filtered by rt_denoise.  native=True: the one call rt_denoised_render, which keeps
        everything but the four results on the device and filters with rt_denoise (luma_mode 0) or rt_denoise_sym (luma_mode 1, the
        energy-preserving stop); with luma_mode 0 its results are the composition's bit for bit.  native=False (the default) is the
        composition below, which ignores luma_mode.  spp must be even: samples [0, spp/2) and [spp/2, spp) go through
        the resumable path (rt_render_accumulate) into ONE accumulator, so `noisy` is bit for bit render()'s frame; the half-means A and B
        give variance = (l_A - l_B)^2 / 4 of the pixel's mean luminance l.  guides=False skips rt_render_aov (aov is None then: scenes
        with media or moving spheres).  cfg: rt_denoise_config fields.  Returns (denoised, noisy, variance, aov)."""
        if spp < 2 or spp % 2:
            raise ValueError("render_denoised needs an even spp >= 2 (two half-frames), got %r" % (spp,))
        if native:
            p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, kernel=kernel, device=device,
                               integrator=integrator)
            c = denoise_config(**cfg)
            den, noisy = np.zeros((height, width, 3)), np.zeros((height, width, 3))
            variance = np.zeros((height, width))
            aov = np.zeros((height, width, 8)) if guides else None
            st = rt_stats()
            _chk(self.L.rt_denoised_render(self.h, C.byref(camera.c), C.byref(p), C.byref(c), int(luma_mode), int(aov_spp) if guides else 0,
                                           den.ctypes.data_as(_dp), noisy.ctypes.data_as(_dp), variance.ctypes.data_as(_dp),
                                           aov.ctypes.data_as(_dp) if guides else None, C.byref(st)))
            return den, noisy, variance, aov
        p = default_params(width=width, height=height, spp=spp, max_depth=max_depth, t_min=t_min, seed=seed, kernel=kernel, device=device,
                           integrator=integrator)
        half = spp // 2
        state, _ = self.render_accumulate(camera, p, 0, half)
        first = state.copy()
        state, _ = self.render_accumulate(camera, p, half, spp, state)
        noisy = accum_finalize(p, state)
        ph = default_params(width=width, height=height, spp=half, max_depth=max_depth, t_min=t_min, seed=seed, kernel=kernel, device=device,
                            integrator=integrator)
        mean_a = accum_finalize(ph, first)
        mean_b = accum_finalize(ph, state - first)
        variance = (luminance(mean_a) - luminance(mean_b)) ** 2 / 4.0
        aov = None
        if guides:  # (the guides take kernel 1's or kernel 2's walk: kernels 5 / 6 render the frame, the automatic choice walks the guides)
            aov = self.render_aov(camera, width, height, aov_spp=aov_spp, seed=seed, kernel=kernel if kernel in (1, 2) else 0, t_min=t_min,
                                  device=device)[0]
        return denoise(noisy, variance, aov, **cfg), noisy, variance, aov

    def render_denoised_device(self, camera, params, d_out_ptr, d_noisy_ptr=None, d_variance_ptr=None, d_aov_ptr=None, aov_spp=4, luma_mode=1,
                               stream_ptr=None, **cfg):
        """rt_denoised_render_device: the denoised frame [H, W, 3] -- and, where a pointer is given, the noisy frame [H, W, 3], the variance
        [H, W] and the guides [H, W, 8] -- into raw device pointers (e.g. torch tensor .data_ptr()) of the call's device, queued on
        stream_ptr.  aov_spp = 0: no guides (d_aov_ptr must be None).  Returns the stats dict after the work has completed on that stream."""
        c = denoise_config(**cfg)
        st = rt_stats()
        _chk(self.L.rt_denoised_render_device(self.h, C.byref(camera.c), C.byref(params), C.byref(c), int(luma_mode), int(aov_spp), C.c_void_p(d_out_ptr),
                                              C.c_void_p(d_noisy_ptr or 0), C.c_void_p(d_variance_ptr or 0), C.c_void_p(d_aov_ptr or 0),
                                              C.c_void_p(stream_ptr or 0), C.byref(st)))
        return st.as_dict()

    def debug_hit(self, rays, t_min=1e-3, t_max=float("inf"), kernel=1):
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros((r.shape[0], 12), dtype=np.float64)
        _chk(self.L.rt_debug_hit_device(self.h, int(kernel), r.shape[0], r.ctypes.data_as(_dp), float(t_min), float(t_max),
                                        out.ctypes.data_as(_dp)))
        return out

    def debug_env_table(self, device=0):
        """rt_debug_env_table_device: the quantised weights q, uint32 [H, W] (row j = v cell j), as `device` built them"""
        w, h = C.c_int(), C.c_int()
        _chk(self.L.rt_debug_env_table_device(self.h, int(device), C.byref(w), C.byref(h), None))
        q = np.zeros((h.value, w.value), dtype=np.uint32)
        _chk(self.L.rt_debug_env_table_device(self.h, int(device), C.byref(w), C.byref(h), q.ctypes.data_as(C.POINTER(C.c_uint32))))
        return q

    def debug_env_sample(self, xi, device=0):
        """rt_debug_env_sample_device: xi [n, 4] -> [n, 4] = direction, pdf"""
        x = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, 4)
        out = np.zeros((x.shape[0], 4), dtype=np.float64)
        _chk(self.L.rt_debug_env_sample_device(self.h, int(device), x.shape[0], x.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def debug_env_pdf(self, dirs, device=0):
        """rt_debug_env_pdf_device: directions [n, 3] (any length) -> pdf [n] per solid angle"""
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(d.shape[0], dtype=np.float64)
        _chk(self.L.rt_debug_env_pdf_device(self.h, int(device), d.shape[0], d.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def debug_area_sample(self, o_xi, device=0):
        """rt_debug_area_sample_device: [n, 7] = origin, xi0 (picks the area light), xi1..xi3 -> [n, 4] = direction, pdf (summed over
        all area lights)"""
        x = np.ascontiguousarray(o_xi, dtype=np.float64).reshape(-1, 7)
        out = np.zeros((x.shape[0], 4), dtype=np.float64)
        _chk(self.L.rt_debug_area_sample_device(self.h, int(device), x.shape[0], x.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def debug_area_pdf(self, rays, device=0):
        """rt_debug_area_pdf_device: rays [n, 6] = origin, direction (any length) -> pdf [n] per solid angle, summed over all area lights"""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros(r.shape[0], dtype=np.float64)
        _chk(self.L.rt_debug_area_pdf_device(self.h, int(device), r.shape[0], r.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def debug_shade(self, rows, keys, device=0):
        """rt_debug_shade_device: rows [n, 17] = mat, mix, ray origin, ray direction, p, normal, front_face, u, v; keys uint64 [n, 3] =
        seed, pixel, sample -> [n, 22] = scattered, diffuse, out_dir, att, emitted, mixed, continued, beta, dir, unit-zero status, the
        next draw's two 32-bit halves"""
        x = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 17)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(x.shape[0], 3)
        out = np.zeros((x.shape[0], 22), dtype=np.float64)
        _chk(self.L.rt_debug_shade_device(self.h, int(device), x.shape[0], x.ctypes.data_as(_dp), k.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          out.ctypes.data_as(_dp)))
        return out

    def debug_walk(self, rays7, keys, t_min=1e-3, kernel=1, device=0):
        """rt_debug_walk_device: rays7 [n, 7] = origin, direction, ray time; keys uint64 [n, 3] = seed, pixel, sample -> [n, 14] =
        debug_hit's 12 fields, then the next draw's two 32-bit halves.  The closest-hit query for scenes with media or moving spheres."""
        r = np.ascontiguousarray(rays7, dtype=np.float64).reshape(-1, 7)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(r.shape[0], 3)
        out = np.zeros((r.shape[0], 14), dtype=np.float64)
        _chk(self.L.rt_debug_walk_device(self.h, int(device), int(kernel), r.shape[0], r.ctypes.data_as(_dp), k.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         float(t_min), out.ctypes.data_as(_dp)))
        return out

    def debug_occluded(self, rays7, t_min=1e-3, kernel=1, device=0):
        """rt_debug_occluded_device: rays7 [n, 7] = origin, direction, t_max -> bool [n]: some surface lies within [t_min, t_max] of the
        ray (the any-hit walk of render_ao's occlusion rays; kernel 1: reference order, 2: the accel)."""
        r = np.ascontiguousarray(rays7, dtype=np.float64).reshape(-1, 7)
        out = np.zeros(r.shape[0], dtype=np.float64)
        _chk(self.L.rt_debug_occluded_device(self.h, int(device), int(kernel), r.shape[0], r.ctypes.data_as(_dp), float(t_min), out.ctypes.data_as(_dp)))
        return out != 0.0

    def debug_sppm_trace(self, camera, width, height, iteration=0, photons_per_iter=1, max_bounces=4096, seed=1, capacity=(0, 0), rows=None,
                         photons=True, points=True, device=0):
        """rt_debug_sppm_trace_device: the photon pass and the eye pass of iteration `iteration` of render_sppm's pre-pass, through the
        render's own light table, variant choice, launches and grow-and-retry -> dict(global [n, 9], caustic [n, 9] = {position, power,
        norm} in the device's order, points [width * height, 7] = {valid, p, bsdf}, n_global, n_caustic, S, photon_launches, variant:
        bit 0 accel, 1 LDS tables, 2 nested chain walk, 3 MEDIA, unit_zero).  capacity = the device stores' initial photons (global,
        caustic; 0 = the render's); rows = the host buffers' rows (default: sized by a first call where the defaults are too few);
        photons=False / points=False skips that pass (its outputs are None)."""
        io = rt_debug_sppm_trace()
        io.width, io.height, io.iteration, io.photons_per_iter, io.max_bounces = int(width), int(height), int(iteration), int(photons_per_iter), int(max_bounces)
        io.seed, io.capacity_global, io.capacity_caustic = int(seed), int(capacity[0]), int(capacity[1])
        pts = np.zeros((int(width) * int(height), 7)) if points else None
        if points:
            io.points = pts.ctypes.data_as(_dp)
        sized = rows is not None
        rows = tuple(int(r) for r in rows) if sized else (8 * int(photons_per_iter) + 1024, 2 * int(photons_per_iter) + 1024)
        while True:
            g = np.zeros((rows[0], 9)) if photons else None
            c = np.zeros((rows[1], 9)) if photons else None
            if photons:
                io.global_, io.global_rows = g.ctypes.data_as(_dp), rows[0]
                io.caustic, io.caustic_rows = c.ctypes.data_as(_dp), rows[1]
            rc = self.L.rt_debug_sppm_trace_device(self.h, C.byref(camera.c), int(device), C.byref(io))
            if rc == -1 and not sized and photons and (io.n_global > rows[0] or io.n_caustic > rows[1]):  # RT_ERR_ARG with the counts: size a second call
                rows, sized = (max(rows[0], int(io.n_global)), max(rows[1], int(io.n_caustic))), True
                continue
            break
        if rc != -2:  # RT_ERR_UNIT_ZERO is a result here: every output is written
            _chk(rc)
        return {"global": g[:io.n_global].copy() if photons else None, "caustic": c[:io.n_caustic].copy() if photons else None, "points": pts,
                "n_global": int(io.n_global), "n_caustic": int(io.n_caustic), "S": int(io.shift), "photon_launches": int(io.photon_launches),
                "variant": int(io.variant), "unit_zero": rc == -2}

    def debug_light_sample(self, o_light, keys, device=0):
        """rt_debug_light_sample_device: [n, 4] = origin, object light index; keys uint64 [n, 3] -> [n, 6] = direction, unit-zero status,
        the next draw's two 32-bit halves"""
        x = np.ascontiguousarray(o_light, dtype=np.float64).reshape(-1, 4)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(x.shape[0], 3)
        out = np.zeros((x.shape[0], 6), dtype=np.float64)
        _chk(self.L.rt_debug_light_sample_device(self.h, int(device), x.shape[0], x.ctypes.data_as(_dp), k.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 out.ctypes.data_as(_dp)))
        return out

    def debug_light_pdf(self, rays, device=0, n_lights=None):
        """rt_debug_light_pdf_device: rays [n, 6] = origin, direction -> [n, L]: the pdf of each of the L object lights, in list order"""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n_lights = getattr(self, "n_lights", None) if n_lights is None else int(n_lights)
        if n_lights is None:  # (a scene from a file: the caller knows its light list)
            raise ValueError("debug_light_pdf: pass n_lights, the length of the scene's object light list")
        out = np.zeros((r.shape[0], max(1, n_lights)), dtype=np.float64)  # (a scene without lights is refused)
        _chk(self.L.rt_debug_light_pdf_device(self.h, int(device), r.shape[0], r.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out


AREA_TRI_DTYPE = np.dtype([("a", "<f8", 3), ("e0", "<f8", 3), ("e1", "<f8", 3), ("n", "<f8", 3), ("area2", "<f8"), ("q", "<u4"), ("light", "<i4")])
assert AREA_TRI_DTYPE.itemsize == C.sizeof(rt_area_tri) == 112


def load_scene_file(path, commit=True):
    """rt_scene_load_file: returns (World, Camera) for data/<name>.json|.yaml.  commit=False: rt_scene_parse_file, the same scene left
    uncommitted (set a background or lights, then World.commit())."""
    L = lib()
    h = C.c_void_p()
    cam = rt_camera()
    fn = L.rt_scene_load_file if commit else L.rt_scene_parse_file
    _chk(fn(os.fsencode(path), C.byref(h), C.byref(cam)))
    return World(h), Camera.from_struct(cam)


def select_scene(cube_obj_path, aspect_ratio=1.0, bvh_seed=1, commit=True):
    """scene.rs:114-116 select_scene(_index) == cornell_box_scene(): returns (World, Camera); commit=False leaves it uncommitted."""
    w = World()
    cam = rt_camera()
    _chk(w.L.rt_scene_cornell_box(w.h, os.fsencode(cube_obj_path), float(aspect_ratio), int(bvh_seed), C.byref(cam)))
    if commit:
        w.commit()
    return w, Camera.from_struct(cam)


def set_tuning(**fields):
    """rt_tuning_set: measurement / test hooks (process-wide; the library reads no environment variable).
    set_tuning() with no arguments restores the automatic defaults."""
    t = rt_tuning()
    lib().rt_tuning_default(C.byref(t))
    for k, v in fields.items():
        if not hasattr(t, k):
            raise TypeError("unknown rt_tuning field %r" % k)
        setattr(t, k, v)
    _chk(lib().rt_tuning_set(C.byref(t)))


def release_workspaces():
    """rt_release_workspaces: free the idle per-device render workspaces; returns the bytes released."""
    return int(lib().rt_release_workspaces())


def debug_schedule(tiles_owned, n_waves, s_begin, s_end, sub_spp=8, job_units=2):
    """rt_debug_schedule: (rounds, levels) with levels = [(first round, first unit, first sample, samples per unit, units per job), ...] and the
    closing row (rounds, units, s_end, 0, 0) last.  Host logic only."""
    out = (C.c_int * 25)()
    rounds = _chk(lib().rt_debug_schedule(int(tiles_owned), int(n_waves), int(s_begin), int(s_end), int(sub_spp), int(job_units), out))
    rows = [tuple(out[5 * i:5 * i + 5]) for i in range(5)]
    n = next(i for i, r in enumerate(rows) if r[3] == 0)
    return rounds, rows[:n + 1]


def debug_grid_shape(lo, hi, n):
    """rt_debug_grid_shape: (cell, (dim0, dim1, dim2)) of the uniform grid build_grid lays over n photons with the bounding box [lo, hi].
    Host logic only."""
    cell = C.c_double()
    dim = (C.c_int32 * 3)()
    _chk(lib().rt_debug_grid_shape(_arr3(lo), _arr3(hi), int(n), C.byref(cell), dim))
    return cell.value, tuple(dim)


def debug_sppm_gather(global_photons, caustic_photons, points, stats, k_global, k_caustic, alpha, S, n_emitted, device=0, grids=True):
    """rt_debug_sppm_gather_device: one iteration of the render's SPPM gather.  global_photons [n, 9], caustic_photons [n, 9] =
    {position, power, norm} (either may be empty), points [m, 7] = {valid, p, bsdf}, stats [m, 10] = the state before the iteration ->
    dict(stats [m, 10] after it, estimates [m, 6], unit_zero, grid_global, grid_caustic); a grid = dict(lo, cell, dim, cell_start, index),
    the last two None for an empty map or with grids=False."""
    maps = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 9) for a in (global_photons, caustic_photons)]
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 7)
    st = np.array(stats, dtype=np.float64).reshape(-1, 10)
    if len(st) != len(pts):
        raise ValueError("stats and points must have the same number of rows")
    est = np.zeros((len(pts), 6))
    io = rt_debug_sppm_gather()
    io.n_global, io.n_caustic, io.m = len(maps[0]), len(maps[1]), len(pts)
    io.global_ = maps[0].ctypes.data_as(_dp) if len(maps[0]) else None
    io.caustic = maps[1].ctypes.data_as(_dp) if len(maps[1]) else None
    io.points, io.stats, io.estimates = pts.ctypes.data_as(_dp), st.ctypes.data_as(_dp), est.ctypes.data_as(_dp)
    io.k_global, io.k_caustic, io.alpha, io.shift, io.n_emitted = int(k_global), int(k_caustic), float(alpha), int(S), float(n_emitted)
    tables = []
    for g, ph in ((io.grid_global, maps[0]), (io.grid_caustic, maps[1])):
        cs = ix = None
        if grids and len(ph) and np.isfinite(ph[:, 0:3]).all():
            _, dim = debug_grid_shape(ph[:, 0:3].min(axis=0), ph[:, 0:3].max(axis=0), len(ph))
            cs = np.zeros(dim[0] * dim[1] * dim[2] + 1, dtype=np.uint32)
            ix = np.zeros(len(ph), dtype=np.uint32)
            g.cell_start, g.cell_start_capacity = cs.ctypes.data_as(C.POINTER(C.c_uint32)), len(cs)
            g.index, g.index_capacity = ix.ctypes.data_as(C.POINTER(C.c_uint32)), len(ix)
        tables.append((cs, ix))
    rc = lib().rt_debug_sppm_gather_device(int(device), C.byref(io))
    if rc != -2:  # RT_ERR_UNIT_ZERO is a result here: every output is written
        _chk(rc)
    out = {"stats": st, "estimates": est, "unit_zero": rc == -2}
    for name, g, (cs, ix) in (("grid_global", io.grid_global, tables[0]), ("grid_caustic", io.grid_caustic, tables[1])):
        out[name] = {"lo": np.array(g.lo[:]), "cell": g.cell, "dim": tuple(g.dim[:]), "cell_start": cs, "index": ix}
    return out


def _regions(regions):
    """[(x0, y0, x1, y1), ...] -> (rt_region array, count); an empty list still has an address, so the library answers n_regions == 0 itself"""
    regions = [rt_region(*[int(v) for v in r]) for r in regions]
    return (rt_region * max(1, len(regions)))(*regions), len(regions)


def region_doubles(params, regions):
    """rt_region_doubles: the f64 count of the packed output of World.render_regions_device"""
    arr, n = _regions(regions)
    return int(_chk(lib().rt_region_doubles(C.byref(params), n, arr)))


def region_tiles(width, height, regions):
    """rt_region_tiles: the image tiles (ty * tiles_x + tx, ascending, unique; int32 array) a region call of a width x height frame traces.
    Host only."""
    p = default_params(width=width, height=height)
    arr, n = _regions(regions)
    out = np.zeros(_chk(lib().rt_region_tiles(C.byref(p), n, arr, 0, None)), dtype=np.int32)
    _chk(lib().rt_region_tiles(C.byref(p), n, arr, out.size, out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def tiles_owned(params):
    return int(lib().rt_tiles_owned(C.byref(params)))


def tiles_total(params):
    return int(lib().rt_tiles_total(C.byref(params)))


def assemble_frame_device(params, d_gathered_ptr, tiles_per_rank_stride, d_frame_ptr, stream_ptr=None):
    _chk(lib().rt_assemble_frame_device(C.byref(params), C.c_void_p(d_gathered_ptr), int(tiles_per_rank_stride),
                                        C.c_void_p(d_frame_ptr), C.c_void_p(stream_ptr or 0)))


def accum_finalize(params, state):
    """rt_accum_finalize: the frame [H, W, 3] of a complete host-held accumulator state (World.render_accumulate)"""
    out = np.zeros((params.height, params.width, 3), dtype=np.float64)
    _chk(lib().rt_accum_finalize(C.byref(params), state.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
    return out


def accum_finalize_device(params, d_accum_ptr, d_tiles_ptr, stream_ptr=None):
    """rt_accum_finalize_device: d_tiles = d_accum / params.spp (the end of a resumable render, World.render_accumulate_device)"""
    _chk(lib().rt_accum_finalize_device(C.byref(params), C.c_void_p(d_accum_ptr), C.c_void_p(d_tiles_ptr), C.c_void_p(stream_ptr or 0)))


def denoise_config(**fields):
    """rt_default_denoise_config with `fields` (rt_denoise_config names) set"""
    c = rt_denoise_config()
    lib().rt_default_denoise_config(C.byref(c))
    for k, v in fields.items():
        if k == "reserved" or not hasattr(c, k):
            raise TypeError("unknown denoiser setting %r" % k)
        setattr(c, k, v)
    return c


def luminance(rgb):
    """l = (0.2126 r + 0.7152 g) + 0.0722 b, the filter's luminance (same operation order)"""
    rgb = np.asarray(rgb, dtype=np.float64)
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


def denoise(rgb, variance=None, aov=None, return_variance=False, symmetric=False, **cfg):
    """rt_denoise, or with symmetric=True rt_denoise_sym (the luminance stop sqrt(v_p + v_q), which keeps the frame's mean; it needs a
    variance): the a-trous filter on host arrays.  rgb [H, W, 3]; variance [H, W] of each pixel's mean luminance (None: no luminance
    weight); aov [H, W, 8] from World.render_aov (None: no guides).  cfg: rt_denoise_config fields (iterations, normal_power_log2,
    sigma_depth, sigma_albedo, sigma_luma, eps, guides).  Returns the filtered [H, W, 3], and with return_variance also the filtered variance."""
    c = denoise_config(**cfg)
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb must be [H, W, 3]")
    h, w = rgb.shape[:2]
    var_p = aov_p = None
    if variance is not None:
        variance = np.ascontiguousarray(variance, dtype=np.float64)
        if variance.shape != (h, w):
            raise ValueError("variance must be [H, W]")
        var_p = variance.ctypes.data_as(_dp)
    if aov is not None:
        aov = np.ascontiguousarray(aov, dtype=np.float64)
        if aov.shape != (h, w, 8):
            raise ValueError("aov must be [H, W, 8]")
        aov_p = aov.ctypes.data_as(_dp)
    out = np.zeros_like(rgb)
    out_var = np.zeros((h, w), dtype=np.float64) if return_variance else None
    fn = lib().rt_denoise_sym if symmetric else lib().rt_denoise
    _chk(fn(C.byref(c), w, h, rgb.ctypes.data_as(_dp), var_p, aov_p, out.ctypes.data_as(_dp), out_var.ctypes.data_as(_dp) if out_var is not None else None))
    return (out, out_var) if return_variance else out


def denoise_device(width, height, d_rgb_ptr, d_out_ptr, d_variance_ptr=None, d_aov_ptr=None, d_out_variance_ptr=None, stream_ptr=None,
                   symmetric=False, **cfg):
    """rt_denoise_device (symmetric=True: rt_denoise_sym_device): raw device pointers (e.g. torch tensor .data_ptr()) of the current device;
    returns when the passes are done"""
    c = denoise_config(**cfg)
    fn = lib().rt_denoise_sym_device if symmetric else lib().rt_denoise_device
    _chk(fn(C.byref(c), int(width), int(height), C.c_void_p(d_rgb_ptr), C.c_void_p(d_variance_ptr or 0), C.c_void_p(d_aov_ptr or 0),
            C.c_void_p(d_out_ptr), C.c_void_p(d_out_variance_ptr or 0), C.c_void_p(stream_ptr or 0)))


def temporal_config(**fields):
    """rt_default_temporal_config with `fields` (rt_temporal_config names) set"""
    c = rt_temporal_config()
    lib().rt_default_temporal_config(C.byref(c))
    for k, v in fields.items():
        if k == "reserved" or not hasattr(c, k):
            raise TypeError("unknown temporal setting %r" % k)
        setattr(c, k, v)
    return c


def _camera_frame(cam):
    """an rt_camera_frame of a Camera, or the rt_camera_frame itself"""
    return cam if isinstance(cam, rt_camera_frame) or cam is None else cam.frame()


def temporal_accumulate(rgb, aov, cam_cur, variance=None, prev_history=None, prev_aov=None, cam_prev=None, return_variance=False, **cfg):
    """rt_temporal_accumulate: one step of temporal accumulation with reprojection on host arrays (include/rtamd.h has the rule).
    rgb [H, W, 3], aov [H, W, 8] from World.render_aov, variance [H, W] (None: none) of the current frame; cam_cur / cam_prev a Camera or an
    rt_camera_frame; prev_history [H, W, 6], prev_aov [H, W, 8] and cam_prev of the previous frame, all None on a first frame.  cfg:
    rt_temporal_config fields.  Returns the history [H, W, 6] = {r, g, b, m1, m2, n}, and with return_variance also the variance [H, W] of
    the accumulated mean luminance."""
    c = temporal_config(**cfg)
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb must be [H, W, 3]")
    h, w = rgb.shape[:2]

    def arr(a, shape, name):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError("%s must be %r" % (name, list(shape)))
        return a, a.ctypes.data_as(_dp)
    aov, aov_p = arr(aov, (h, w, 8), "aov")
    variance, var_p = arr(variance, (h, w), "variance")
    prev_history, hist_p = arr(prev_history, (h, w, 6), "prev_history")
    prev_aov, paov_p = arr(prev_aov, (h, w, 8), "prev_aov")
    f_cur, f_prev = _camera_frame(cam_cur), _camera_frame(cam_prev)
    out = np.zeros((h, w, 6), dtype=np.float64)
    out_var = np.zeros((h, w), dtype=np.float64) if return_variance else None
    _chk(lib().rt_temporal_accumulate(C.byref(c), w, h, C.byref(f_prev) if f_prev is not None else None,
                                      C.byref(f_cur) if f_cur is not None else None, rgb.ctypes.data_as(_dp), aov_p, var_p, hist_p, paov_p,
                                      out.ctypes.data_as(_dp), out_var.ctypes.data_as(_dp) if out_var is not None else None))
    return (out, out_var) if return_variance else out


def temporal_accumulate_device(width, height, cam_cur, d_rgb_ptr, d_aov_ptr, d_out_history_ptr, d_variance_ptr=None, d_prev_history_ptr=None,
                               d_prev_aov_ptr=None, cam_prev=None, d_out_variance_ptr=None, stream_ptr=None, **cfg):
    """rt_temporal_accumulate_device: raw device pointers (e.g. torch tensor .data_ptr()) of the current device; returns when the step is done"""
    c = temporal_config(**cfg)
    f_cur, f_prev = _camera_frame(cam_cur), _camera_frame(cam_prev)
    _chk(lib().rt_temporal_accumulate_device(C.byref(c), int(width), int(height), C.byref(f_prev) if f_prev is not None else None, C.byref(f_cur),
                                             C.c_void_p(d_rgb_ptr), C.c_void_p(d_aov_ptr), C.c_void_p(d_variance_ptr or 0),
                                             C.c_void_p(d_prev_history_ptr or 0), C.c_void_p(d_prev_aov_ptr or 0), C.c_void_p(d_out_history_ptr),
                                             C.c_void_p(d_out_variance_ptr or 0), C.c_void_p(stream_ptr or 0)))


class Sequence:
    """rt_sequence: frames of one world and size on one device, accumulated over time.  The history, the previous guides
    and the previous camera stay on the device; cfg: rt_temporal_config fields."""

    RETURNS = ("rgb", "accum", "history", "variance", "stats")

    def __init__(self, world, width, height, device=-1, **cfg):
        self.L = lib()
        self.world, self.width, self.height = world, int(width), int(height)
        self.h = C.c_void_p()
        c = temporal_config(**cfg)
        _chk(self.L.rt_sequence_create(self.width, self.height, int(device), C.byref(c), C.byref(self.h)))
        self._next_seed_offset = 0

    def __del__(self):
        if getattr(self, "h", None):
            self.L.rt_sequence_destroy(self.h)
            self.h = None

    @property
    def frames(self):
        """frames since the last reset"""
        return _chk(self.L.rt_sequence_frames(self.h))

    def reset(self):
        """the next frame resets every pixel"""
        _chk(self.L.rt_sequence_reset(self.h))

    def frame(self, camera, spp, seed=None, aov_spp=4, luma_mode=1, denoise=None, returns=("rgb",), world=None, max_depth=50, t_min=1e-3,
              kernel=0, integrator=0):
        """rt_sequence_frame: one frame of `spp` samples through `camera`, accumulated into the history and filtered (luma_mode 1:
        rt_denoise_sym, 0: rt_denoise, -1: no filter).  seed None: 1 + the number of frames this Sequence has rendered, so that frames do
        not repeat their noise.  denoise: a dict of rt_denoise_config fields.  returns: which of "rgb" (the frame), "accum" (the unfiltered
        accumulation [H, W, 3]), "history" [H, W, 6], "variance" [H, W], "stats" come back, in that order (a single name: that array)."""
        names = (returns,) if isinstance(returns, str) else tuple(returns)
        for n in names:
            if n not in self.RETURNS:
                raise ValueError("unknown output %r (one of %s)" % (n, ", ".join(self.RETURNS)))
        if seed is None:
            seed = 1 + self._next_seed_offset
        w = world if world is not None else self.world
        p = default_params(width=self.width, height=self.height, spp=int(spp), max_depth=max_depth, t_min=t_min, seed=int(seed), kernel=kernel,
                           integrator=integrator)
        dn = denoise_config(**(denoise or {}))
        shapes = {"rgb": (self.height, self.width, 3), "accum": (self.height, self.width, 3), "history": (self.height, self.width, 6),
                  "variance": (self.height, self.width)}
        out = {k: np.zeros(shapes[k], dtype=np.float64) for k in shapes if k == "rgb" or k in names}
        ptr = lambda k: out[k].ctypes.data_as(_dp) if k in out else None
        st = rt_stats()
        _chk(self.L.rt_sequence_frame(self.h, w.h, C.byref(camera.c), C.byref(p), C.byref(dn), int(luma_mode), int(aov_spp), ptr("rgb"), ptr("accum"),
                                      ptr("history"), ptr("variance"), C.byref(st)))
        self._next_seed_offset += 1
        out["stats"] = st.as_dict()
        res = tuple(out[n] for n in names)
        return res[0] if isinstance(returns, str) else res


def tonemap_u8(rgb):
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    out = np.zeros(a.shape, dtype=np.uint8)
    _chk(lib().rt_tonemap_u8(a.ctypes.data_as(_dp), a.size, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def write_png(path, rgb_u8):
    a = np.ascontiguousarray(rgb_u8, dtype=np.uint8)
    _chk(lib().rt_write_png(os.fsencode(path), a.shape[1], a.shape[0], a.ctypes.data_as(C.POINTER(C.c_uint8))))


def debug_rng(seed, pixel, sample, n, device=True):
    out = (C.c_uint64 * n)()
    fn = lib().rt_debug_rng_device if device else lib().rt_debug_rng_host
    _chk(fn(int(seed), int(pixel), int(sample), n, out))
    return [int(x) for x in out]


def debug_rng_floats(seed, pixel, sample, n, lo=-1.0, hi=1.0, device=True):
    """(first n gen::<f64>(), first n gen_range(lo..hi)) of stream (seed, pixel, sample), computed by the device or the host code"""
    g, r = (C.c_double * n)(), (C.c_double * n)()
    _chk(lib().rt_debug_rng_floats(int(seed), int(pixel), int(sample), n, float(lo), float(hi), 1 if device else 0, g, r))
    return [float(x) for x in g], [float(x) for x in r]


def debug_math(op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        bp = b.ctypes.data_as(_dp)
    _chk(lib().rt_debug_math_device(op, a.size, a.ctypes.data_as(_dp), bp, out.ctypes.data_as(_dp)))
    return out
