"""ctypes mirror of include/glaze_abi.h and loader for libglaze_hip.so.

This is the Python-side stub of the C ABI (the Rust `-sys` binding a glaze maintainer would write
is shown in INTEGRATION.md).  There is NO fallback: if the shared library (and with it the HIP
code object) is missing, importing the render path raises.
"""
import ctypes as C
import os

NAME_MAX = 256

# status codes
OK, E_IO, E_INVALID_INPUT, E_INVALID_DATA, E_ARG, E_DEVICE, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6

CAMERA_PERSPECTIVE, CAMERA_ORTHOGRAPHIC = 0, 1
MAT_FLAT, MAT_LAMBERT, MAT_MIRROR, MAT_GLASS, MAT_METAL, MAT_FROSTED, MAT_UBER = range(7)
LIGHT_OMNI, LIGHT_SUN, LIGHT_AREA, LIGHT_SKY = range(4)
TEX_GRAY, TEX_RGBA_SRGB, TEX_RGBA_NORM = 1, 2, 3
DIRECT, PATH_TRACE = 0, 1


class Vertex(C.Structure):
    _fields_ = [("vv", C.c_float * 3), ("vn", C.c_float * 3), ("vt", C.c_float * 2)]


class Mesh(C.Structure):
    _fields_ = [("id", C.c_uint16), ("material", C.c_uint16), ("index_offset", C.c_uint32), ("index_count", C.c_uint32)]


class Transform(C.Structure):
    _fields_ = [("m", C.c_float * 16)]


class MeshInstance(C.Structure):
    _fields_ = [("mesh_id", C.c_uint16), ("transform_id", C.c_uint16)]


class Camera(C.Structure):
    _fields_ = [("type", C.c_uint32), ("position", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3),
                ("fovx_or_scale", C.c_float), ("near_plane", C.c_float), ("far_plane", C.c_float)]


class Material(C.Structure):
    _fields_ = [("mtype", C.c_uint8), ("metal", C.c_uint8), ("diffuse_mul", C.c_uint8 * 3), ("emissive_col", C.c_uint8 * 3),
                ("has_emissive", C.c_uint8), ("_pad", C.c_uint8 * 3),
                ("ior", C.c_float), ("roughness_mul", C.c_float), ("metalness_mul", C.c_float), ("anisotropy", C.c_float),
                ("diffuse", C.c_uint16), ("roughness", C.c_uint16), ("metalness", C.c_uint16), ("normal", C.c_uint16),
                ("opacity", C.c_uint16), ("_pad2", C.c_uint16), ("name", C.c_char * NAME_MAX)]


class Light(C.Structure):
    _fields_ = [("ltype", C.c_uint32), ("position", C.c_float * 3), ("direction", C.c_float * 3), ("resource_id", C.c_uint32),
                ("intensity", C.c_float), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float), ("roll_deg", C.c_float),
                ("color", C.c_float * 16), ("name", C.c_char * NAME_MAX)]


class Texture(C.Structure):
    _fields_ = [("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("mip_levels", C.c_uint32),
                ("pixels", C.c_void_p), ("name", C.c_char * NAME_MAX)]


class Meta(C.Structure):
    _fields_ = [("scene_centre", C.c_float * 3), ("scene_radius", C.c_float), ("exposure", C.c_float)]


class SceneDescC(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("n_vertices", C.c_uint64),
                ("indices", C.c_void_p), ("n_indices", C.c_uint64),
                ("meshes", C.c_void_p), ("n_meshes", C.c_uint32),
                ("transforms", C.c_void_p), ("n_transforms", C.c_uint32),
                ("instances", C.c_void_p), ("n_instances", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32),
                ("lights", C.c_void_p), ("n_lights", C.c_uint32),
                ("textures", C.c_void_p), ("n_textures", C.c_uint32),
                ("camera", C.c_void_p), ("meta", C.c_void_p)]


class SerializeDescC(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("n_vertices", C.c_uint64), ("indices", C.c_void_p), ("n_indices", C.c_uint64),
                ("meshes", C.c_void_p), ("n_meshes", C.c_uint64), ("transforms", C.c_void_p), ("n_transforms", C.c_uint64),
                ("instances", C.c_void_p), ("n_instances", C.c_uint64), ("cameras", C.c_void_p), ("n_cameras", C.c_uint64),
                ("textures", C.c_void_p), ("n_textures", C.c_uint64), ("materials", C.c_void_p), ("n_materials", C.c_uint64),
                ("lights", C.c_void_p), ("n_lights", C.c_uint64), ("meta", C.c_void_p)]


class SceneInfo(C.Structure):
    _fields_ = [("n_vertices", C.c_uint64), ("n_triangles", C.c_uint64), ("n_world_triangles", C.c_uint64),
                ("n_instances", C.c_uint32), ("n_materials", C.c_uint32), ("n_lights", C.c_uint32), ("n_rt_lights", C.c_uint32),
                ("n_textures", C.c_uint32), ("bvh_nodes", C.c_uint32), ("bvh_depth", C.c_uint32),
                ("bvh_sah_cost", C.c_float), ("build_ms", C.c_float), ("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3),
                ("bvh_grid_lo", C.c_float * 3), ("bvh_grid_cell", C.c_float * 3),
                ("as_levels", C.c_uint32), ("n_as_triangles", C.c_uint32), ("as_bytes", C.c_uint64),
                ("bvh_nodes8", C.c_uint32), ("_reserved", C.c_uint32)]


GEOMETRY_REFIT, GEOMETRY_REBUILD = 0, 1
SKIN_LINEAR, SKIN_DUAL_QUATERNION = 0, 1


class GeometryUpdateInfo(C.Structure):
    """glz_geometry_update_info"""
    _fields_ = [("mode", C.c_uint32), ("meshes_touched", C.c_uint32), ("update_ms", C.c_float), ("box_area", C.c_float),
                ("box_area_built", C.c_float)]


class RenderStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("samples", C.c_uint64), ("render_ms", C.c_double),
                ("trace_closest_ms", C.c_double), ("shade_ms", C.c_double), ("trace_shadow_ms", C.c_double), ("other_ms", C.c_double),
                ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("closest_nodes", C.c_uint64), ("closest_tris", C.c_uint64), ("shadow_nodes", C.c_uint64), ("shadow_tris", C.c_uint64),
                ("hits", C.c_uint64), ("fresh_paths", C.c_uint64), ("phase", C.c_uint64 * 12),
                ("tex_fetches", C.c_uint64), ("tex_bytes", C.c_uint64), ("alpha_tex_bytes", C.c_uint64), ("light_samples", C.c_uint64),
                ("sky_samples", C.c_uint64)]


class DenoiseParams(C.Structure):
    """glz_denoise_params; the defaults are the library's (glz_renderer_set_denoise(r, NULL))"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("normal_power_log2", C.c_uint32),
                ("eps_albedo", C.c_float), ("eps_depth", C.c_float), ("eps_color", C.c_float)]
    DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_depth=1.0, normal_power_log2=6, eps_albedo=1.0 / 256.0, eps_depth=1e-3, eps_color=1e-8)

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown denoise parameter(s): %s" % ", ".join(sorted(unknown)))
        super().__init__(**dict(self.DEFAULTS, **kw))


class DespeckleParams(C.Structure):
    """glz_despeckle_params; the defaults are the library's (glz_renderer_set_despeckle(r, enabled, NULL))"""
    _fields_ = [("radius", C.c_uint32), ("trim", C.c_uint32), ("ratio", C.c_float)]
    DEFAULTS = dict(radius=2, trim=2, ratio=8.0)

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown despeckle parameter(s): %s" % ", ".join(sorted(unknown)))
        super().__init__(**dict(self.DEFAULTS, **kw))


class ReprojectParams(C.Structure):
    """glz_reproject_params; the default is the library's (params NULL)"""
    _fields_ = [("depth_tolerance", C.c_float)]
    DEFAULTS = dict(depth_tolerance=1.0 / 64.0)

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown reproject parameter(s): %s" % ", ".join(sorted(unknown)))
        super().__init__(**dict(self.DEFAULTS, **kw))


class PreviousState(C.Structure):
    """glz_previous_state: what glz_renderer_read_motion_from / glz_renderer_reproject_from take for the previous frame"""
    _fields_ = [("camera", C.c_void_p), ("transforms", C.c_void_p), ("n_transforms", C.c_uint32), ("vertices", C.c_void_p),
                ("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32)]


class Skin(C.Structure):
    """glz_skin"""
    _fields_ = [("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32), ("joints", C.c_void_p), ("weights", C.c_void_p), ("n_bones", C.c_uint32)]


class Pose(C.Structure):
    """glz_pose"""
    _fields_ = [("skin", C.c_int), ("bones", C.c_void_p), ("n_bones", C.c_uint32)]


class MorphTarget(C.Structure):
    """glz_morph_target"""
    _fields_ = [("vertices", C.c_void_p), ("d_position", C.c_void_p), ("d_normal", C.c_void_p), ("n", C.c_uint32)]


class Morph(C.Structure):
    """glz_morph"""
    _fields_ = [("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32), ("targets", C.c_void_p), ("n_targets", C.c_uint32), ("skin", C.c_int)]


class MorphWeights(C.Structure):
    """glz_morph_weights"""
    _fields_ = [("morph", C.c_int), ("weights", C.c_void_p), ("n_targets", C.c_uint32)]


class Animation(C.Structure):
    """glz_animation"""
    _fields_ = [("morphs", C.c_void_p), ("n_morphs", C.c_uint32), ("poses", C.c_void_p), ("n_poses", C.c_uint32)]


class Skeleton(C.Structure):
    """glz_skeleton"""
    _fields_ = [("skin", C.c_int), ("n_bones", C.c_uint32), ("parents", C.c_void_p), ("inverse_bind", C.c_void_p), ("root", C.c_float * 16)]


class Clip(C.Structure):
    """glz_clip"""
    _fields_ = [("skeleton", C.c_int), ("n_keys", C.c_uint32), ("times", C.c_void_p), ("translations", C.c_void_p), ("rotations", C.c_void_p),
                ("scales", C.c_void_p), ("morph_weights", C.c_void_p), ("n_targets", C.c_uint32)]


class Play(C.Structure):
    """glz_play"""
    _fields_ = [("clip", C.c_int), ("time", C.c_float)]


class Normals(C.Structure):
    """glz_normals"""
    _fields_ = [("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32), ("groups", C.c_void_p)]


MORPH_LDS_TARGETS = 1024   # kMorphLdsTargets (csrc/kernels.h): the morph kernels stage the weight table in LDS up to this many targets
AOV_NORMAL_DEPTH, AOV_ALBEDO_INSTANCE = 0, 1
GUIDE_FIRST_HIT, GUIDE_THROUGH_SPECULAR, GUIDE_MAX_BOUNCES = 0, 1, 8
DENOISE_MAX_ITERATIONS, DENOISE_MAX_NORMAL_POWER_LOG2 = 8, 31
POST_TIMING_SLOTS = 3 + DENOISE_MAX_ITERATIONS     # glz_debug_post_timing

DRAW_CALLBACK = C.CFUNCTYPE(None, C.c_void_p)

# every symbol include/glaze_abi.h declares: name -> (restype, argtypes)
_P = C.c_void_p
PROTOTYPES = {
    "glz_last_error": (C.c_char_p, []),
    "glz_version": (C.c_char_p, []),
    "glz_last_status": (C.c_int, []),
    "glz_parse": (_P, [C.c_char_p]),
    "glz_parsed_free": (None, [_P]),
    "glz_parsed_vertices": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_meshes": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_indices": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_transforms": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_instances": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_cameras": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_materials": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_lights": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_parsed_textures": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_serialize": (C.c_int, [C.c_char_p, _P]),
    "glz_convert_obj": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, _P]),
    "glz_save_image": (C.c_int, [C.c_char_p, _P, C.c_uint32, C.c_uint32]),
    "glz_parsed_update": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P]),
    "glz_parsed_meta": (C.c_int, [_P, _P]),
    "glz_converted_file": (C.c_int, [C.c_char_p]),
    "glz_instance_create": (_P, [C.c_int]),
    "glz_instance_destroy": (None, [_P]),
    "glz_instance_device": (C.c_int, [_P]),
    "glz_instance_stream": (_P, [_P]),
    "glz_instance_set_bvh_builder": (C.c_int, [_P, C.c_int]),
    "glz_scene_create": (_P, [_P, _P]),
    "glz_scene_create_from_desc": (_P, [_P, _P]),
    "glz_scene_destroy": (None, [_P]),
    "glz_scene_get_info": (C.c_int, [_P, _P]),
    "glz_scene_camera": (C.c_int, [_P, _P]),
    "glz_renderer_create": (_P, [_P, _P, C.c_uint32, C.c_uint32]),
    "glz_renderer_destroy": (None, [_P]),
    "glz_renderer_set_integrator": (C.c_int, [_P, C.c_int]),
    "glz_renderer_set_exposure": (C.c_int, [_P, C.c_float]),
    "glz_renderer_update_camera": (C.c_int, [_P, _P]),
    "glz_renderer_change_resolution": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "glz_renderer_change_scene": (C.c_int, [_P, _P]),
    "glz_renderer_update_materials_and_lights": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32]),
    "glz_renderer_refresh_binded_textures": (C.c_int, [_P, _P, C.c_uint32]),
    "glz_renderer_update_transforms": (C.c_int, [_P, _P, C.c_uint32]),
    "glz_renderer_update_vertices": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int]),
    "glz_renderer_geometry_update_info": (C.c_int, [_P, _P]),
    "glz_renderer_add_skin": (C.c_int, [_P, _P]),
    "glz_renderer_remove_skin": (C.c_int, [_P, C.c_int]),
    "glz_renderer_pose_skins": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "glz_renderer_read_vertices": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "glz_renderer_read_motion_posed": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "glz_renderer_reproject_posed": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P]),
    "glz_host_skin": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "glz_renderer_set_skin_blend": (C.c_int, [_P, C.c_int, C.c_int]),
    "glz_renderer_skin_blend": (C.c_int, [_P, C.c_int]),
    "glz_host_skin_dq": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "glz_host_bone_dual_quats": (C.c_int, [_P, C.c_uint32, _P]),
    "glz_renderer_add_morph": (C.c_int, [_P, _P]),
    "glz_renderer_remove_morph": (C.c_int, [_P, C.c_int]),
    "glz_renderer_animate": (C.c_int, [_P, _P, C.c_int]),
    "glz_renderer_read_motion_animated": (C.c_int, [_P, _P, _P, _P]),
    "glz_renderer_reproject_animated": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "glz_host_morph": (C.c_int, [_P, C.c_uint64, _P, C.c_uint32, _P, _P]),
    "glz_debug_morph_timing": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "glz_renderer_add_skeleton": (C.c_int, [_P, _P]),
    "glz_renderer_remove_skeleton": (C.c_int, [_P, C.c_int]),
    "glz_renderer_add_clip": (C.c_int, [_P, _P]),
    "glz_renderer_remove_clip": (C.c_int, [_P, C.c_int]),
    "glz_renderer_play": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "glz_host_clip_bones": (C.c_int, [_P, _P, C.c_float, _P, _P]),
    "glz_debug_clip_bones": (C.c_int, [_P, _P, _P, _P]),
    "glz_debug_clip_timing": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P]),
    "glz_renderer_add_normals": (C.c_int, [_P, _P]),
    "glz_renderer_remove_normals": (C.c_int, [_P, C.c_int]),
    "glz_host_vertex_normals": (C.c_int, [_P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    "glz_host_weld_groups": (C.c_int, [_P, C.c_uint64, _P]),
    "glz_debug_normals_timing": (C.c_int, [_P, C.c_int, C.c_uint32, _P, _P]),
    "glz_debug_read_leaf_records": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_debug_read_tlas_instances": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_debug_instance_boxes": (C.c_int64, [_P, C.c_int, C.c_uint64, _P, _P]),
    "glz_debug_box_kernel_ms": (C.c_float, [_P]),
    "glz_host_instance_boxes": (C.c_int64, [_P, C.c_uint64, _P, _P]),
    "glz_renderer_wait_idle": (C.c_int, [_P]),
    "glz_renderer_steps_per_sample": (C.c_uint32, [_P]),
    "glz_renderer_draw": (C.c_int, [_P, C.c_size_t, _P, _P, _P]),
    "glz_renderer_restart": (C.c_int, [_P]),
    "glz_renderer_step": (C.c_int, [_P, C.c_uint32]),
    "glz_renderer_read_rgba8": (C.c_int, [_P, _P]),
    "glz_renderer_set_seed": (C.c_int, [_P, C.c_uint64]),
    "glz_renderer_set_depth": (C.c_int, [_P, C.c_uint32]),
    "glz_renderer_read_hdr": (C.c_int, [_P, _P]),
    "glz_renderer_read_result": (C.c_int, [_P, _P]),
    "glz_renderer_launch_constants": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "glz_renderer_push_constants": (C.c_int, [_P, _P]),
    "glz_renderer_set_partition": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "glz_renderer_set_chains": (C.c_int, [_P, C.c_uint32]),
    "glz_renderer_export_device": (C.c_int, [_P, C.c_int, _P]),
    "glz_renderer_packed_pixels": (C.c_uint64, [_P, C.c_uint32, C.c_uint32]),
    "glz_renderer_export_packed": (C.c_int, [_P, C.c_int, _P]),
    "glz_renderer_scatter_packed": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "glz_renderer_scatter_packed_all": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, _P]),
    "glz_renderer_tonemap_device": (C.c_int, [_P, _P, _P]),
    "glz_renderer_enable_counters": (C.c_int, [_P, C.c_int]),
    "glz_renderer_get_stats": (C.c_int, [_P, _P]),
    "glz_debug_trace_closest": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_float, _P, _P, _P, _P, _P]),
    "glz_debug_trace_any": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_float, _P]),
    "glz_debug_read_derivatives": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_debug_read_rt_materials": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_debug_read_rt_lights": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_debug_read_sky": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_debug_read_bvh": (C.c_int64, [_P, _P, C.c_int64, _P, C.c_int64]),
    "glz_debug_read_bvh8": (C.c_int64, [_P, _P, C.c_int64]),
    "glz_host_launch_constants": (C.c_int, [C.c_uint64, C.c_uint32, _P, _P]),
    "glz_host_push_constants": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "glz_host_chain_owner": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    "glz_host_build_sah": (C.c_int, [C.c_uint32, _P, _P, _P, _P]),
    "glz_host_srgb8_thresholds": (C.c_int, [_P]),
    "glz_debug_tonemap": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "glz_debug_sample_texture": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, _P]),
    "glz_debug_detmath": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_uint64]),
    "glz_debug_color_to_spec": (C.c_int, [_P, C.c_int, _P, C.c_uint64, _P]),
    "glz_debug_scene_set_spectra": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "glz_debug_bsdf_value": (C.c_int,[_P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, _P, _P]),
    "glz_debug_bsdf_sample": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, _P, _P, _P]),
    "glz_debug_light_sample": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, C.c_float, _P, _P, _P, _P]),
    "glz_debug_read_texture_level": (C.c_int64, [_P, C.c_uint32, C.c_uint32, _P, C.c_int64, _P, _P]),
    "glz_host_mip_level": (C.c_int64, [_P, C.c_uint32, _P, C.c_int64, _P, _P]),
    "glz_renderer_set_texture_lod": (C.c_int, [_P, C.c_int]),
    "glz_debug_rccl_selftest": (C.c_int, [_P, C.c_uint64, _P]),
    "glz_instance_set_as_levels": (C.c_int, [_P, C.c_int]),
    "glz_renderer_set_devices": (C.c_int, [_P, _P, C.c_int]),
    "glz_renderer_set_launch_mode": (C.c_int, [_P, C.c_int]),
    "glz_renderer_set_node_width": (C.c_int, [_P, C.c_int]),
    "glz_renderer_node_width": (C.c_int, [_P]),
    "glz_renderer_launch_mode": (C.c_int, [_P]),
    "glz_renderer_device_count": (C.c_int, [_P]),
    "glz_renderer_device_scene_info": (C.c_int, [_P, C.c_int, _P]),
    "glz_rccl_version": (C.c_int, []),
    "glz_host_tile_owner": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    "glz_renderer_read_aov": (C.c_int, [_P, C.c_int, _P]),
    "glz_renderer_set_denoise": (C.c_int, [_P, _P]),
    "glz_renderer_read_denoised": (C.c_int, [_P, _P, _P]),
    "glz_renderer_set_despeckle": (C.c_int, [_P, C.c_int, _P]),
    "glz_renderer_despeckle": (C.c_int, [_P, _P]),
    "glz_renderer_read_despeckled": (C.c_int, [_P, _P, _P]),
    "glz_renderer_read_motion": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "glz_renderer_reproject": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P]),
    "glz_renderer_read_motion_from": (C.c_int, [_P, _P, _P]),
    "glz_renderer_reproject_from": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "glz_debug_motion_timing_from": (C.c_int, [_P, _P, _P]),
    "glz_debug_skin_timing": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "glz_host_project_constants": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "glz_host_project_points": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P]),
    "glz_host_reproject": (C.c_int, [C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "glz_debug_project_points": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P]),
    "glz_debug_motion_timing": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "glz_debug_reproject": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _P]),
    "glz_host_despeckle": (C.c_int, [C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.c_int, _P]),
    "glz_debug_despeckle": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.c_int, _P, _P]),
    "glz_host_denoise": (C.c_int, [C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    "glz_debug_denoise": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    "glz_debug_camera_rays": (C.c_int, [_P, C.c_float, C.c_float, _P, _P]),
    "glz_debug_post_timing": (C.c_int, [_P, _P]),
    "glz_renderer_set_guide_mode": (C.c_int, [_P, C.c_int, C.c_uint32]),
    "glz_renderer_guide_mode": (C.c_int, [_P, _P]),
    "glz_debug_guide_chain": (C.c_int, [_P, C.c_uint32, _P, _P, _P]),
    "glz_host_traversal_offsets_fit": (C.c_int, [C.c_uint64] * 6),
    "glz_host_sky_row_pairs": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "glz_host_sky_bracket_table": (C.c_int, [_P, C.c_uint64, _P]),
    "glz_host_sky_cdf_search": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_uint64, _P, _P]),
    "glz_host_texel_wrap": (C.c_int, [_P, C.c_uint64, C.c_int32, _P]),
    "glz_host_conductor_finite": (C.c_int, [_P, _P, _P]),
    "glz_host_metal_spectra": (C.c_int, [C.c_uint32, _P, _P]),
}

_LIB = None


def library_path():
    # GLAZE_HIP_LIB selects another build of the same library (kernel tuning experiments); never a different backend
    return os.environ.get("GLAZE_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libglaze_hip.so")


class GlazeLibraryMissing(ImportError):
    pass


def lib():
    """Loads libglaze_hip.so (built in-tree by `__graft_entry__.build()` / glaze_amd/csrc/Makefile)."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise GlazeLibraryMissing(
                "%s not found: build it with `make -C glaze_amd/csrc` (there is no CPU fallback for the render path)" % path)
        handle = C.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)   # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


class GlazeError(IOError):
    def __init__(self, status, message):
        super().__init__("%s (status %d)" % (message, status))
        self.status = status


def last_error():
    l = lib()
    msg = l.glz_last_error()
    return GlazeError(l.glz_last_status(), msg.decode("utf8", "replace") if msg else "unknown error")


def check(status):
    if status < 0:
        raise last_error()
    return status
