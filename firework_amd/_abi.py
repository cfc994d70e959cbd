"""ctypes mirror of include/firework_hip.h (the C ABI).  Field order and types must match the header."""
import ctypes as C

FW_ABI_VERSION = 8
FW_INIT_NO_ARENA = 0xFFFFFFFFFFFFFFFF   # fw_init: no path arena (the first render sizes its own)
FW_MAX_SEGMENTS = 11

# fw_status
FW_OK = 0
FW_ERR_BAD_ARG = -1
FW_ERR_EMPTY_SCENE = -2
FW_ERR_NAN_BBOX = -3
FW_ERR_MESH_NORMALS = -4
FW_ERR_MESH_UVS = -5
FW_ERR_UNSUPPORTED = -6
FW_ERR_HIP = -7
FW_ERR_NO_DEVICE = -8
FW_ERR_BVH_DEPTH = -9
FW_ERR_OOM = -10

# kinds
FW_TEX_CONSTANT, FW_TEX_CHECKER, FW_TEX_PERLIN, FW_TEX_TURBULENCE, FW_TEX_MARBLE, FW_TEX_IMAGE = range(6)
FW_MAT_LAMBERTIAN, FW_MAT_METAL, FW_MAT_DIELECTRIC, FW_MAT_EMISSIVE, FW_MAT_ISOTROPIC, FW_MAT_GGX = range(6)   # 5: GgxMat
(FW_SHAPE_SPHERE, FW_SHAPE_XYRECT, FW_SHAPE_XZRECT, FW_SHAPE_YZRECT, FW_SHAPE_RECT3D,
 FW_SHAPE_TRIANGLE_MESH, FW_SHAPE_CONSTANT_MEDIUM, FW_SHAPE_CONE, FW_SHAPE_CYLINDER, FW_SHAPE_DISK) = range(10)
FW_ENV_COLOR, FW_ENV_SKY, FW_ENV_HDR = range(3)
FW_RNG_CTR, FW_RNG_LCG = 0, 1
FW_FLAG_TIME_KERNELS = 1
FW_FLAG_COUNT_DEPOSITS = 2
FW_FLAG_LIGHT_SAMPLING = 4   # next-event estimation with MIS
FW_LIGHT_RECORD_FLOATS = 16  # fw_selftest_lights
FW_FLAG_ENV_SAMPLING = 8     # importance sampling of an HDR environment map
FW_ENV_SAMPLE_FLOATS = 6     # fw_selftest_env_sample
FW_FLAG_ALL_EMITTERS = 16    # with FW_FLAG_LIGHT_SAMPLING: every emitting primitive, picked by power
FW_EMITTER_RECORD_FLOATS = 5  # fw_selftest_emitters
FW_EMITTER_SAMPLE_FLOATS = 9  # fw_selftest_emitter_sample
FW_GGX_IN_FLOATS, FW_GGX_OUT_FLOATS = 15, 11  # fw_selftest_ggx
FW_NO_HIT = 0xFFFFFFFF   # fw_hit.object of a miss
FW_LIGHT_POINT, FW_LIGHT_SPOT, FW_LIGHT_DIRECTIONAL = range(3)   # fw_light_kind
FW_MAX_LIGHTS = 65536

f32, i32, u32, u64 = C.c_float, C.c_int32, C.c_uint32, C.c_uint64


class fw_vec3(C.Structure):
    _fields_ = [("x", f32), ("y", f32), ("z", f32)]


class fw_rotor3(C.Structure):
    _fields_ = [("s", f32), ("xy", f32), ("xz", f32), ("yz", f32)]


class fw_texture(C.Structure):
    _fields_ = [("kind", i32), ("color", fw_vec3), ("scale", f32), ("depth", u32), ("odd", i32), ("even", i32),
                ("img_w", u32), ("img_h", u32), ("img_rgb8", C.POINTER(C.c_uint8))]


class fw_material(C.Structure):
    _fields_ = [("kind", i32), ("texture", i32), ("albedo", fw_vec3), ("roughness", f32), ("ref_idx", f32)]


class fw_shape(C.Structure):
    _fields_ = [("kind", i32), ("material", i32), ("radius", f32), ("height", f32), ("phi_max", f32),
                ("inner_radius", f32), ("a_min", f32), ("a_max", f32), ("b_min", f32), ("b_max", f32), ("k", f32), ("flip_normal", i32),
                ("pos", fw_vec3), ("size", fw_vec3),
                ("verts", C.POINTER(f32)), ("n_verts", u32), ("indices", C.POINTER(u32)), ("n_indices", u32),
                ("normals", C.POINTER(f32)), ("uvs", C.POINTER(f32)),
                ("inner", i32), ("density", f32)]


class fw_object(C.Structure):
    _fields_ = [("shape", i32), ("position", fw_vec3), ("rotation", fw_rotor3), ("flip_normals", i32)]


class fw_environment(C.Structure):
    _fields_ = [("kind", i32), ("color", fw_vec3), ("zenith", fw_vec3), ("horizon", fw_vec3),
                ("hdr_w", u32), ("hdr_h", u32), ("hdr_rgb", C.POINTER(f32))]


class fw_scene_desc(C.Structure):
    _fields_ = [("objects", C.POINTER(fw_object)), ("n_objects", u32),
                ("shapes", C.POINTER(fw_shape)), ("n_shapes", u32),
                ("materials", C.POINTER(fw_material)), ("n_materials", u32),
                ("textures", C.POINTER(fw_texture)), ("n_textures", u32),
                ("environment", fw_environment)]


class fw_light(C.Structure):
    _fields_ = [("kind", i32), ("position", fw_vec3), ("direction", fw_vec3), ("intensity", fw_vec3), ("cos_inner", f32), ("cos_outer", f32)]


class fw_camera_settings(C.Structure):
    _fields_ = [("cam_pos", fw_vec3), ("look_at", fw_vec3), ("vfov", f32), ("aperture", f32), ("focus_dist", f32)]


class fw_render_params(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("samples", u32), ("gamma", f32), ("use_bvh", i32),
                ("multithreaded", i32), ("camera", fw_camera_settings), ("seed", u64), ("rng_mode", i32),
                ("pixel_ids", C.POINTER(u32)), ("n_pixels", u32), ("paths_per_batch", u32), ("flags", u32),
                ("outputs_on_device", i32), ("stream", C.c_void_p)]


class fw_stats(C.Structure):
    _fields_ = [("samples", u64), ("rays", u64), ("rays_per_depth", u64 * FW_MAX_SEGMENTS),
                ("algorithmic_bytes", u64), ("ms_scene", C.c_double), ("ms_render", C.c_double),
                ("ms_raygen", C.c_double), ("ms_extend", C.c_double), ("ms_shade", C.c_double),
                ("ms_accumulate", C.c_double),
                ("n_extend_launches", u32), ("n_shade_launches", u32), ("n_batches", u32),
                ("tlas_nodes", u32), ("blas_nodes", u32), ("reserved", u32),
                ("bytes_raygen", u64), ("bytes_extend", u64), ("bytes_shade", u64), ("bytes_accumulate", u64),
                ("deposits", u64), ("parked_rays", u64), ("ms_wall", C.c_double), ("ms_d2h", C.c_double)]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class fw_hit(C.Structure):
    _fields_ = [("t", f32), ("point", fw_vec3), ("normal", fw_vec3), ("u", f32), ("v", f32),
                ("material", u32), ("object", u32), ("prim", u32)]


class fw_trace_params(C.Structure):
    _fields_ = [("use_bvh", i32), ("flags", u32), ("seed", u64), ("key_base", u32), ("rays_per_batch", u32),
                ("on_device", i32), ("stream", C.c_void_p)]


class fw_render_rays_params(C.Structure):
    _fields_ = [("n_rays", u32), ("first_sample", u32), ("samples", u32), ("per_sample_rays", i32), ("keys", C.POINTER(u32)),
                ("key_base", u32), ("seed", u64), ("use_bvh", i32), ("gamma", f32), ("paths_per_batch", u32), ("flags", u32),
                ("on_device", i32), ("stream", C.c_void_p)]


# fw_denoise (include/firework_hip.h): the filter's constants and its parameters
FW_DENOISE_EPS = 0.01
FW_DENOISE_NORMAL_POW = 128
FW_DENOISE_PLANE = 0.01
FW_DENOISE_LUM = 128.0
FW_DENOISE_ITERATIONS = 5
FW_DENOISE_MAX_ITERATIONS = 10


class fw_denoise_params(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("iterations", u32), ("gamma", f32), ("device", i32), ("on_device", i32),
                ("stream", C.c_void_p)]


# fw_temporal (include/firework_hip.h): the reprojection's constants and its parameters
FW_TEMPORAL_NORMAL_COS = 0.9
FW_TEMPORAL_PLANE = 0.02
FW_TEMPORAL_MIN_TAP = 1e-3


class fw_temporal_params(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("camera", fw_camera_settings), ("prev_camera", fw_camera_settings), ("samples", u32),
                ("max_history", f32), ("device", i32), ("on_device", i32), ("stream", C.c_void_p)]


# camera models on the device (include/firework_hip.h: fw_model_rays, fw_render_model, fw_render_model_aovs)
FW_MODEL_PANORAMA, FW_MODEL_ORTHOGRAPHIC, FW_MODEL_FISHEYE = range(3)


class fw_camera_model(C.Structure):
    _fields_ = [("kind", i32), ("width", u32), ("height", u32), ("camera", fw_camera_settings), ("view_height", C.c_double),
                ("fov", C.c_double), ("jitter", i32), ("seed", u64), ("chunk_samples", u32)]


# irradiance probes on the device (include/firework_hip.h: fw_probe_rays, fw_probe_project, fw_bake_probes)
class fw_probe_set(C.Structure):
    _fields_ = [("n_probes", u32), ("positions", C.POINTER(f32)), ("directions", u32), ("jitter", i32), ("seed", u64), ("chunk_probes", u32)]


# baked probes read back (include/firework_hip.h: fw_probe_irradiance, fw_probe_shade)
FW_PROBE_WRAP = 1


class fw_probe_grid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("counts", u32 * 3), ("flags", u32)]


class fw_probe_shade_params(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("gamma", f32), ("device", i32), ("on_device", i32), ("stream", C.c_void_p)]


# probe visibility (include/firework_hip.h: fw_probe_depth_reduce, fw_bake_probe_depth, fw_probe_irradiance_vis, fw_probe_shade_vis)
class fw_probe_depth(C.Structure):
    _fields_ = [("resolution", u32), ("sharpness_log2", u32), ("max_distance", f32)]


# the four prototypes (argument types; every one returns int), applied by _lib.load
PROBE_DEPTH_PROTOTYPES = {
    "fw_probe_depth_reduce": [C.c_int, C.POINTER(fw_probe_depth), u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_probe_depth": [C.c_void_p, C.POINTER(fw_probe_set), C.POINTER(fw_probe_depth), C.POINTER(fw_trace_params), u32, u32, C.c_void_p,
                            C.c_void_p, C.POINTER(fw_stats)],
    "fw_probe_irradiance_vis": [C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p, f32, C.c_int, u32, C.c_void_p,
                                C.c_void_p, u32, C.c_void_p, C.c_int, C.c_void_p],
    "fw_probe_shade_vis": [C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p, f32, C.POINTER(fw_probe_shade_params),
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}


# lightmaps on the device (include/firework_hip.h: fw_lightmap_texels, fw_lightmap_rays, fw_lightmap_reduce, fw_lightmap_dilate,
# fw_bake_lightmap)
class fw_lightmap(C.Structure):
    _fields_ = [("verts", C.POINTER(f32)), ("n_verts", u32), ("indices", C.POINTER(u32)), ("n_indices", u32), ("normals", C.POINTER(f32)),
                ("uvs", C.POINTER(f32)), ("position", fw_vec3), ("rotation", fw_rotor3), ("flip_normals", i32), ("width", u32), ("height", u32),
                ("directions", u32), ("jitter", i32), ("seed", u64), ("bias", f32), ("flip", i32), ("chunk_texels", u32)]


# ambient occlusion (include/firework_hip.h: fw_ao_rays, fw_ao_reduce, fw_bake_ao)
class fw_ao(C.Structure):
    _fields_ = [("directions", u32), ("falloff", u32), ("radius", f32), ("bias", f32), ("jitter", u32), ("chunk_points", u32), ("seed", u64)]


# the three prototypes (argument types; every one returns int), applied by _lib.load
AO_PROTOTYPES = {
    "fw_ao_rays": [C.POINTER(fw_ao), C.c_int, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_ao_reduce": [C.c_int, C.POINTER(fw_ao), u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_ao": [C.c_void_p, C.POINTER(fw_ao), C.POINTER(fw_trace_params), u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p,
                   C.c_void_p, C.POINTER(fw_stats)],
}


# direct light of point, spot and directional lights at surface points (include/firework_hip.h: fw_direct_rays, fw_direct_reduce,
# fw_bake_direct)
class fw_direct(C.Structure):
    _fields_ = [("lobe", u32), ("face_view", u32), ("bias", f32), ("chunk_points", u32)]


# the three prototypes (argument types; every one returns int), applied by _lib.load
DIRECT_PROTOTYPES = {
    "fw_direct_rays": [C.POINTER(fw_direct), C.c_void_p, u32, C.c_int, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p,
                       C.c_void_p, C.c_int, C.c_void_p],
    "fw_direct_reduce": [C.c_int, C.POINTER(fw_direct), C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_direct": [C.c_void_p, C.POINTER(fw_direct), C.POINTER(fw_trace_params), u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32,
                       C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.POINTER(fw_stats)],
}


# final gather (include/firework_hip.h: fw_hit_surface, fw_gather_reduce, fw_bake_gather)
FW_GATHER_DIRECT = 1


class fw_gather(C.Structure):
    _fields_ = [("directions", u32), ("jitter", u32), ("bias", f32), ("direct_bias", f32), ("flags", u32), ("chunk_points", u32), ("seed", u64)]


# the three prototypes (argument types; every one returns int), applied by _lib.load
GATHER_PROTOTYPES = {
    "fw_hit_surface": [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_int, C.c_void_p],
    "fw_gather_reduce": [C.c_int, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_gather": [C.c_void_p, C.POINTER(fw_gather), C.POINTER(fw_trace_params), C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_depth),
                       C.c_void_p, f32, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p, C.c_void_p,
                       C.POINTER(fw_stats)],
}


# reflection gather (include/firework_hip.h: fw_reflect_rays, fw_reflect_reduce, fw_bake_reflect)
FW_REFLECT_DIRECT = 1


class fw_reflect(C.Structure):
    _fields_ = [("directions", u32), ("jitter", u32), ("bias", f32), ("direct_bias", f32), ("flags", u32), ("chunk_points", u32), ("seed", u64)]


# the three prototypes (argument types; every one returns int), applied by _lib.load
REFLECT_PROTOTYPES = {
    "fw_reflect_rays": [C.POINTER(fw_reflect), C.c_int, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_int, C.c_void_p],
    "fw_reflect_reduce": [C.c_int, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_reflect": [C.c_void_p, C.POINTER(fw_reflect), C.POINTER(fw_trace_params), C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_depth),
                        C.c_void_p, f32, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p,
                        C.c_void_p, C.POINTER(fw_stats)],
}


# sphere and rectangle emitters sampled at surface points (include/firework_hip.h: fw_scene_area_lights, fw_area_rays, fw_area_reduce,
# fw_area_mask, fw_bake_area); FW_GATHER_NO_LIGHTS is fw_gather.flags' bit for the gather's complement
FW_GATHER_NO_LIGHTS = 4


class fw_area(C.Structure):
    _fields_ = [("samples", u32), ("jitter", u32), ("bias", f32), ("chunk_points", u32), ("seed", u64)]


# the five prototypes (argument types; every one returns int), applied by _lib.load
AREA_PROTOTYPES = {
    "fw_scene_area_lights": [C.c_void_p, C.c_void_p, u32, C.POINTER(u32)],
    "fw_area_rays": [C.POINTER(fw_area), C.c_void_p, u32, C.c_int, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                     C.c_void_p],
    "fw_area_reduce": [C.c_int, u32, C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_area_mask": [C.c_int, C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_area": [C.c_void_p, C.POINTER(fw_area), C.POINTER(fw_trace_params), u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p,
                     C.c_void_p, C.POINTER(fw_stats)],
}


# every emitter sampled at surface points, picked by power (include/firework_hip.h: fw_selftest_emitters_records, fw_scene_emitters,
# fw_emitters_cdf, fw_emitters_rays, fw_emitters_reduce, fw_bake_emitters); FW_GATHER_NO_EMITTERS is fw_gather.flags' bit for the
# gather's complement
FW_GATHER_NO_EMITTERS = 16
FW_EMITTERS_RECORD_FLOATS = 16


class fw_emitters(C.Structure):
    _fields_ = [("samples", u32), ("jitter", u32), ("bias", f32), ("chunk_points", u32), ("seed", u64)]


# the six prototypes (argument types; every one returns int), applied by _lib.load
EMITTERS_PROTOTYPES = {
    "fw_selftest_emitters_records": [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.POINTER(u32)],
    "fw_scene_emitters": [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.POINTER(u32)],
    "fw_emitters_cdf": [C.c_void_p, u32, C.c_void_p, C.POINTER(C.c_double)],
    "fw_emitters_rays": [C.POINTER(fw_emitters), C.c_void_p, C.c_void_p, u32, C.c_int, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p,
                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_emitters_reduce": [C.c_int, u32, C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                           C.c_void_p],
    "fw_bake_emitters": [C.c_void_p, C.POINTER(fw_emitters), C.POINTER(fw_trace_params), u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32,
                         C.c_void_p, C.c_void_p, C.POINTER(fw_stats)],
}


# SunSky: an analytic sun-and-sky environment (include/firework_hip.h: fw_check_sky, fw_sky_map, fw_sky_radiance, fw_sky_sun)
FW_SKY_DISC = 1


class fw_sky(C.Structure):
    _fields_ = [("sun_elevation", f32), ("sun_azimuth", f32), ("turbidity", f32), ("sun_irradiance", fw_vec3), ("sun_radius", f32),
                ("altitude", f32), ("ground_albedo", fw_vec3), ("view_steps", u32), ("light_steps", u32), ("sun_samples", u32), ("flags", u32)]


# the four prototypes (argument types; every one returns int), applied by _lib.load
SKY_PROTOTYPES = {
    "fw_check_sky": [C.POINTER(fw_sky)],
    "fw_sky_map": [C.POINTER(fw_sky), C.c_int, u32, u32, C.c_void_p, C.c_int, C.c_void_p],
    "fw_sky_radiance": [C.POINTER(fw_sky), C.c_int, u32, C.c_void_p, u32, C.c_void_p, C.c_int, C.c_void_p],
    "fw_sky_sun": [C.POINTER(fw_sky), C.POINTER(fw_light)],
}


# probe relocation and classification (include/firework_hip.h: fw_probe_survey, fw_probe_relocate_step, fw_relocate_probes,
# fw_probe_irradiance_placed, fw_probe_shade_placed)
class fw_probe_relocate(C.Structure):
    _fields_ = [("min_front", f32), ("back_fraction", f32), ("max_offset", f32 * 3)]


# the five prototypes (argument types; every one returns int), applied by _lib.load
PROBE_PLACE_PROTOTYPES = {
    "fw_probe_survey": [C.c_int, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_probe_relocate_step": [C.c_int, C.POINTER(fw_probe_relocate), u32, u32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "fw_relocate_probes": [C.c_void_p, C.POINTER(fw_probe_set), C.POINTER(fw_probe_relocate), C.POINTER(fw_trace_params), u32, u32, C.c_void_p,
                           C.c_void_p, C.POINTER(fw_stats)],
    "fw_probe_irradiance_placed": [C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p, f32, C.c_void_p, C.c_int, u32,
                                   C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_int, C.c_void_p],
    "fw_probe_shade_placed": [C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p, f32, C.c_void_p,
                              C.POINTER(fw_probe_shade_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}


# probe radiance maps (include/firework_hip.h: fw_probe_radiance_reduce, fw_probe_radiance_prefilter, fw_bake_probe_radiance,
# fw_probe_radiance_lookup, fw_probe_shade_glossy)
FW_PROBE_RADIANCE_MAX_LEVELS = 4


class fw_probe_radiance(C.Structure):
    _fields_ = [("resolution", u32), ("sharpness_log2", u32), ("levels", u32), ("roughness", f32 * FW_PROBE_RADIANCE_MAX_LEVELS)]


# the five prototypes (argument types; every one returns int), applied by _lib.load
PROBE_RADIANCE_PROTOTYPES = {
    "fw_probe_radiance_reduce": [C.c_int, C.POINTER(fw_probe_radiance), u32, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_probe_radiance_prefilter": [C.c_int, C.POINTER(fw_probe_radiance), u32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_bake_probe_radiance": [C.c_void_p, C.POINTER(fw_probe_set), C.POINTER(fw_probe_radiance), C.POINTER(fw_render_rays_params), u32, u32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fw_stats)],
    "fw_probe_radiance_lookup": [C.POINTER(fw_probe_grid), C.POINTER(fw_probe_radiance), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p, f32,
                                 C.c_void_p, C.c_int, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_probe_shade_glossy": [C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_radiance), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p,
                              f32, C.c_void_p, C.POINTER(fw_probe_shade_params), C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p,
                              C.c_void_p],
}


# the split sum's BRDF term: a GGX albedo table (include/firework_hip.h: fw_check_ggx_quad, fw_ggx_terms, fw_ggx_table,
# fw_ggx_table_lookup, fw_probe_shade_split)
FW_SPLIT_ENERGY = 1


class fw_ggx_quad(C.Structure):
    _fields_ = [("m1", u32), ("m2", u32)]


# the five prototypes (argument types; every one returns int), applied by _lib.load
GGX_TABLE_PROTOTYPES = {
    "fw_check_ggx_quad": [C.POINTER(fw_ggx_quad)],
    "fw_ggx_terms": [C.POINTER(fw_ggx_quad), C.c_int, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_ggx_table": [C.POINTER(fw_ggx_quad), C.c_int, u32, u32, C.c_void_p, C.c_int, C.c_void_p],
    "fw_ggx_table_lookup": [C.c_int, u32, u32, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "fw_probe_shade_split": [C.POINTER(fw_probe_grid), C.c_void_p, C.POINTER(fw_probe_radiance), C.c_void_p, C.POINTER(fw_probe_depth), C.c_void_p,
                             f32, C.c_void_p, C.POINTER(fw_probe_shade_params), C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32, u32,
                             C.c_void_p, C.c_void_p, C.c_void_p],
}


def vec3(v):
    return fw_vec3(float(v[0]), float(v[1]), float(v[2]))
