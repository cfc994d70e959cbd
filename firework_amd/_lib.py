"""Loads libfirework_hip.so (HIP kernels + C ABI) and wraps its entry points.

There is deliberately NO fallback: if the shared library is missing, fails to load, or no GPU is
visible, every call raises.  The CPU oracle under oracle/ is test infrastructure and is never
reachable from here.
"""
import ctypes as C
import math
import os
import re

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FIREWORK_LIB") or os.path.join(_HERE, "lib", "libfirework_hip.so")
_lib = None


class FireworkError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"firework_hip error {status}: {detail}")


def load(preload=False, device=None):
    """Load the native library once.  torch is imported first so that the process holds exactly one
    HIP runtime (torch bundles libamdhip64.so.7; our library's DT_NEEDED resolves to that copy).
    Loading makes no HIP call (ABI v7).  preload=True also runs fw_init on `device` (default: LOCAL_RANK's, else 0) — context, code
    objects, kernel handles and the default path arena — which is what the CLI and bench.py want before their timed regions."""
    global _lib
    if _lib is not None:
        if preload:
            init(device)
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FireworkError(A.FW_ERR_NO_DEVICE, f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`"
                            " (or `make`) — there is no CPU fallback")
    if os.environ.get("FIREWORK_NO_TORCH", "0") != "1":
        import torch  # noqa: F401  (plumbing: one HIP runtime per process, streams, torch.distributed)
    lib = C.CDLL(LIB_PATH)
    lib.fw_abi_version.restype = C.c_int
    lib.fw_strerror.restype = C.c_char_p
    lib.fw_strerror.argtypes = [C.c_int]
    lib.fw_last_error.restype = C.c_char_p
    lib.fw_device_count.restype = C.c_int
    lib.fw_scene_create.restype = C.c_int
    lib.fw_scene_create.argtypes = [C.POINTER(A.fw_scene_desc), C.c_int, C.POINTER(C.c_void_p)]
    lib.fw_scene_update.restype = C.c_int
    lib.fw_scene_update.argtypes = [C.c_void_p, C.POINTER(A.fw_scene_desc)]
    lib.fw_scene_set_lights.restype = C.c_int
    lib.fw_scene_set_lights.argtypes = [C.c_void_p, C.POINTER(A.fw_light), C.c_uint32]
    lib.fw_check_lights.restype = C.c_int
    lib.fw_check_lights.argtypes = [C.POINTER(A.fw_light), C.c_uint32]
    lib.fw_scene_destroy.restype = None
    lib.fw_scene_destroy.argtypes = [C.c_void_p]
    lib.fw_render.restype = C.c_int
    lib.fw_render.argtypes = [C.c_void_p, C.POINTER(A.fw_render_params), C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(A.fw_stats)]
    lib.fw_render_scene.restype = C.c_int
    lib.fw_render_scene.argtypes = [C.POINTER(A.fw_scene_desc), C.POINTER(A.fw_render_params), C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_render_scene_tiled.restype = C.c_int
    lib.fw_render_scene_tiled.argtypes = [C.POINTER(A.fw_scene_desc), C.POINTER(A.fw_render_params), C.POINTER(C.c_int), C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_render_progressive.restype = C.c_int
    lib.fw_render_progressive.argtypes = [C.c_void_p, C.POINTER(A.fw_render_params), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_release_workspace.restype = None
    lib.fw_release_workspace.argtypes = [C.c_int]
    lib.fw_selftest_arith.restype = C.c_int
    lib.fw_selftest_arith.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fw_selftest_libm.restype = C.c_int
    lib.fw_selftest_libm.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fw_set_option.restype = C.c_int
    lib.fw_set_option.argtypes = [C.c_char_p, C.c_char_p]
    lib.fw_selftest_wide_bvh.restype = C.c_int
    lib.fw_selftest_lights.restype = C.c_int
    lib.fw_selftest_lights.argtypes = [C.POINTER(A.fw_scene_desc), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.fw_selftest_wide_bvh.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.fw_selftest_env_dist.restype = C.c_int
    lib.fw_selftest_env_dist.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_double)]
    lib.fw_selftest_env_sample.restype = C.c_int
    lib.fw_selftest_env_sample.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.fw_selftest_emitters.restype = C.c_int
    lib.fw_selftest_emitters.argtypes = [C.POINTER(A.fw_scene_desc), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.fw_selftest_emitter_sample.restype = C.c_int
    lib.fw_selftest_emitter_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.fw_selftest_ggx.restype = C.c_int
    lib.fw_selftest_ggx.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.fw_selftest_bvh_build.restype = C.c_int
    lib.fw_selftest_bvh_build.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.fw_selftest_bvh_trees.restype = C.c_int
    lib.fw_selftest_bvh_trees.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.fw_init.restype = C.c_int
    lib.fw_init.argtypes = [C.c_int, C.c_uint64]
    lib.fw_trace_rays.restype = C.c_int
    lib.fw_trace_rays.argtypes = [C.c_void_p, C.POINTER(A.fw_trace_params), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_camera_rays.restype = C.c_int
    lib.fw_camera_rays.argtypes = [C.POINTER(A.fw_render_params), C.c_int, C.c_uint32, C.c_void_p]
    lib.fw_render_adaptive.restype = C.c_int
    lib.fw_render_adaptive.argtypes = [C.c_void_p, C.POINTER(A.fw_render_params), C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_render_views.restype = C.c_int
    lib.fw_render_views.argtypes = [C.c_void_p, C.POINTER(A.fw_render_params), C.POINTER(A.fw_camera_settings), C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_render_rays.restype = C.c_int
    lib.fw_render_rays.argtypes = [C.c_void_p, C.POINTER(A.fw_render_rays_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_render_aovs.restype = C.c_int
    lib.fw_render_aovs.argtypes = [C.c_void_p, C.POINTER(A.fw_render_params), C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_model_rays.restype = C.c_int
    lib.fw_model_rays.argtypes = [C.POINTER(A.fw_camera_model), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    lib.fw_render_model.restype = C.c_int
    lib.fw_render_model.argtypes = [C.c_void_p, C.POINTER(A.fw_camera_model), C.POINTER(A.fw_render_rays_params), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_render_model_aovs.restype = C.c_int
    lib.fw_render_model_aovs.argtypes = [C.c_void_p, C.POINTER(A.fw_camera_model), C.POINTER(A.fw_render_params), C.c_void_p,
                                         C.POINTER(A.fw_stats)]
    lib.fw_probe_rays.restype = C.c_int
    lib.fw_probe_rays.argtypes = [C.POINTER(A.fw_probe_set), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    lib.fw_probe_project.restype = C.c_int
    lib.fw_probe_project.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.fw_bake_probes.restype = C.c_int
    lib.fw_bake_probes.argtypes = [C.c_void_p, C.POINTER(A.fw_probe_set), C.POINTER(A.fw_render_rays_params), C.c_uint32, C.c_uint32, C.c_void_p,
                                   C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_probe_irradiance.restype = C.c_int
    lib.fw_probe_irradiance.argtypes = [C.POINTER(A.fw_probe_grid), C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_int, C.c_void_p]
    lib.fw_probe_shade.restype = C.c_int
    lib.fw_probe_shade.argtypes = [C.POINTER(A.fw_probe_grid), C.c_void_p, C.POINTER(A.fw_probe_shade_params), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]
    for name, argtypes in (list(A.PROBE_DEPTH_PROTOTYPES.items()) + list(A.AO_PROTOTYPES.items()) + list(A.PROBE_PLACE_PROTOTYPES.items())
                           + list(A.PROBE_RADIANCE_PROTOTYPES.items()) + list(A.DIRECT_PROTOTYPES.items()) + list(A.SKY_PROTOTYPES.items())
                           + list(A.GGX_TABLE_PROTOTYPES.items()) + list(A.GATHER_PROTOTYPES.items()) + list(A.REFLECT_PROTOTYPES.items())
                           + list(A.AREA_PROTOTYPES.items()) + list(A.EMITTERS_PROTOTYPES.items())):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = argtypes
    lib.fw_lightmap_texels.restype = C.c_int
    lib.fw_lightmap_texels.argtypes = [C.POINTER(A.fw_lightmap), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_void_p]
    lib.fw_lightmap_rays.restype = C.c_int
    lib.fw_lightmap_rays.argtypes = [C.POINTER(A.fw_lightmap), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    lib.fw_lightmap_reduce.restype = C.c_int
    lib.fw_lightmap_reduce.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                       C.c_void_p]
    lib.fw_lightmap_dilate.restype = C.c_int
    lib.fw_lightmap_dilate.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    lib.fw_bake_lightmap.restype = C.c_int
    lib.fw_bake_lightmap.argtypes = [C.c_void_p, C.POINTER(A.fw_lightmap), C.POINTER(A.fw_render_rays_params), C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.POINTER(A.fw_stats)]
    lib.fw_denoise.restype = C.c_int
    lib.fw_denoise.argtypes = [C.POINTER(A.fw_denoise_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fw_debug_kernels.restype = C.c_int
    lib.fw_debug_kernels.argtypes = [C.c_int, C.c_char_p, C.c_uint32]
    lib.fw_temporal.restype = C.c_int
    lib.fw_temporal.argtypes = [C.POINTER(A.fw_temporal_params)] + [C.c_void_p] * 10
    if lib.fw_abi_version() != A.FW_ABI_VERSION:
        raise FireworkError(A.FW_ERR_BAD_ARG, "ABI version mismatch between _abi.py and libfirework_hip.so")
    _lib = lib
    if preload:
        init(device)
    return lib


def init(device=None, arena_bytes=0):
    """fw_init: explicit, idempotent initialisation of one device (default: LOCAL_RANK's, else 0).  arena_bytes 0 = the default
    arena, A.FW_INIT_NO_ARENA = none."""
    lib = load()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0") or 0)
        if device >= max(1, lib.fw_device_count()):
            device = 0
    _check(lib, lib.fw_init(int(device), int(arena_bytes)))


def _check(lib, st):
    if st != A.FW_OK:
        raise FireworkError(st, f"{lib.fw_strerror(st).decode()} | {lib.fw_last_error().decode()}")


def set_option(name, value=None):
    """fw_set_option: one runtime switch of the library (FIREWORK_<NAME>; the environment itself is read once, at load).
    value None = back to the default; name None = back to what the environment said at load time."""
    lib = load()
    _check(lib, lib.fw_set_option(None if name is None else str(name).encode(), None if value is None else str(value).encode()))


class options:
    """with _lib.options(FIREWORK_BVH="median", NO_DEFER="1"): ...  — switches set for the block, defaults restored after it."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            set_option(k, None)
        return False


def last_kernels(device=0):
    """fw_debug_kernels: the names of the walk and shade kernels the last call on `device` launched, e.g. 'k_shade_pl<2,0>' or
    'k_blas_wide<q8,no tris>@12' (@: waves per workgroup of an LDS-resident walk); device -1: every name this build can launch."""
    lib = load()
    n = lib.fw_debug_kernels(int(device), None, 0)
    if n < 0:
        _check(lib, n)
    buf = C.create_string_buffer(n + 1)
    n = lib.fw_debug_kernels(int(device), buf, n + 1)
    if n < 0:
        _check(lib, n)
    text = buf.value.decode()
    return frozenset(re.split(r",(?![^<]*>)", text)) if text else frozenset()      # (a comma inside <> belongs to a name)


def has_ab():
    """True for the A/B build (make ab: -DFW_AB=1), which also carries the measured-slower alternative kernels and their switches."""
    return hasattr(load(), "fw_debug_ab")


def selftest_wide_bvh(boxes, fmt):
    """fw_selftest_wide_bvh (CPU only): wide-node builder + invariant check over (n, 6) float32 item boxes.  -> (violations, stats)"""
    lib = load()
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    bad = C.c_uint32()
    stats = (C.c_uint32 * 4)()
    _check(lib, lib.fw_selftest_wide_bvh(b.ctypes.data, b.shape[0], int(fmt), C.byref(bad), stats))
    return int(bad.value), dict(nodes=int(stats[0]), leaves=int(stats[1]), free_slots=int(stats[2]), depth=int(stats[3]))


def _light_array(lights):
    """(ctypes array or None, n) of a sequence of api lights or fw_light records"""
    recs = [l if isinstance(l, A.fw_light) else l.to_abi() for l in lights]
    return ((A.fw_light * len(recs))(*recs) if recs else None), len(recs)


def check_lights(lights):
    """fw_check_lights (CPU only, no device touched): raises FireworkError for a list fw_scene_set_lights would refuse.  `lights`: api
    PointLight / SpotLight / DirectionalLight objects or _abi.fw_light records"""
    lib = load()
    arr, n = _light_array(lights)
    _check(lib, lib.fw_check_lights(arr, n))


def selftest_lights(scene_desc):
    """fw_selftest_lights (CPU only): the sampled lights of a SceneDesc as FW_FLAG_LIGHT_SAMPLING sees them.  -> list of dicts
    with obj, kind, corners ((4, 3) world corners of a rectangle) or centre + radius (a sphere), area, p_pick"""
    lib = load()
    n = C.c_uint32()
    _check(lib, lib.fw_selftest_lights(scene_desc.ptr(), None, 0, C.byref(n)))
    out = np.zeros((max(1, n.value), A.FW_LIGHT_RECORD_FLOATS), np.float32)
    _check(lib, lib.fw_selftest_lights(scene_desc.ptr(), out.ctypes.data, n.value, C.byref(n)))
    return _light_dicts(out[:n.value])


def _light_dicts(records):
    """fw_selftest_lights' records ((Ln, FW_LIGHT_RECORD_FLOATS) float32) as a list of dicts"""
    lights = []
    for r in records:
        d = dict(obj=int(r[0]), kind=int(r[1]), area=float(r[14]), p_pick=float(r[15]))
        if d["kind"] == A.FW_SHAPE_SPHERE:
            d["centre"], d["radius"] = r[2:5].astype(np.float64), float(r[5])
        else:
            d["corners"] = r[2:14].reshape(4, 3).astype(np.float64)
        lights.append(d)
    return lights


def light_records(scene_desc):
    """fw_selftest_lights' records themselves: (Ln, FW_LIGHT_RECORD_FLOATS) float32, what area_rays takes as `lights` (CPU only)"""
    lib = load()
    n = C.c_uint32()
    _check(lib, lib.fw_selftest_lights(scene_desc.ptr(), None, 0, C.byref(n)))
    out = np.zeros((n.value, A.FW_LIGHT_RECORD_FLOATS), np.float32)
    if n.value:
        _check(lib, lib.fw_selftest_lights(scene_desc.ptr(), out.ctypes.data, n.value, C.byref(n)))
    return out


def selftest_emitters(scene_desc):
    """fw_selftest_emitters (CPU only): the entries of a SceneDesc as FW_FLAG_ALL_EMITTERS sees them.  -> dict of arrays
    obj, prim, kind (int64) and area, weight (float64 of the float32 records), one element per entry"""
    lib = load()
    n = C.c_uint32()
    _check(lib, lib.fw_selftest_emitters(scene_desc.ptr(), None, 0, C.byref(n)))
    out = np.zeros((max(1, n.value), A.FW_EMITTER_RECORD_FLOATS), np.float32)
    _check(lib, lib.fw_selftest_emitters(scene_desc.ptr(), out.ctypes.data, n.value, C.byref(n)))
    r = out[:n.value]
    return dict(obj=r[:, 0].astype(np.int64), prim=r[:, 1].astype(np.int64), kind=r[:, 2].astype(np.int64),
                area=r[:, 3].astype(np.float64), weight=r[:, 4].astype(np.float64))


def selftest_emitter_sample(device_scene, x, n, seed=1):
    """fw_selftest_emitter_sample: n picks of a DeviceScene's FW_FLAG_ALL_EMITTERS table from world point x, as k_shade_pl draws them.
    -> dict: entry (int64), p_pick (the stored table's), p_omega, world (n, 3) and obj_point (n, 3) (the point in the object's frame)"""
    lib = load()
    xv = np.ascontiguousarray(x, np.float32)
    out = np.zeros((int(n), A.FW_EMITTER_SAMPLE_FLOATS), np.float32)
    _check(lib, lib.fw_selftest_emitter_sample(device_scene.handle, xv.ctypes.data, int(n), int(seed) & 0xFFFFFFFF, out.ctypes.data))
    return dict(entry=out[:, 0].copy().view(np.uint32).astype(np.int64), p_pick=out[:, 1].astype(np.float64),
                p_omega=out[:, 2].astype(np.float64), world=out[:, 3:6].astype(np.float64), obj_point=out[:, 6:9].astype(np.float64))


def selftest_ggx(entries, device=0):
    """fw_selftest_ggx: (n, 15) float32 entries (normal xyz, ray direction xyz, roughness, F0 rgb, xi1, xi2, omega xyz) through the device
    functions a GgxMat vertex is shaded with.  -> dict of float32 arrays: wi (n, 3), atten (n, 3), alive (n,) bool,
    fcos (n, 3), pb (n,)"""
    lib = load()
    e = np.ascontiguousarray(entries, np.float32)
    assert e.ndim == 2 and e.shape[1] == A.FW_GGX_IN_FLOATS, e.shape
    out = np.zeros((e.shape[0], A.FW_GGX_OUT_FLOATS), np.float32)
    _check(lib, lib.fw_selftest_ggx(int(device), e.shape[0], e.ctypes.data, out.ctypes.data))
    return dict(wi=out[:, 0:3].copy(), atten=out[:, 3:6].copy(), alive=out[:, 6] != 0, fcos=out[:, 7:10].copy(), pb=out[:, 10].copy())


def selftest_env_dist(rgb, device=0):
    """fw_selftest_env_dist: the FW_FLAG_ENV_SAMPLING table of an (h, w, 3) float map as the device builds it.
    -> ((h, w) float32 per-texel probabilities, total weight)"""
    lib = load()
    m = np.ascontiguousarray(rgb, np.float32)
    h, w = m.shape[:2]
    p = np.zeros((h, w), np.float32)
    total = C.c_double()
    _check(lib, lib.fw_selftest_env_dist(int(device), m.ctypes.data, w, h, p.ctypes.data, C.byref(total)))
    return p, float(total.value)


def selftest_env_sample(rgb, n, seed=1, device=0):
    """fw_selftest_env_sample: n directions drawn from the table of an (h, w, 3) float map as k_shade_env draws them.  -> (dirs (n, 3),
    reported pdf (n,), drawn texel (n,), looked-up texel (n,))"""
    lib = load()
    m = np.ascontiguousarray(rgb, np.float32)
    h, w = m.shape[:2]
    out = np.zeros((int(n), A.FW_ENV_SAMPLE_FLOATS), np.float32)
    _check(lib, lib.fw_selftest_env_sample(int(device), m.ctypes.data, w, h, int(n), int(seed) & 0xFFFFFFFF, out.ctypes.data))
    return out[:, 0:3].copy(), out[:, 3].copy(), out[:, 4].astype(np.int64), out[:, 5].astype(np.int64)


def selftest_bvh_build(boxes, threads):
    """fw_selftest_bvh_build (CPU only): the host tree builders with `threads` threads.  -> (hash of the median tree, hash of the SAH tree, stats)"""
    lib = load()
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    h = (C.c_uint64 * 2)()
    st = (C.c_uint32 * 4)()
    _check(lib, lib.fw_selftest_bvh_build(b.ctypes.data, b.shape[0], int(threads), h, st))
    return int(h[0]), int(h[1]), dict(median_nodes=int(st[0]), median_depth=int(st[1]), sah_nodes=int(st[2]), sah_depth=int(st[3]))


def selftest_bvh_trees(boxes, device):
    """fw_selftest_bvh_trees: both trees over n boxes (n x 6 float32), built on GPU `device` or, for device = -1, by the host builders.
    -> (median-split nodes, SAH nodes, stats): node arrays of shape (nodes, 8) float32, stats = [median nodes, depth, SAH nodes, depth]"""
    lib = load()
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    n = b.shape[0]
    cap = max(1, 2 * n - 1) * 8
    ref = np.zeros(cap, np.float32)
    sah = np.zeros(cap, np.float32)
    st = (C.c_uint32 * 4)()
    _check(lib, lib.fw_selftest_bvh_trees(int(device), b.ctypes.data, n, ref.ctypes.data, sah.ctypes.data, st))
    stats = np.array(list(st), np.uint32)
    return ref[: int(stats[0]) * 8].reshape(-1, 8), sah[: int(stats[2]) * 8].reshape(-1, 8), stats


def selftest_arith(n, seed=1, mode=0, device=0):
    lib = load()
    d, s = C.c_uint64(), C.c_uint64()
    _check(lib, lib.fw_selftest_arith(device, n, seed, mode, C.byref(d), C.byref(s)))
    return int(d.value), int(s.value)


LIBM_FN = dict(logf=0, log10f=1, sinf=2, asinf=3, acosf=4, atanf=5, atan2f=6, powf=7)


def selftest_libm(fn, x, y=None, device=0):
    """fw_selftest_libm: the device's restated glibc function `fn` over float32 arrays."""
    lib = load()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    yy = None if y is None else np.ascontiguousarray(y, np.float32)
    _check(lib, lib.fw_selftest_libm(device, LIBM_FN[fn], x.size, x.ctypes.data, None if yy is None else yy.ctypes.data, out.ctypes.data))
    return out


def build_id():
    """sha256 of the loaded library file: identifies the kernels a checkpoint's sums were made with."""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def release_workspace(device=0):
    load().fw_release_workspace(device)


def device_count():
    return load().fw_device_count()


# numpy mirror of fw_hit (include/firework_hip.h): what DeviceScene.trace returns for host rays
HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, (3,)), ("normal", np.float32, (3,)), ("u", np.float32),
                      ("v", np.float32), ("material", np.uint32), ("object", np.uint32), ("prim", np.uint32)], align=True)
# column of each field in the (n, 12) float32 records DeviceScene.trace returns for device tensors; material / object / prim are
# integers: read them through an int32 view, hit_fields(records)
HIT_COLUMNS = dict(t=0, point=slice(1, 4), normal=slice(4, 7), u=7, v=8, material=9, object=10, prim=11)


def hit_fields(records):
    """The fields of (n, 12) float32 trace records (a torch tensor) as views: t, point (n, 3), normal (n, 3), u, v float32; material,
    object, prim int32 (object == -1, i.e. FW_NO_HIT, on a miss)."""
    ints = records.view(dtype=__import__("torch").int32)
    out = {k: records[:, c] for k, c in HIT_COLUMNS.items() if k not in ("material", "object", "prim")}
    out.update(material=ints[:, 9], object=ints[:, 10], prim=ints[:, 11])
    return out


def camera_rays(renderer, sample=0, pixel_ids=None, device=0):
    """fw_camera_rays: the segment-0 rays a render of `renderer` traces for `sample` of each pixel (pixel_ids, or every pixel in index
    order), as an (n, 6) float32 array of origin and direction."""
    lib = load()
    ids = None if pixel_ids is None else np.ascontiguousarray(np.asarray(pixel_ids, dtype=np.uint32))
    p = renderer.to_params(ids)
    n = int(ids.shape[0]) if ids is not None else p.width * p.height
    out = np.empty((n, 6), np.float32)
    _check(lib, lib.fw_camera_rays(C.byref(p), int(device), int(sample), out.ctypes.data))
    return out


def _stream_arg(stream, torch_device):
    """the hipStream_t argument of a call on device tensors: `stream` (a raw handle), or for None the current torch stream of torch_device"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(torch_device).cuda_stream
    return C.c_void_p(stream) if stream else None


def _host_f32(arr, shape, name):
    """the check of a caller-owned host array that a call updates in place"""
    if not (isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == tuple(shape) and arr.flags["C_CONTIGUOUS"]):
        raise ValueError(f"{name} must be a contiguous float32 array of shape {tuple(shape)}")


def _check_device_tensor(t, shape, dtype, device, name):
    if (tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device.type != "cuda"
            or (t.device.index or 0) != device):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on cuda:{device}")


_HOST_DTYPES = dict(f32=np.float32, u8=np.uint8, ids=np.uint32)
_DEVICE_DTYPES = dict(f32="float32", u8="uint8", ids="int32")      # (torch's, by name: torch is imported on the device side only)


class _Side:
    """Where the arrays of one call lie — host (numpy) arrays, or torch tensors on cuda:`device` — and how each of them reaches the C ABI.
    The only place that tells the two apart: `first`, the call's first array, decides (or on_device=True does), and torch is imported for
    the device side only.  Every method returns the array as the call uses it and ptr() its pointer.  The object holds whatever a pointer
    points into, so a wrapper that keeps its _Side in a local until the C function has returned needs no keepalive of its own."""

    def __init__(self, first, device, on_device=False):
        self.device = int(device)
        self.on_device = bool(on_device) or type(first).__module__.startswith("torch")
        self._keep = []
        if self.on_device:
            import torch
            self._torch, self.dev = torch, torch.device("cuda", self.device)

    def _dtype(self, kind):
        """kind: "f32", "u8", or "ids": uint32 on the host, their int32 bits on the device"""
        return getattr(self._torch, _DEVICE_DTYPES[kind]) if self.on_device else _HOST_DTYPES[kind]

    def ptr(self, a):
        return None if a is None else a.data_ptr() if self.on_device else a.ctypes.data

    def ptrs(self, *arrays):
        return tuple(self.ptr(a) for a in arrays)

    def count(self, a, cols):
        """N of an (N, cols) input: a device tensor's rows; a host array may have any shape of N * cols elements"""
        return int(a.shape[0]) if self.on_device else int(np.size(a)) // cols

    def inp(self, a, shape, name, kind="f32", below=None):
        """an input array of `shape` (None stays None).  Host: converted only if it is not a contiguous array of the dtype already.
        Device: checked, never copied.  below: every element must be in 0..below-1."""
        if a is None:
            return None
        if self.on_device:
            _check_device_tensor(a, shape, self._dtype(kind), self.device, name)
        else:
            a = np.asarray(a, self._dtype(kind))
            if a.size != math.prod(shape):
                raise ValueError(f"{name} must have shape {tuple(shape)}")
            a = np.ascontiguousarray(a.reshape(shape))
        if below is not None and a.shape[0] and not (0 <= int(a.min()) and int(a.max()) < below):
            raise ValueError(f"every id must be in 0..{below - 1}")
        self._keep.append(a)
        return a

    def hits(self, hits, total):
        """DeviceScene.trace's records of `total` rays: a HIT_DTYPE array on the host, an (total, 12) float32 tensor on the device"""
        if self.on_device:
            return self.inp(hits, (total, 12), "hits")
        h = np.ascontiguousarray(hits)
        if h.dtype != HIT_DTYPE or h.shape != (total,):
            raise ValueError("host hits must be an array of HIT_DTYPE, one record per ray")
        self._keep.append(h)
        return h

    def columns(self, n, *named):
        """(arrays, row stride in floats) of (n, 3) float32 inputs given as (array, name) pairs and read in place: each contiguous, or all
        of them column ranges of one contiguous (n, S) array — fw_render_aovs' records (aov[:, 8:11], aov[:, 4:7]), a ray buffer's
        rays[:, 3:6] — with unit column stride and one common row stride >= 3.  Host arrays laid out otherwise are copied."""
        arrays = [a for a, _ in named]
        if self.on_device:
            s0 = int(arrays[0].stride(0)) if arrays[0].dim() == 2 else 0
            stride = s0 if n > 1 else max(3, s0)
            for t, name in named:
                if (t.dtype != self._torch.float32 or tuple(t.shape) != (n, 3) or t.stride(1) != 1 or t.device.type != "cuda"
                        or (t.device.index or 0) != self.device or (n > 1 and int(t.stride(0)) != stride) or stride < 3):
                    raise ValueError(f"{name} must be an ({n}, 3) float32 tensor on cuda:{self.device} with unit column stride and a row stride >= 3, "
                                     "the same as the arrays it comes with")
        else:
            arrays = [np.asarray(a, np.float32) for a in arrays]
            for a, (_, name) in zip(arrays, named):
                if a.size != n * 3:
                    raise ValueError(f"{name} must have shape ({n}, 3)")
            arrays = [a.reshape(n, 3) for a in arrays]
            st = arrays[0].strides
            if not (st[1] == 4 and st[0] % 4 == 0 and st[0] >= 12 and all(a.strides == st for a in arrays)):
                arrays = [np.ascontiguousarray(a) for a in arrays]
            stride = arrays[0].strides[0] // 4
        self._keep += arrays
        return arrays, stride

    def new(self, shape, kind="f32", fill=None):
        """a new output on the call's side: uninitialised, or filled with `fill`"""
        if self.on_device:
            if fill is None:
                return self._torch.empty(shape, dtype=self._dtype(kind), device=self.dev)
            return self._torch.full(shape, fill, dtype=self._dtype(kind), device=self.dev)
        return np.empty(shape, self._dtype(kind)) if fill is None else np.full(shape, fill, self._dtype(kind))

    def new_hits(self, n):
        """new records of n rays for fw_trace_rays to fill, of the kind hits() takes"""
        return self.new((n, 12)) if self.on_device else np.zeros(n, HIT_DTYPE)

    def out(self, a, shape, name, fill=None):
        """a float32 array that the call writes or updates in place: the caller's own `a`, checked and never copied, or for None a new one"""
        if a is None:
            return self.new(shape, fill=fill)
        if self.on_device:
            _check_device_tensor(a, shape, self._torch.float32, self.device, name)
        else:
            _host_f32(a, shape, name)
        return a

    def tail(self, stream):
        """the (on_device, stream) arguments that end a call; stream None: the current torch stream"""
        return (1, _stream_arg(stream, self.dev)) if self.on_device else (0, None)

    def params(self, p, stream=None):
        """the same two, for a call that carries them in its params struct"""
        if self.on_device:
            p.on_device, p.stream = 1, _stream_arg(stream, self.dev)


def _model_abi(model, chunk=None):
    """a fw_camera_model from an api.CameraModel (or a fw_camera_model, copied), with chunk_samples = chunk when given"""
    m = model.to_abi() if hasattr(model, "to_abi") else A.fw_camera_model.from_buffer_copy(model)
    if chunk is not None:
        m.chunk_samples = int(chunk)
    return m


def model_rays(model, first_sample=0, n_samples=1, device=0, out=None, stream=None):
    """fw_model_rays: the rays of the absolute samples [first_sample, first_sample + n_samples) of a camera model (an api.CameraModel or
    a fw_camera_model), generated on the device: (n_samples, W * H, 6) float32 origin + direction, row 0 = the image top.  Returns a
    numpy array; out: a contiguous float32 device tensor of that shape on cuda:`device` to fill instead, on `stream` (default: the
    current torch stream); returned."""
    lib = load()
    m = _model_abi(model)
    s = _Side(out, device)
    out = s.out(out, (int(n_samples), int(m.width) * int(m.height), 6), "out")
    _check(lib, lib.fw_model_rays(C.byref(m), int(device), int(first_sample), int(n_samples), s.ptr(out), *s.tail(stream)))
    return out


def _probe_abi(probes, chunk=None):
    """(fw_probe_set, the positions array it points into) from an api.ProbeSet, with chunk_probes = chunk when given"""
    s, pos = probes.to_abi()
    if chunk is not None:
        s.chunk_probes = int(chunk)
    return s, pos


def probe_rays(probes, round=0, first_probe=0, n=None, device=0, out=None, stream=None):
    """fw_probe_rays: the rays of round `round` of the probes [first_probe, first_probe + n) of an api.ProbeSet (n None: to the last
    one), generated on the device: (n * D, 6) float32 origin + direction, entry p * D + j = direction j of probe p.  Returns a numpy
    array; out: a contiguous float32 device tensor of that shape on cuda:`device` to fill instead, on `stream` (default: the current
    torch stream); returned."""
    lib = load()
    ps, _pos = _probe_abi(probes)
    if n is None:
        n = int(ps.n_probes) - int(first_probe)
    s = _Side(out, device)
    out = s.out(out, (int(n) * int(ps.directions), 6), "out")
    _check(lib, lib.fw_probe_rays(C.byref(ps), int(device), int(round), int(first_probe), int(n), s.ptr(out), *s.tail(stream)))
    return out


def _per_probe(rays, other, other_cols, directions):
    """(N, N * D) of one round's rays (N * D, 6) and the (N * D, ...) array that comes with them: accum (other_cols 4) or hits (None)"""
    d = int(directions)
    total = int(rays.shape[0])
    ok = d >= 1 and total % d == 0 and tuple(rays.shape) == (total, 6)
    if other_cols is None:
        if not ok or int(other.shape[0]) != total:
            raise ValueError(f"rays must have shape (N * {d}, 6) and hits N * {d} records")
    elif not ok or tuple(other.shape) != (total, other_cols):
        raise ValueError(f"rays must have shape (N * {d}, 6) and accum (N * {d}, {other_cols})")
    return total // d, total


def probe_project(rays, accum, samples, directions, sums=None, device=0, stream=None):
    """fw_probe_project: adds (4 pi / D) sum_j Y_k(d_pj) accum[p D + j] / samples, rounded to float32 once, to sums[p][k].  rays (N * D,
    6) and accum (N * D, 4) float32, sums (N, 9, 3) float32 updated in place (None: zeros); numpy arrays, or contiguous torch tensors
    on cuda:`device`, projected on `stream` (default: the current torch stream) where they lie.  Returns sums."""
    lib = load()
    n, total = _per_probe(rays, accum, 4, directions)
    s = _Side(rays, device)
    r, a = s.inp(rays, (total, 6), "rays"), s.inp(accum, (total, 4), "accum")
    sums = s.out(sums, (n, 9, 3), "sums", fill=0.0)
    _check(lib, lib.fw_probe_project(int(device), n, int(directions), int(samples), *s.ptrs(r, a, sums), *s.tail(stream)))
    return sums


def _grid_abi(grid):
    """(fw_probe_grid, its probe count) from an api.ProbeGrid, or an api.ProbeSet made by ProbeSet.grid (wrap on)"""
    from .api import ProbeGrid
    g = ProbeGrid.of(grid)
    return g.to_abi(), g.n_probes


def _vis_of(depth, moments, normal_bias):
    """the visibility of a lookup as (depth, moments, normal_bias), or None without one"""
    if (depth is None) != (moments is None):
        raise ValueError("depth and moments are given together or not at all")
    return None if depth is None else (depth, moments, normal_bias)


def _vis_args(s, vis, n_probes):
    """[fw_probe_depth, moments pointer, normal_bias] of a lookup; vis (see _vis_of) None: no visibility, [NULL, NULL, 0].  moments
    (n, R, R, 2) float32, on the side of the call's other arrays"""
    if vis is None:
        return [None, None, 0.0]
    depth, moments, normal_bias = vis
    pd = depth.to_abi()
    R = int(pd.resolution)
    return [C.byref(pd), s.ptr(s.inp(moments, (n_probes, R, R, 2), "moments")), float(normal_bias)]


def _placement_arg(s, placement, n_probes):
    """the placement pointer of a lookup: (n, 4) float32 records (ox, oy, oz, a), on the side of the call's other arrays; None: NULL"""
    return s.ptr(s.inp(placement, (n_probes, 4), "placement"))


def _sh_lookup(s, lib, stem, g, sh, n_probes, vis, placement):
    """(the entry point, its leading arguments) of fw_probe_irradiance or fw_probe_shade (`stem`): the plain form, _vis with a visibility
    only, _placed with a placement (and there a visibility or NULLs)"""
    head = [C.byref(g), s.ptr(s.inp(sh, (n_probes, 9, 3), "sh"))]
    if placement is not None:
        return getattr(lib, stem + "_placed"), head + _vis_args(s, vis, n_probes) + [_placement_arg(s, placement, n_probes)]
    if vis is not None:
        return getattr(lib, stem + "_vis"), head + _vis_args(s, vis, n_probes)
    return getattr(lib, stem), head


def probe_irradiance(grid, sh, positions, normals, out=None, stream=None, device=0, _vis=None, _placed=None):
    """fw_probe_irradiance: the irradiance the probe grid `grid` (an api.ProbeGrid, or an api.ProbeSet made by ProbeSet.grid) with the
    coefficients sh (n, 9, 3) float32 gives at the points `positions` with the normals `normals`, (N, 3) float32 each; not clamped.
    numpy arrays: returns an (N, 3) float32 array (out: a contiguous float32 array of that shape to fill instead).  Torch tensors on
    cuda:`device`: looked up on `stream` (default: the current torch stream) where they lie; returns a device tensor (out: a contiguous
    (N, 3) float32 tensor to fill instead).  positions and normals: contiguous (N, 3), or two column ranges of one contiguous (N, S)
    array such as fw_render_aovs' records (aov[:, 8:11], aov[:, 4:7]), read in place."""
    lib = load()
    g, n_probes = _grid_abi(grid)
    s = _Side(positions, device)
    n = s.count(positions, 3)
    fn, head = _sh_lookup(s, lib, "fw_probe_irradiance", g, sh, n_probes, _vis, _placed)
    (p, nr), stride = s.columns(n, (positions, "positions"), (normals, "normals"))
    out = s.out(out, (n, 3), "out")
    _check(lib, fn(*head, int(device), n, *s.ptrs(p, nr), stride, s.ptr(out), *s.tail(stream)))
    return out


def probe_irradiance_vis(grid, sh, depth, moments, positions, normals, normal_bias=0.0, out=None, stream=None, device=0):
    """fw_probe_irradiance_vis: probe_irradiance with every corner probe weighted by its visibility from the point: depth an
    api.ProbeDepth, moments (n, R, R, 2) float32 as DeviceScene.bake_probe_depth returns them (a device tensor when the points are),
    normal_bias >= 0 in world units.  Everything else as probe_irradiance."""
    return probe_irradiance(grid, sh, positions, normals, out, stream, device, _vis=(depth, moments, normal_bias))


def probe_irradiance_placed(grid, sh, placement, positions, normals, depth=None, moments=None, normal_bias=0.0, out=None, stream=None, device=0):
    """fw_probe_irradiance_placed: probe_irradiance — or with depth (an api.ProbeDepth) and moments probe_irradiance_vis — over moved and
    classified probes: placement (n, 4) float32 records (ox, oy, oz, a) as DeviceScene.relocate_probes returns them (a device tensor when
    the points are).  An inactive probe (a == 0) is skipped and the remaining weights are always normalised.  Everything else as
    probe_irradiance."""
    return probe_irradiance(grid, sh, positions, normals, out, stream, device, _vis=_vis_of(depth, moments, normal_bias), _placed=placement)


def probe_survey(rays, hits, directions, out=None, device=0, stream=None):
    """fw_probe_survey: the survey (N, 3, 4) float32 of one round — per probe (back.xyz, dist), (front.xyz, dist) and (n_back, n_front,
    n_miss, 0) — from rays (N * D, 6) float32 and hits as DeviceScene.trace returns them for those rays: a HIT_DTYPE array for numpy rays,
    or an (N * D, 12) float32 device tensor for rays on cuda:`device`, surveyed on `stream` (default: the current torch stream) where they
    lie.  out: an array or tensor of that shape to overwrite instead.  Returns the survey."""
    lib = load()
    n, total = _per_probe(rays, hits, None, directions)
    s = _Side(rays, device)
    r, h = s.inp(rays, (total, 6), "rays"), s.hits(hits, total)
    out = s.out(out, (n, 3, 4), "out")
    _check(lib, lib.fw_probe_survey(int(device), n, int(directions), *s.ptrs(r, h, out), *s.tail(stream)))
    return out


def probe_relocate_step(relocation, survey, placement, directions, move=True, device=0, stream=None):
    """fw_probe_relocate_step: one step of an api.ProbeRelocation (with a max_offset of its own) over survey (N, 3, 4) and placement (N, 4)
    float32, which is updated in place and returned: numpy arrays, or contiguous torch tensors on cuda:`device`, stepped on `stream`
    (default: the current torch stream) where they lie.  move=False writes the state a only."""
    lib = load()
    rl = relocation.to_abi()
    n = int(placement.shape[0])
    s = _Side(placement, device)
    sv = s.inp(survey, (n, 3, 4), "survey")
    s.out(placement, (n, 4), "placement")
    _check(lib, lib.fw_probe_relocate_step(int(device), C.byref(rl), n, int(directions), *s.ptrs(sv, placement), int(bool(move)), *s.tail(stream)))
    return placement


def probe_depth_reduce(depth, rays, hits, directions, sums=None, device=0, stream=None):
    """fw_probe_depth_reduce: adds one round's depth sums (A, B, W per texel, each rounded to float32 once) to sums (N, R, R, 4) float32,
    updated in place (None: zeros); .w is left alone.  rays (N * D, 6) float32 and hits as DeviceScene.trace returns them for those rays:
    a HIT_DTYPE array for numpy rays, or an (N * D, 12) float32 device tensor for rays on cuda:`device`, reduced on `stream` (default: the
    current torch stream) where they lie.  Returns sums."""
    lib = load()
    pd = depth.to_abi()
    R = int(pd.resolution)
    n, total = _per_probe(rays, hits, None, directions)
    s = _Side(rays, device)
    r, h = s.inp(rays, (total, 6), "rays"), s.hits(hits, total)
    sums = s.out(sums, (n, R, R, 4), "sums", fill=0.0)
    _check(lib, lib.fw_probe_depth_reduce(int(device), C.byref(pd), n, int(directions), *s.ptrs(r, h, sums), *s.tail(stream)))
    return sums


def probe_radiance_reduce(radiance, rays, accum, samples, directions, sums=None, device=0, stream=None):
    """fw_probe_radiance_reduce: adds one round's radiance sums (A_r, A_g, A_b, W per texel, each rounded to float32 once) to sums (N, R,
    R, 4) float32, updated in place (None: zeros).  radiance an api.ProbeRadiance; rays (N * D, 6) and accum (N * D, 4) float32 as
    DeviceScene.render_rays leaves it: numpy arrays, or contiguous torch tensors on cuda:`device`, reduced on `stream` (default: the
    current torch stream) where they lie.  Returns sums."""
    lib = load()
    pr = radiance.to_abi()
    R = int(pr.resolution)
    n, total = _per_probe(rays, accum, 4, directions)
    s = _Side(rays, device)
    r, a = s.inp(rays, (total, 6), "rays"), s.inp(accum, (total, 4), "accum")
    sums = s.out(sums, (n, R, R, 4), "sums", fill=0.0)
    _check(lib, lib.fw_probe_radiance_reduce(int(device), C.byref(pr), n, int(directions), int(samples), *s.ptrs(r, a, sums), *s.tail(stream)))
    return sums


def probe_radiance_prefilter(radiance, sums, out=None, device=0, stream=None):
    """fw_probe_radiance_prefilter: the maps (N, M, 4) float32 — (r, g, b, flag) per texel of every level, M = radiance.texels — of the
    sums (N, R, R, 4) float32: level 0 divided, the levels above it GGX-prefiltered from level 0.  numpy arrays, or contiguous torch
    tensors on cuda:`device`, filtered on `stream` (default: the current torch stream) where they lie.  out: an array or tensor of that
    shape to overwrite instead.  Returns the maps."""
    lib = load()
    pr = radiance.to_abi()
    R, M = int(pr.resolution), int(radiance.texels)
    n = int(sums.shape[0])
    s = _Side(sums, device)
    sm = s.inp(sums, (n, R, R, 4), "sums")
    out = s.out(out, (n, M, 4), "out")
    _check(lib, lib.fw_probe_radiance_prefilter(int(device), C.byref(pr), n, *s.ptrs(sm, out), *s.tail(stream)))
    return out


def _radiance_args(s, radiance, maps, vis, placement, n_probes):
    """the [pr, maps, pd, moments, normal_bias, placement] arguments of fw_probe_radiance_lookup and the glossy shades: maps (n, M, 4)
    float32; vis (see _vis_of) and placement optional; on the side of the call's other arrays"""
    pr = radiance.to_abi()
    mp = s.inp(maps, (n_probes, int(radiance.texels), 4), "maps")
    return [C.byref(pr), s.ptr(mp)] + _vis_args(s, vis, n_probes) + [_placement_arg(s, placement, n_probes)]


def probe_radiance_lookup(grid, radiance, maps, positions, normals, dirs, roughness, depth=None, moments=None, normal_bias=0.0, placement=None,
                          out=None, stream=None, device=0):
    """fw_probe_radiance_lookup: the radiance the probes of `grid` (see probe_irradiance) hold along `dirs` at the roughness `roughness`,
    seen from the points `positions` with the normals `normals`: maps (n, M, 4) float32 as DeviceScene.bake_probe_radiance returns them
    for radiance (an api.ProbeRadiance), positions, normals and dirs (N, 3) and roughness (N,) float32; not clamped.  depth with moments,
    normal_bias and placement weight the corners as probe_irradiance_placed does (placement None: every probe active where it stands).
    numpy arrays: returns an (N, 3) float32 array.  Contiguous torch tensors on cuda:`device`: looked up on `stream` (default: the current
    torch stream) where they lie; returns a device tensor.  out: an array or tensor of that shape to fill instead."""
    lib = load()
    g, n_probes = _grid_abi(grid)
    s = _Side(positions, device)
    n = s.count(positions, 3)
    p, nr, dr = (s.inp(a, (n, 3), name) for a, name in ((positions, "positions"), (normals, "normals"), (dirs, "dirs")))
    ro = s.inp(roughness, (n,), "roughness")
    head = _radiance_args(s, radiance, maps, _vis_of(depth, moments, normal_bias), placement, n_probes)
    out = s.out(out, (n, 3), "out")
    _check(lib, lib.fw_probe_radiance_lookup(C.byref(g), *head, int(device), n, *s.ptrs(p, nr), 3, *s.ptrs(dr, ro, out), *s.tail(stream)))
    return out


def _table_arg(s, table):
    """(pointer, n_mu, n_rho) of an (n_rho, n_mu, 2) float32 table, on the side of the call's other arrays"""
    shape = tuple(table.shape) if s.on_device else np.shape(table)
    if len(shape) != 3 or shape[2] != 2:
        raise ValueError("table must have the shape (n_rho, n_mu, 2)")
    return s.ptr(s.inp(table, shape, "table")), int(shape[1]), int(shape[0])


def _probe_shade(grid, sh, aov, width, height, gamma, device, stream, outputs, vis=None, placement=None, glossy=None, split=None):
    """The one body of probe_shade and its _vis, _placed, _glossy and _split forms.  vis: see _vis_of; glossy: (radiance, maps, spec, view)
    or None for the diffuse forms; split: (table, flags) or None, with glossy only."""
    lib = load()
    g, n_probes = _grid_abi(grid)
    n = int(width) * int(height)
    s = _Side(aov, device)
    p = A.fw_probe_shade_params()
    p.width, p.height, p.gamma, p.device = int(width), int(height), float(gamma), int(device)
    if glossy is None:
        fn, head = _sh_lookup(s, lib, "fw_probe_shade", g, sh, n_probes, vis, placement)
        mid = (C.byref(p), s.ptr(s.inp(aov, (n, 12), "aov")))
    else:
        radiance, maps, spec, view = glossy
        fn, head = lib.fw_probe_shade_glossy, [C.byref(g), s.ptr(s.inp(sh, (n_probes, 9, 3), "sh"))]
        a, sp = s.inp(aov, (n, 12), "aov"), s.inp(spec, (n, 4), "spec")
        (vw,), stride = s.columns(n, (view, "view"))
        head += _radiance_args(s, radiance, maps, vis, placement, n_probes)
        mid = (C.byref(p), *s.ptrs(a, sp, vw), stride)
        if split is not None:
            fn, mid = lib.fw_probe_shade_split, mid + _table_arg(s, split[0]) + (int(split[1]),)
    rgb8, gam, lin = (s.new((n, 3), kind) if name in outputs else None for name, kind in (("rgb8", "u8"), ("gamma", "f32"), ("linear", "f32")))
    s.params(p, stream)
    _check(lib, fn(*head, *mid, *s.ptrs(lin, gam, rgb8)))
    return rgb8, gam, lin


def probe_shade(grid, sh, aov, width, height, gamma=2.2, device=0, stream=None, outputs=("rgb8", "gamma", "linear"), _vis=None, _placed=None):
    """fw_probe_shade: fw_render_aovs' records `aov` (N, 12) lit from the probe grid `grid` (see probe_irradiance) with the coefficients
    sh (n, 9, 3): out = albedo (coverage max(E, 0) / pi + (1 - coverage)), resolved as fw_denoise resolves its outputs.  All host arrays
    (numpy): returns (rgb8, gamma, linear) host arrays of shape (N, 3).  Contiguous float32 torch tensors on cuda:`device`: shaded on
    `stream` (default: the current torch stream), returns device tensors.  outputs: which of the three to compute; the others are
    returned as None.  width * height must be N."""
    return _probe_shade(grid, sh, aov, width, height, gamma, device, stream, outputs, _vis, _placed)


def probe_shade_vis(grid, sh, depth, moments, aov, width, height, normal_bias=0.0, gamma=2.2, device=0, stream=None,
                    outputs=("rgb8", "gamma", "linear")):
    """fw_probe_shade_vis: probe_shade with the lookup of probe_irradiance_vis (depth, moments, normal_bias: see there)."""
    return _probe_shade(grid, sh, aov, width, height, gamma, device, stream, outputs, (depth, moments, normal_bias))


def probe_shade_placed(grid, sh, placement, aov, width, height, depth=None, moments=None, normal_bias=0.0, gamma=2.2, device=0, stream=None,
                       outputs=("rgb8", "gamma", "linear")):
    """fw_probe_shade_placed: probe_shade with the lookup of probe_irradiance_placed (placement, depth, moments, normal_bias: see there)."""
    return _probe_shade(grid, sh, aov, width, height, gamma, device, stream, outputs, _vis_of(depth, moments, normal_bias), placement)


def probe_shade_glossy(grid, sh, radiance, maps, aov, spec, view, width, height, depth=None, moments=None, normal_bias=0.0, placement=None,
                       gamma=2.2, device=0, stream=None, outputs=("rgb8", "gamma", "linear")):
    """fw_probe_shade_glossy: probe_shade_placed where spec's roughness is not > 0, and elsewhere a conductor lit by the radiance maps
    along the mirrored view direction: spec (N, 4) float32 (F0.rgb, rho), view (N, 3) float32 — contiguous, or three columns of a
    contiguous (N, S) array such as rays[:, 3:6], read in place — the ray direction from the eye.  radiance, maps, depth, moments,
    normal_bias and placement as probe_radiance_lookup; everything else as probe_shade."""
    return _probe_shade(grid, sh, aov, width, height, gamma, device, stream, outputs, _vis_of(depth, moments, normal_bias), placement,
                        glossy=(radiance, maps, spec, view))


def probe_shade_split(grid, sh, radiance, maps, aov, spec, view, table, width, height, flags=0, depth=None, moments=None, normal_bias=0.0,
                      placement=None, gamma=2.2, device=0, stream=None, outputs=("rgb8", "gamma", "linear")):
    """fw_probe_shade_split: probe_shade_glossy with the split sum's BRDF term: a glossy pixel is v ((F0 A + B) Ls) + (1 - v) a with (A, B)
    looked up in `table` ((n_rho, n_mu, 2) float32, as ggx_table returns it; a device tensor when the other arrays are) at the cosine of
    the view and the pixel's roughness; flags: FW_SPLIT_ENERGY multiplies by 1 + F0 (1 / (A + B) - 1).  Everything else as
    probe_shade_glossy."""
    return _probe_shade(grid, sh, aov, width, height, gamma, device, stream, outputs, _vis_of(depth, moments, normal_bias), placement,
                        glossy=(radiance, maps, spec, view), split=(table, flags))


def _lightmap_abi(lightmap, chunk=None):
    """(fw_lightmap, the arrays it points into) from an api.Lightmap, with chunk_texels = chunk when given"""
    s, keep = lightmap.to_abi()
    if chunk is not None:
        s.chunk_texels = int(chunk)
    return s, keep


def lightmap_texels(lightmap, device=0, on_device=False, stream=None):
    """fw_lightmap_texels: (records (W * H, 8) float32, owner (W * H,) uint32 — int32 bits on the device — and the number of covered
    texels) of an api.Lightmap, rasterised on the device.  numpy arrays, or with on_device=True torch tensors on cuda:`device`, written on
    `stream` (default: the current torch stream)."""
    lib = load()
    lm, _keep = _lightmap_abi(lightmap)
    n = int(lm.width) * int(lm.height)
    count = C.c_uint32(0)
    s = _Side(None, device, on_device)
    rec, own = s.new((n, 8), fill=float("nan")), s.new((n,), "ids", fill=0)
    _check(lib, lib.fw_lightmap_texels(C.byref(lm), int(device), *s.ptrs(rec, own), C.byref(count), *s.tail(stream)))
    return rec, own, int(count.value)


def lightmap_covered(lightmap, device=0):
    """the number of covered texels of an api.Lightmap (fw_lightmap_texels with no arrays)"""
    lib = load()
    s, _keep = _lightmap_abi(lightmap)
    count = C.c_uint32(0)
    _check(lib, lib.fw_lightmap_texels(C.byref(s), int(device), None, None, C.byref(count), 0, None))
    return int(count.value)


def lightmap_rays(lightmap, round=0, first=0, n=None, device=0, out=None, stream=None):
    """fw_lightmap_rays: the rays of round `round` of the entries [first, first + n) of an api.Lightmap's covered list (n None: to the
    last one), generated on the device: (n * D, 6) float32 origin + direction, entry q * D + j = direction j of covered texel q.  Returns
    a numpy array; out: a contiguous float32 device tensor of that shape on cuda:`device` to fill instead, on `stream` (default: the
    current torch stream); returned."""
    lib = load()
    lm, _keep = _lightmap_abi(lightmap)
    if n is None:
        n = (int(out.shape[0]) // int(lm.directions)) if out is not None else lightmap_covered(lightmap, device) - int(first)
    s = _Side(out, device)
    out = s.out(out, (int(n) * int(lm.directions), 6), "out")
    _check(lib, lib.fw_lightmap_rays(C.byref(lm), int(device), int(round), int(first), int(n), s.ptr(out), *s.tail(stream)))
    return out


def lightmap_reduce(accum, samples, directions, sums, texel_ids=None, device=0, stream=None):
    """fw_lightmap_reduce: adds (pi / D) sum_j accum[q D + j] / samples, rounded to float32 once, to sums[texel_ids[q]] (texel_ids None:
    sums[q]).  accum (n * D, 4) float32; sums (n_texels, 4) or (H, W, 4) float32, updated in place (.w untouched); texel_ids n distinct
    ids (uint32 numpy / int32 torch).  numpy arrays, or contiguous torch tensors on cuda:`device`, reduced on `stream` (default: the
    current torch stream) where they lie.  Returns sums."""
    lib = load()
    d = int(directions)
    total = int(accum.shape[0])
    if d < 1 or total % d or tuple(accum.shape) != (total, 4):
        raise ValueError(f"accum must have shape (n * {d}, 4)")
    n = total // d
    if sums.shape[-1] != 4:
        raise ValueError("sums must have shape (n_texels, 4) or (H, W, 4)")
    n_texels = int(np.prod(sums.shape[:-1]))
    if texel_ids is not None and tuple(texel_ids.shape) != (n,):
        raise ValueError(f"texel_ids must have shape ({n},)")
    s = _Side(accum, device)
    a, ids = s.inp(accum, (total, 4), "accum"), s.inp(texel_ids, (n,), "texel_ids", "ids")
    s.out(sums, tuple(sums.shape), "sums")
    _check(lib, lib.fw_lightmap_reduce(int(device), n, d, int(samples), *s.ptrs(ids, a, sums), n_texels, *s.tail(stream)))
    return sums


def lightmap_dilate(image, passes, device=0, stream=None):
    """fw_lightmap_dilate: `passes` dilation passes of image (H, W, 4) float32 (rgb, a), in place: a contiguous numpy array, or a
    contiguous torch tensor on cuda:`device`, dilated on `stream` (default: the current torch stream).  Returns image."""
    lib = load()
    if len(image.shape) != 3 or image.shape[2] != 4:
        raise ValueError("image must have shape (H, W, 4)")
    h, w = int(image.shape[0]), int(image.shape[1])
    s = _Side(image, device)
    s.out(image, (h, w, 4), "image")
    _check(lib, lib.fw_lightmap_dilate(int(device), w, h, int(passes), s.ptr(image), *s.tail(stream)))
    return image


class _AoPoints:
    """The surface points of an AO call as the C ABI takes them, read in place.  positions and normals: (M, 3) float32 each, contiguous
    or two column ranges of one contiguous (M, S) array such as fw_render_aovs' records (aov[:, 8:11], aov[:, 4:7]) or
    fw_lightmap_texels' (rec[:, 0:3], rec[:, 4:7]); numpy arrays, or torch tensors on cuda:`device`.  ids: n distinct ids below M (uint32
    numpy / int32 torch) or None: every point in order.  Arrays indexed by id (sums, out) have M records.  side: the call's _Side."""

    def __init__(self, positions, normals, ids, device):
        s = self.side = _Side(positions, device)
        m = self.m = int(positions.shape[0])
        if m < 1 or tuple(positions.shape) != (m, 3) or tuple(normals.shape) != (m, 3):
            raise ValueError("positions and normals must have the same shape (M, 3), M >= 1")
        (p, nr), self.stride = s.columns(m, (positions, "positions"), (normals, "normals"))
        self.n = m if ids is None else len(ids)
        self.pos, self.nrm, self.ids = s.ptrs(p, nr, s.inp(ids, (self.n,), "ids", "ids", below=m))

    def records(self, arr, name, floats=4):
        """the pointer of an array indexed by id, checked: (M, floats) or (H, W, floats) float32 with H W = M, where the points lie"""
        shape = tuple(arr.shape)
        if shape[-1] != floats or int(np.prod(shape[:-1])) != self.m:
            raise ValueError(f"{name} must have shape ({self.m}, {floats}) or (H, W, {floats}) with H W = {self.m}")
        return self.side.ptr(self.side.out(arr, shape, name))


def ao_rays(ao, positions, normals, ids=None, round=0, device=0, out=None, stream=None):
    """fw_ao_rays: the rays of round `round` of an api.AmbientOcclusion around surface points (see _AoPoints), generated on the device:
    (n * D, 6) float32 origin + direction, entry q * D + j = direction j of point ids[q] (ids None: q).  numpy points: returns a numpy
    array.  Points on cuda:`device`: generated on `stream` (default: the current torch stream) where they lie; returns a device tensor.
    out: a contiguous float32 array or tensor of that shape to fill instead."""
    lib = load()
    a = ao.to_abi()
    pts = _AoPoints(positions, normals, ids, device)
    s = pts.side
    out = s.out(out, (pts.n * int(a.directions), 6), "out")
    _check(lib, lib.fw_ao_rays(C.byref(a), int(device), int(round), pts.n, pts.pos, pts.nrm, pts.stride, pts.ids, s.ptr(out), *s.tail(stream)))
    return out


def ao_reduce(ao, rays, hits, sums, ids=None, device=0, stream=None):
    """fw_ao_reduce: adds one round's reduction (Bx, By, Bz, O, each rounded to float32 once) of an api.AmbientOcclusion to
    sums[ids[q]] (ids None: sums[q]); sums (M, 4) or (H, W, 4) float32, updated in place.  rays (n * D, 6) float32 and hits as
    DeviceScene.trace returns them for those rays: a HIT_DTYPE array for numpy rays, or an (n * D, 12) float32 device tensor for rays on
    cuda:`device`, reduced on `stream` (default: the current torch stream) where they lie; ids n distinct ids (uint32 numpy / int32
    torch).  Returns sums."""
    lib = load()
    a = ao.to_abi()
    d = int(a.directions)
    total = int(rays.shape[0])
    if d < 1 or total % d or tuple(rays.shape) != (total, 6) or int(hits.shape[0]) != total:
        raise ValueError(f"rays must have shape (n * {d}, 6) and hits n * {d} records")
    n = total // d
    m = int(np.prod(tuple(sums.shape)[:-1]))
    if sums.shape[-1] != 4 or (ids is None and m < n) or (ids is not None and tuple(ids.shape) != (n,)):
        raise ValueError(f"sums must have shape (M, 4) or (H, W, 4) with M >= {n}, ids shape ({n},)")
    s = _Side(rays, device)
    r, h = s.inp(rays, (total, 6), "rays"), s.hits(hits, total)
    s.out(sums, tuple(sums.shape), "sums")
    i = s.inp(ids, (n,), "ids", "ids", below=m)
    _check(lib, lib.fw_ao_reduce(int(device), C.byref(a), n, *s.ptrs(i, r, h, sums), *s.tail(stream)))
    return sums


class _DirectPoints(_AoPoints):
    """_AoPoints with a direct-light call's optional per-id arrays, of the points' kind (numpy / torch on cuda:`device`).  view: (M, 3)
    float32, contiguous or a column range of a contiguous (M, S) array such as a ray buffer's rays[:, 3:6]; spec: (M, 4) float32
    contiguous (F0.rgb, rho), needs view.  Arrays indexed by id (sums, out) have M records of 8 floats."""

    def __init__(self, positions, normals, ids, view, spec, device):
        super().__init__(positions, normals, ids, device)
        if spec is not None and view is None:
            raise ValueError("spec needs view")
        self.view, self.view_stride = None, 3
        if view is not None:
            (v,), self.view_stride = self.side.columns(self.m, (view, "view"))
            self.view = self.side.ptr(v)
        self.spec = self.side.ptr(self.side.inp(spec, (self.m, 4), "spec"))


def direct_rays(direct, lights, positions, normals, ids=None, view=None, spec=None, device=0, out=None, stream=None):
    """fw_direct_rays: the shadow rays of an api.DirectLight from surface points (see _DirectPoints) towards `lights` (api lights or
    fw_light records), generated on the device: (n * Ln, 6) float32, entry q * Ln + i = point ids[q] (ids None: q) towards light i, or
    six zeros.  numpy points: returns a numpy array.  Points on cuda:`device`: generated on `stream` (default: the current torch stream)
    where they lie; returns a device tensor.  out: a contiguous float32 array or tensor of that shape to fill instead."""
    lib = load()
    d = direct.to_abi()
    arr, ln = _light_array(lights)
    pts = _DirectPoints(positions, normals, ids, view, spec, device)
    s = pts.side
    out = s.out(out, (pts.n * ln, 6), "out")
    _check(lib, lib.fw_direct_rays(C.byref(d), arr, ln, int(device), pts.n, pts.pos, pts.nrm, pts.stride, pts.ids, pts.view, pts.view_stride,
                                   pts.spec, s.ptr(out), *s.tail(stream)))
    return out


def direct_reduce(direct, lights, positions, normals, rays, hits, sums, ids=None, view=None, spec=None, device=0, stream=None):
    """fw_direct_reduce: adds one round's reduction (E.rgb, N, S.rgb, each rounded to float32 once) of an api.DirectLight to sums[ids[q]]
    (ids None: sums[q]); sums (M, 8) or (H, W, 8) float32, updated in place; its last float is never written.  rays (n * Ln, 6) float32
    and hits as DeviceScene.trace returns them for those rays: a HIT_DTYPE array for numpy rays, or an (n * Ln, 12) float32 device
    tensor for rays on cuda:`device`, reduced on `stream` (default: the current torch stream) where they lie.  Returns sums."""
    lib = load()
    d = direct.to_abi()
    arr, ln = _light_array(lights)
    pts = _DirectPoints(positions, normals, ids, view, spec, device)
    s = pts.side
    total = pts.n * ln
    if tuple(rays.shape) != (total, 6) or int(hits.shape[0]) != total:
        raise ValueError(f"rays must have shape ({total}, 6) and hits {total} records")
    p_sums = pts.records(sums, "sums", 8)
    r, h = s.inp(rays, (total, 6), "rays"), s.hits(hits, total)
    _check(lib, lib.fw_direct_reduce(int(device), C.byref(d), arr, ln, pts.n, pts.pos, pts.nrm, pts.stride, pts.ids, pts.view, pts.view_stride,
                                     pts.spec, *s.ptrs(r, h), p_sums, *s.tail(stream)))
    return sums


def gather_reduce(surface, irradiance, directions, sums, direct=None, ids=None, device=0, stream=None):
    """fw_gather_reduce: adds one round's reduction (E.rgb, sky, each rounded to float32 once) of a final gather to sums[ids[q]] (ids
    None: sums[q]); sums (M, 4) or (H, W, 4) float32, updated in place.  surface (n * D, 16) float32 as DeviceScene.hit_surface returns
    it, irradiance (n * D, 3) float32 the probe lookup at those records, direct (n * D, 8) float32 as DeviceScene.bake_direct's out for
    them, or None: numpy arrays, or tensors on cuda:`device`, reduced on `stream` (default: the current torch stream) where they lie; ids
    n distinct ids (uint32 numpy / int32 torch).  Returns sums."""
    lib = load()
    d = int(directions)
    total = int(surface.shape[0])
    if d < 1 or total % d or tuple(surface.shape) != (total, 16):
        raise ValueError(f"surface must have shape (n * {d}, 16)")
    n = total // d
    m = int(np.prod(tuple(sums.shape)[:-1]))
    if sums.shape[-1] != 4 or (ids is None and m < n) or (ids is not None and tuple(ids.shape) != (n,)):
        raise ValueError(f"sums must have shape (M, 4) or (H, W, 4) with M >= {n}, ids shape ({n},)")
    s = _Side(surface, device)
    rec, e, ed = s.inp(surface, (total, 16), "surface"), s.inp(irradiance, (total, 3), "irradiance"), s.inp(direct, (total, 8), "direct")
    s.out(sums, tuple(sums.shape), "sums")
    i = s.inp(ids, (n,), "ids", "ids", below=m)
    _check(lib, lib.fw_gather_reduce(int(device), d, n, *s.ptrs(i, rec, e, ed, sums), *s.tail(stream)))
    return sums


def reflect_rays(reflect, positions, normals, view, spec, ids=None, round=0, device=0, out=None, weights=None, stream=None):
    """fw_reflect_rays: the reflection rays of round `round` of an api.ReflectionGather at glossy surface points (see _DirectPoints;
    view and spec are required), generated on the device: (rays (n * D, 6) float32 origin + direction, weights (n * D, 2) float32
    (g, s)), entry q * D + j = ray j of point ids[q] (ids None: q).  numpy points: returns numpy arrays.  Points on cuda:`device`:
    generated on `stream` (default: the current torch stream) where they lie; returns device tensors.  out, weights: contiguous
    float32 arrays or tensors of those shapes to fill instead."""
    lib = load()
    g = reflect.to_abi()
    if view is None or spec is None:
        raise ValueError("reflection rays need view and spec")
    pts = _DirectPoints(positions, normals, ids, view, spec, device)
    s = pts.side
    total = pts.n * int(g.directions)
    out, weights = s.out(out, (total, 6), "out"), s.out(weights, (total, 2), "weights")
    _check(lib, lib.fw_reflect_rays(C.byref(g), int(device), int(round), pts.n, pts.pos, pts.nrm, pts.stride, pts.ids, pts.view, pts.view_stride,
                                    pts.spec, *s.ptrs(out, weights), *s.tail(stream)))
    return out, weights


def reflect_reduce(surface, irradiance, weights, directions, sums, direct=None, ids=None, device=0, stream=None):
    """fw_reflect_reduce: adds one round's reduction (P.rgb, alive, Q.rgb, sky, each rounded to float32 once) of a reflection gather to
    sums[ids[q]] (ids None: sums[q]); sums (M, 8) or (H, W, 8) float32, updated in place.  surface, irradiance and direct as
    gather_reduce takes them, weights (n * D, 2) float32 as reflect_rays returns them: numpy arrays, or tensors on cuda:`device`,
    reduced on `stream` (default: the current torch stream) where they lie; ids n distinct ids (uint32 numpy / int32 torch).
    Returns sums."""
    lib = load()
    d = int(directions)
    total = int(surface.shape[0])
    if d < 1 or total % d or tuple(surface.shape) != (total, 16):
        raise ValueError(f"surface must have shape (n * {d}, 16)")
    n = total // d
    m = int(np.prod(tuple(sums.shape)[:-1]))
    if sums.shape[-1] != 8 or (ids is None and m < n) or (ids is not None and tuple(ids.shape) != (n,)):
        raise ValueError(f"sums must have shape (M, 8) or (H, W, 8) with M >= {n}, ids shape ({n},)")
    s = _Side(surface, device)
    rec, e, ed = s.inp(surface, (total, 16), "surface"), s.inp(irradiance, (total, 3), "irradiance"), s.inp(direct, (total, 8), "direct")
    w = s.inp(weights, (total, 2), "weights")
    s.out(sums, tuple(sums.shape), "sums")
    i = s.inp(ids, (n,), "ids", "ids", below=m)
    _check(lib, lib.fw_reflect_reduce(int(device), d, n, *s.ptrs(i, rec, e, ed, w, sums), *s.tail(stream)))
    return sums


def _light_records(lights):
    """(contiguous (Ln, 16) float32 host array, Ln) of area-light records as light_records / DeviceScene.area_lights return them"""
    rec = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(-1, A.FW_LIGHT_RECORD_FLOATS))
    return rec, int(rec.shape[0])


def _light_objects(objects):
    """(contiguous uint32 host array, Ln) of the lights' object indices; area-light records ((Ln, 16) float32) give their first column"""
    o = np.asarray(objects)
    if o.ndim == 2:
        o = o[:, 0]
    o = np.ascontiguousarray(o.astype(np.uint32).reshape(-1))
    return o, int(o.size)


def area_rays(area, lights, positions, normals, ids=None, round=0, device=0, out=None, weights=None, stream=None):
    """fw_area_rays: the shadow rays of round `round` of an api.AreaLight from surface points (see _AoPoints) towards points drawn on
    `lights` ((Ln, 16) float32 records, a host array always), generated on the device: (rays (n * Ln * S, 6) float32 origin +
    direction, weights (n * Ln * S,) float32), entry (q * Ln + i) * S + s = sample s of light i from point ids[q] (ids None: q); a dead
    entry is six zeros and the weight 0.  numpy points: returns numpy arrays.  Points on cuda:`device`: generated on `stream`
    (default: the current torch stream) where they lie; returns device tensors.  out, weights: contiguous float32 arrays or tensors of
    those shapes to fill instead."""
    lib = load()
    a = area.to_abi()
    rec, ln = _light_records(lights)
    pts = _AoPoints(positions, normals, ids, device)
    s = pts.side
    total = pts.n * ln * int(a.samples)
    out, weights = s.out(out, (total, 6), "out"), s.out(weights, (total,), "weights")
    _check(lib, lib.fw_area_rays(C.byref(a), rec.ctypes.data, ln, int(device), int(round), pts.n, pts.pos, pts.nrm, pts.stride, pts.ids,
                                 *s.ptrs(out, weights), *s.tail(stream)))
    return out, weights


def area_reduce(weights, hits, surface, objects, samples, sums, ids=None, device=0, stream=None):
    """fw_area_reduce: adds one round's reduction (E.rgb, vis, each rounded to float32 once) of an api.AreaLight to sums[ids[q]] (ids
    None: sums[q]); sums (M, 4) or (H, W, 4) float32, updated in place.  weights (n * Ln * S,) float32 as area_rays returns them, hits as
    DeviceScene.trace returns them for those rays, surface (n * Ln * S, 16) float32 as DeviceScene.hit_surface returns it for them: numpy
    arrays (hits a HIT_DTYPE array), or tensors on cuda:`device`, reduced on `stream` (default: the current torch stream) where they
    lie.  objects: the Ln lights' object indices (or their records), a host array always.  Returns sums."""
    lib = load()
    obj, ln = _light_objects(objects)
    m = ln * int(samples)
    total = int(surface.shape[0])
    if m < 1 or total % m or tuple(surface.shape) != (total, 16) or int(hits.shape[0]) != total:
        raise ValueError(f"surface must have shape (n * {m}, 16) and hits n * {m} records")
    n = total // m
    rows = int(np.prod(tuple(sums.shape)[:-1]))
    if sums.shape[-1] != 4 or (ids is None and rows < n) or (ids is not None and tuple(ids.shape) != (n,)):
        raise ValueError(f"sums must have shape (M, 4) or (H, W, 4) with M >= {n}, ids shape ({n},)")
    s = _Side(surface, device)
    w, h, rec = s.inp(weights, (total,), "weights"), s.hits(hits, total), s.inp(surface, (total, 16), "surface")
    s.out(sums, tuple(sums.shape), "sums")
    i = s.inp(ids, (n,), "ids", "ids", below=rows)
    _check(lib, lib.fw_area_reduce(int(device), int(samples), obj.ctypes.data, ln, n, *s.ptrs(i, w, h, rec, sums), *s.tail(stream)))
    return sums


def area_mask(hits, surface, objects, device=0, stream=None):
    """fw_area_mask: rewrites in place — to kind -2, every other float 0 — the records of `surface` ((n, 16) float32, contiguous, the
    caller's own) whose kind is 3 and whose hit lies on one of `objects` (the lights' object indices or their records, ascending; a host
    array always).  hits as DeviceScene.trace returned them: numpy arrays, or tensors on cuda:`device`, rewritten on `stream` (default:
    the current torch stream) where they lie.  Returns surface."""
    lib = load()
    obj, ln = _light_objects(objects)
    n = int(surface.shape[0])
    s = _Side(surface, device)
    h = s.hits(hits, n)
    s.out(surface, (n, 16), "surface")
    _check(lib, lib.fw_area_mask(int(device), obj.ctypes.data, ln, n, *s.ptrs(h, surface), *s.tail(stream)))
    return surface


def emitters_records(scene_desc):
    """fw_selftest_emitters_records (CPU only): the world-space records ((N, 16) float32: object, kind, 12 geometry floats, area, weight)
    and codes ((N, 2) uint32: object, prim) of a SceneDesc's emitter entries, in fw_selftest_emitters' order: what emitters_rays and
    emitters_reduce take"""
    lib = load()
    n = C.c_uint32()
    _check(lib, lib.fw_selftest_emitters_records(scene_desc.ptr(), None, None, 0, C.byref(n)))
    rec, codes = np.zeros((n.value, A.FW_EMITTERS_RECORD_FLOATS), np.float32), np.zeros((n.value, 2), np.uint32)
    if n.value:
        _check(lib, lib.fw_selftest_emitters_records(scene_desc.ptr(), rec.ctypes.data, codes.ctypes.data, n.value, C.byref(n)))
    return rec, codes


def emitters_cdf(weights):
    """fw_emitters_cdf (CPU only): (cdf (N,) float64, total) of float32 weights — the records' last column — as api.emitters_cdf states it;
    total 0 means "no emitters" and the cdf is zeros"""
    lib = load()
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    cdf, total = np.zeros(w.size, np.float64), C.c_double()
    _check(lib, lib.fw_emitters_cdf(w.ctypes.data, int(w.size), cdf.ctypes.data, C.byref(total)))
    return cdf, total.value


def _emitters_list(records, cdf):
    """(contiguous (N, 16) float32 records, contiguous (N,) float64 cdf, N), host arrays"""
    rec = np.ascontiguousarray(np.asarray(records, np.float32).reshape(-1, A.FW_EMITTERS_RECORD_FLOATS))
    c = np.ascontiguousarray(np.asarray(cdf, np.float64).reshape(-1))
    if c.size != rec.shape[0]:
        raise ValueError("cdf must have one value per record")
    return rec, c, int(rec.shape[0])


def _picks(s, picks, total):
    """the picks of a call on side s: the caller's own (a contiguous uint32 array, or an int32 tensor of their bits), or a new one"""
    if picks is None:
        return s.new((total,), "ids")
    if s.on_device:
        _check_device_tensor(picks, (total,), s._dtype("ids"), s.device, "picks")
    elif not (isinstance(picks, np.ndarray) and picks.dtype == np.uint32 and picks.shape == (total,) and picks.flags.c_contiguous):
        raise ValueError(f"picks must be a contiguous uint32 array of shape ({total},)")
    return picks


def emitters_rays(emitters, records, cdf, positions, normals, ids=None, round=0, device=0, out=None, weights=None, picks=None, stream=None):
    """fw_emitters_rays: the shadow rays of round `round` of an api.EmitterLights from surface points (see _AoPoints) towards entries of
    `records` ((N, 16) float32) picked through `cdf` ((N,) float64; host arrays always), generated on the device: (rays (n * S, 6)
    float32, weights (n * S,) float32, picks (n * S,) uint32 — on the device their int32 bits), entry q * S + s = sample s from point
    ids[q] (ids None: q); a dead entry is six zeros, the weight 0 and the pick 0xffffffff.  numpy points: returns numpy arrays.  Points on
    cuda:`device`: generated on `stream` (default: the current torch stream) where they lie; returns device tensors.  out, weights,
    picks: contiguous arrays or tensors of those shapes to fill instead."""
    lib = load()
    a = emitters.to_abi()
    rec, c, ne = _emitters_list(records, cdf)
    pts = _AoPoints(positions, normals, ids, device)
    s = pts.side
    total = pts.n * int(a.samples)
    out, weights, picks = s.out(out, (total, 6), "out"), s.out(weights, (total,), "weights"), _picks(s, picks, total)
    _check(lib, lib.fw_emitters_rays(C.byref(a), rec.ctypes.data, c.ctypes.data, ne, int(device), int(round), pts.n, pts.pos, pts.nrm, pts.stride,
                                     pts.ids, *s.ptrs(out, weights, picks), *s.tail(stream)))
    return out, weights, picks


def emitters_reduce(picks, weights, hits, surface, codes, samples, sums, ids=None, device=0, stream=None):
    """fw_emitters_reduce: adds one round's reduction (E.rgb, vis, each rounded to float32 once) of an api.EmitterLights to sums[ids[q]]
    (ids None: sums[q]); sums (M, 4) or (H, W, 4) float32, updated in place.  picks and weights (n * S,) as emitters_rays returns them,
    hits as DeviceScene.trace returns them for those rays, surface (n * S, 16) float32 as DeviceScene.hit_surface returns it for them:
    numpy arrays (hits a HIT_DTYPE array), or tensors on cuda:`device`, reduced on `stream` (default: the current torch stream) where
    they lie.  codes: (N, 2) uint32 (object, prim) per entry, a host array always.  Returns sums."""
    lib = load()
    cod = np.ascontiguousarray(np.asarray(codes).astype(np.uint32).reshape(-1, 2))
    m = int(samples)
    total = int(surface.shape[0])
    if m < 1 or total % m or tuple(surface.shape) != (total, 16) or int(hits.shape[0]) != total:
        raise ValueError(f"surface must have shape (n * {m}, 16) and hits n * {m} records")
    n = total // m
    rows = int(np.prod(tuple(sums.shape)[:-1]))
    if sums.shape[-1] != 4 or (ids is None and rows < n) or (ids is not None and tuple(ids.shape) != (n,)):
        raise ValueError(f"sums must have shape (M, 4) or (H, W, 4) with M >= {n}, ids shape ({n},)")
    s = _Side(surface, device)
    p, w, h, rec = s.inp(picks, (total,), "picks", "ids"), s.inp(weights, (total,), "weights"), s.hits(hits, total), s.inp(surface, (total, 16), "surface")
    s.out(sums, tuple(sums.shape), "sums")
    i = s.inp(ids, (n,), "ids", "ids", below=rows)
    _check(lib, lib.fw_emitters_reduce(int(device), m, cod.ctypes.data, int(cod.shape[0]), n, *s.ptrs(i, p, w, h, rec, sums), *s.tail(stream)))
    return sums


def _sky_abi(sky):
    """a fw_sky from an api.SunSky (or a fw_sky, copied)"""
    return sky.to_abi() if hasattr(sky, "to_abi") else A.fw_sky.from_buffer_copy(sky)


def check_sky(sky):
    """fw_check_sky: raises FireworkError for what the sky calls refuse in a description; touches no device"""
    lib = load()
    s = _sky_abi(sky)
    _check(lib, lib.fw_check_sky(C.byref(s)))


def sky_map(sky, width, height, device=0, out=None, stream=None):
    """fw_sky_map: the (height, width, 3) float32 equirectangular map of an api.SunSky (or a fw_sky), row 0 at the top, baked on the
    device: what HdrEnvironment takes.  Returns a numpy array; out: a contiguous float32 device tensor of that shape on cuda:`device`
    to fill instead, on `stream` (default: the current torch stream); returned."""
    lib = load()
    sk = _sky_abi(sky)
    s = _Side(out, device)
    out = s.out(out, (int(height), int(width), 3), "out")
    _check(lib, lib.fw_sky_map(C.byref(sk), int(device), int(width), int(height), s.ptr(out), *s.tail(stream)))
    return out


def sky_radiance(sky, dirs, device=0, out=None, stream=None):
    """fw_sky_radiance: the (n, 3) float32 radiance of an api.SunSky along directions of any length.  dirs: (n, k) float32 with k >= 3
    whose rows start with the direction — a view such as rays[:, 3:] of an (n, 6) ray buffer is read in place — as a numpy array
    (returns a numpy array) or a tensor on cuda:`device` (evaluated on `stream`, default the current torch stream, where it lies;
    returns a device tensor).  out: a contiguous float32 array or tensor of that shape to fill instead."""
    lib = load()
    sk = _sky_abi(sky)
    s = _Side(dirs, device)
    if not s.on_device:
        dirs = np.asarray(dirs, dtype=np.float32)
        if dirs.ndim != 2:
            dirs = dirs.reshape(-1, dirs.shape[-1])
    if len(dirs.shape) != 2 or dirs.shape[1] < 3:
        raise ValueError("dirs must have shape (n, k) with k >= 3")
    n = int(dirs.shape[0])
    (d,), stride = s.columns(n, (dirs[:, :3], "dirs"))
    out = s.out(out, (n, 3), "out")
    _check(lib, lib.fw_sky_radiance(C.byref(sk), int(device), n, s.ptr(d), stride, s.ptr(out), *s.tail(stream)))
    return out


def sky_sun(sky):
    """fw_sky_sun: the sun of an api.SunSky as a fw_light (FW_LIGHT_DIRECTIONAL, direction -s, irradiance E0 T(O)); host only"""
    lib = load()
    s = _sky_abi(sky)
    out = A.fw_light()
    _check(lib, lib.fw_sky_sun(C.byref(s), C.byref(out)))
    return out


def _quad_abi(quad):
    """a fw_ggx_quad from an api.GgxTable, an (m1, m2) pair or a fw_ggx_quad (copied)"""
    if hasattr(quad, "to_abi"):
        return quad.to_abi()
    if isinstance(quad, A.fw_ggx_quad):
        return A.fw_ggx_quad.from_buffer_copy(quad)
    return A.fw_ggx_quad(int(quad[0]), int(quad[1]))


def check_ggx_quad(quad):
    """fw_check_ggx_quad: raises FireworkError for a quadrature the table calls refuse; touches no device"""
    lib = load()
    q = _quad_abi(quad)
    _check(lib, lib.fw_check_ggx_quad(C.byref(q)))


def _pairs_arg(s, mu, rho):
    """(n, mu, rho) of a list of (mu, rho) pairs: contiguous float32 (n,) arrays on the side `s` of the call"""
    n = s.count(mu, 1)
    return n, s.inp(mu, (n,), "mu"), s.inp(rho, (n,), "rho")


def ggx_terms(quad, mu, rho, device=0, out=None, stream=None):
    """fw_ggx_terms: the (n, 2) float32 terms (A, B) of GgxMat's directional albedo F0 A + B at the pairs (mu[q], rho[q]), integrated on
    the device with the quadrature `quad` (an api.GgxTable, an (m1, m2) pair or a fw_ggx_quad).  numpy arrays: returns a numpy array.
    Contiguous float32 tensors on cuda:`device`: evaluated on `stream` (default: the current torch stream) where they lie; returns a
    device tensor.  out: an array or tensor of that shape to fill instead."""
    lib = load()
    q = _quad_abi(quad)
    s = _Side(mu, device)
    n, m, r = _pairs_arg(s, mu, rho)
    out = s.out(out, (n, 2), "out")
    _check(lib, lib.fw_ggx_terms(C.byref(q), int(device), n, *s.ptrs(m, r, out), *s.tail(stream)))
    return out


def ggx_table(quad, n_mu=None, n_rho=None, device=0, out=None, stream=None):
    """fw_ggx_table: the (n_rho, n_mu, 2) float32 table of the terms (A, B) at the texel centres, baked on the device.  quad: an
    api.GgxTable (whose n_mu and n_rho are the defaults), an (m1, m2) pair or a fw_ggx_quad.  Returns a numpy array; out: a contiguous
    float32 device tensor of that shape on cuda:`device` to fill instead, on `stream` (default: the current torch stream); returned."""
    lib = load()
    q = _quad_abi(quad)
    if (n_mu is None or n_rho is None) and not hasattr(quad, "n_mu"):
        raise ValueError("n_mu and n_rho are needed with a quadrature that is not an api.GgxTable")
    n_mu = int(quad.n_mu if n_mu is None else n_mu)
    n_rho = int(quad.n_rho if n_rho is None else n_rho)
    s = _Side(out, device)
    out = s.out(out, (n_rho, n_mu, 2), "out")
    _check(lib, lib.fw_ggx_table(C.byref(q), int(device), n_mu, n_rho, s.ptr(out), *s.tail(stream)))
    return out


def ggx_table_lookup(table, mu, rho, device=0, out=None, stream=None):
    """fw_ggx_table_lookup: the (n, 2) float32 bilinear lookup of an (n_rho, n_mu, 2) table at the pairs (mu[q], rho[q]), edges clamped,
    zeros for a non-finite pair.  numpy arrays or contiguous float32 tensors on cuda:`device` (the table too), as ggx_terms."""
    lib = load()
    s = _Side(mu, device)
    n, m, r = _pairs_arg(s, mu, rho)
    tp, n_mu, n_rho = _table_arg(s, table)
    out = s.out(out, (n, 2), "out")
    _check(lib, lib.fw_ggx_table_lookup(int(device), n_mu, n_rho, tp, n, *s.ptrs(m, r, out), *s.tail(stream)))
    return out


class DeviceScene:
    """An uploaded scene (`fw_scene*`): SoA scene arrays + TLAS/BLAS resident in HBM."""

    def __init__(self, scene_desc, device=0):
        lib = load()
        self._lib = lib
        self._desc = scene_desc  # keep host buffers alive
        h = C.c_void_p()
        _check(lib, lib.fw_scene_create(scene_desc.ptr(), device, C.byref(h)))
        self.handle = h
        self.device = device
        self._desc_lights = b""              # the lights the latest description carried, as set
        if getattr(scene_desc, "lights", None):
            self.set_lights(scene_desc.lights)
            self._desc_lights = bytes(_light_array(scene_desc.lights)[0])

    def set_lights(self, lights):
        """fw_scene_set_lights: replaces this resident scene's point, spot and directional lights; an empty list removes
        them.  FireworkError for a list the library refuses (the scene is then as it was)."""
        arr, n = _light_array(lights)
        _check(self._lib, self._lib.fw_scene_set_lights(self.handle, arr, n))

    def update(self, scene):
        """fw_scene_update: moves the objects of this resident scene.  `scene` is a SceneDesc of the scene this one was created from with
        other object placements (position, rotation, flip_normals), or that Scene itself after its RenderObjects were moved: then only a
        new fw_object array is built and the kept description's shape, material, texture and environment arrays are reused (no mesh,
        image or HDR array is converted again).  Every later call equals the same call on DeviceScene(the moved scene) bit for bit.
        ValueError if the Scene's objects no longer map to the same shapes; FireworkError for what the library rejects (the scene is
        then as it was)."""
        from .api import Scene
        desc = self._desc.placements(scene) if isinstance(scene, Scene) else scene
        _check(self._lib, self._lib.fw_scene_update(self.handle, desc.ptr()))
        self._desc = desc
        # (fw_scene_update keeps the lights; a description whose lights differ from the last description's has them set again)
        lights = getattr(desc, "lights", None) or []
        arr, n = _light_array(lights)
        if (bytes(arr) if n else b"") != getattr(self, "_desc_lights", b""):     # (a scene wrapped without __init__ has set none)
            self.set_lights(lights)
            self._desc_lights = bytes(arr) if n else b""

    def render(self, renderer, pixel_ids=None, out_device_ptrs=None, stream=None):
        """fw_render.  out_device_ptrs = (rgb8, gamma, linear) raw device pointers (ints or None) to
        keep results in HBM (multi-GPU gather path); otherwise numpy host arrays are returned."""
        from .api import RenderResult
        lib = self._lib
        p = renderer.to_params(pixel_ids)
        n = int(pixel_ids.shape[0]) if pixel_ids is not None else p.width * p.height
        st = A.fw_stats()
        if out_device_ptrs is not None:
            p.outputs_on_device = 1
            p.stream = C.c_void_p(stream) if stream else None
            ptrs = [C.c_void_p(x) if x else None for x in out_device_ptrs]
            _check(lib, lib.fw_render(self.handle, C.byref(p), ptrs[0], ptrs[1], ptrs[2], C.byref(st)))
            return st.as_dict()
        rgb8 = np.empty((n, 3), np.uint8)
        gam = np.empty((n, 3), np.float32)
        lin = np.empty((n, 3), np.float32)
        _check(lib, lib.fw_render(self.handle, C.byref(p), rgb8.ctypes.data, gam.ctypes.data, lin.ctypes.data,
                                  C.byref(st)))
        return RenderResult(rgb8, gam, lin, st.as_dict(), p.width, p.height)

    def render_progressive(self, renderer, first_sample, accum, pixel_ids=None):
        """fw_render_progressive: adds samples [first_sample, first_sample + renderer's samples) to `accum`
        ((n_pixels, 4) float32, zeros before the first call; updated in place) and returns the image resolved so far."""
        from .api import RenderResult
        lib = self._lib
        p = renderer.to_params(pixel_ids)
        n = int(pixel_ids.shape[0]) if pixel_ids is not None else p.width * p.height
        assert accum.dtype == np.float32 and accum.shape == (n, 4) and accum.flags["C_CONTIGUOUS"]
        st = A.fw_stats()
        rgb8 = np.empty((n, 3), np.uint8)
        gam = np.empty((n, 3), np.float32)
        lin = np.empty((n, 3), np.float32)
        _check(lib, lib.fw_render_progressive(self.handle, C.byref(p), int(first_sample), accum.ctypes.data, rgb8.ctypes.data,
                                              gam.ctypes.data, lin.ctypes.data, C.byref(st)))
        return RenderResult(rgb8, gam, lin, st.as_dict(), p.width, p.height)

    def render_adaptive(self, renderer, tolerance, min_samples=16, out=None, stream=None):
        """fw_render_adaptive: the whole frame, each pixel rendered until its noise estimate meets `tolerance` or its count reaches the
        renderer's samples (the cap).  Returns an AdaptiveResult (host numpy arrays).  out: a dict of contiguous device tensors on this
        scene's device to fill instead (keys rgb8 (n, 3) uint8, gamma, linear (n, 3) float32, accum, moments (n, 4) float32,
        round_pixels (32,) int32; any may be missing), launched on `stream` (default: the current torch stream); returns the
        AdaptiveResult with those tensors in place of arrays."""
        from .api import AdaptiveResult
        lib = self._lib
        p = renderer.to_params(None)
        n = p.width * p.height
        st = A.fw_stats()
        if out is not None:
            import torch
            want = dict(rgb8=((n, 3), torch.uint8), gamma=((n, 3), torch.float32), linear=((n, 3), torch.float32),
                        accum=((n, 4), torch.float32), moments=((n, 4), torch.float32), round_pixels=((32,), torch.int32))
            for k, t in out.items():
                shape, dt = want[k]
                if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device.type != "cuda" or (t.device.index or 0) != self.device:
                    raise ValueError(f"out[{k!r}] must be a contiguous {dt} tensor of shape {shape} on cuda:{self.device}")
            p.outputs_on_device = 1
            p.stream = _stream_arg(stream, torch.device("cuda", self.device))
            ptr = {k: (out[k].data_ptr() if k in out else None) for k in want}
            _check(lib, lib.fw_render_adaptive(self.handle, C.byref(p), float(tolerance), int(min_samples), ptr["accum"], ptr["moments"],
                                               ptr["rgb8"], ptr["gamma"], ptr["linear"], ptr["round_pixels"], C.byref(st)))
            return AdaptiveResult(out.get("rgb8"), out.get("gamma"), out.get("linear"), out.get("accum"), out.get("moments"),
                                  out.get("round_pixels"), st.as_dict(), p.width, p.height)
        rgb8 = np.empty((n, 3), np.uint8)
        gam = np.empty((n, 3), np.float32)
        lin = np.empty((n, 3), np.float32)
        acc = np.empty((n, 4), np.float32)
        mom = np.empty((n, 4), np.float32)
        rounds = np.zeros(32, np.uint32)
        _check(lib, lib.fw_render_adaptive(self.handle, C.byref(p), float(tolerance), int(min_samples), acc.ctypes.data, mom.ctypes.data,
                                           rgb8.ctypes.data, gam.ctypes.data, lin.ctypes.data, rounds.ctypes.data, C.byref(st)))
        return AdaptiveResult(rgb8, gam, lin, acc, mom, rounds, st.as_dict(), p.width, p.height)

    def render_views(self, renderer, cameras, pixel_ids=None, out_device_ptrs=None, stream=None):
        """fw_render_views: one render per camera in one call, each equal bit for bit to render() with that camera (the renderer's own
        camera is ignored).  cameras: CameraSettings or fw_camera_settings.  Returns a ViewsResult with (V, N, 3) host arrays, N =
        len(pixel_ids) or width * height.  out_device_ptrs = (rgb8, gamma, linear) raw device pointers (ints or None) of V * N * 3 values
        each to fill instead, launched on `stream` (a raw hipStream_t, or None for the null stream); returns the stats dict then."""
        from .api import ViewsResult
        lib = self._lib
        p = renderer.to_params(pixel_ids)
        n = int(pixel_ids.shape[0]) if pixel_ids is not None else p.width * p.height
        cams = (A.fw_camera_settings * max(1, len(cameras)))(*[c if isinstance(c, A.fw_camera_settings) else c.to_abi() for c in cameras])
        v = len(cameras)
        st = A.fw_stats()
        if out_device_ptrs is not None:
            p.outputs_on_device = 1
            p.stream = C.c_void_p(stream) if stream else None
            ptrs = [C.c_void_p(x) if x else None for x in out_device_ptrs]
            _check(lib, lib.fw_render_views(self.handle, C.byref(p), cams, v, ptrs[0], ptrs[1], ptrs[2], C.byref(st)))
            return st.as_dict()
        rgb8 = np.empty((v, n, 3), np.uint8)
        gam = np.empty((v, n, 3), np.float32)
        lin = np.empty((v, n, 3), np.float32)
        _check(lib, lib.fw_render_views(self.handle, C.byref(p), cams, v, rgb8.ctypes.data, gam.ctypes.data, lin.ctypes.data, C.byref(st)))
        return ViewsResult(rgb8, gam, lin, st.as_dict(), p.width, p.height, pixel_ids is not None)

    def _rays_call(self, fn, head, p, s, stream, accum):
        """what render_rays and render_model share: fn(scene, *head, accum, rgb8, gamma, linear, stats) with accum (N, 4) float32 updated
        in place (None: zeros) and three new outputs on the side `s`.  Returns the RaysResult."""
        from .api import RaysResult
        n = int(p.n_rays)
        st = A.fw_stats()
        accum = s.out(accum, (n, 4), "accum", fill=0.0)
        rgb8, gam, lin = s.new((n, 3), "u8"), s.new((n, 3)), s.new((n, 3))
        s.params(p, stream)
        _check(self._lib, fn(self.handle, *head, *s.ptrs(accum, rgb8, gam, lin), C.byref(st)))
        return RaysResult(rgb8, gam, lin, accum, st.as_dict())

    def render_rays(self, rays, samples, first_sample=0, accum=None, keys=None, key_base=0, seed=0, use_bvh=True, gamma=2.2, stream=None,
                    paths_per_batch=0, flags=0):
        """fw_render_rays: radiance along the caller's rays, samples [first_sample, first_sample + samples) of N entries.  rays: (S, N, 6)
        float32 origin + direction per sample (S = samples; rays[s] is absolute sample first_sample + s), or (N, 6) for the same rays in
        every sample.  Draws of entry i are keyed by keys[i] (N uint32) or key_base + i.  accum: (N, 4) float32 sums of the samples
        before first_sample (updated in place; None: zeros, only with first_sample 0).
        - numpy arrays: returns a RaysResult of host arrays (rgb8 (N, 3) uint8, gamma / linear (N, 3) float32, accum (N, 4)).
        - contiguous torch tensors on this scene's device (rays, and keys / accum when given): rendered on `stream` (default: the current
          torch stream) into new device tensors; returns a RaysResult of tensors.  Device rays are the fast path: host rays pass
          through pinned staging batch by batch."""
        shape = tuple(rays.shape)
        if len(shape) == 3 and shape[2] == 6 and shape[0] == int(samples):
            per_sample, n = 1, int(shape[1])
        elif len(shape) == 2 and shape[1] == 6:
            per_sample, n = 0, int(shape[0])
        else:
            raise ValueError(f"rays must have shape (samples={int(samples)}, N, 6) or (N, 6), not {shape}")
        p = A.fw_render_rays_params()
        p.n_rays, p.first_sample, p.samples, p.per_sample_rays = n, int(first_sample), int(samples), per_sample
        p.key_base, p.seed, p.use_bvh, p.gamma = int(key_base), int(seed), int(bool(use_bvh)), float(gamma)
        p.paths_per_batch, p.flags = int(paths_per_batch), int(flags)
        s = _Side(rays, self.device)
        r = s.inp(rays, shape, "rays")
        if keys is not None:
            p.keys = C.cast(C.c_void_p(s.ptr(s.inp(keys, (n,), "keys", "ids"))), C.POINTER(C.c_uint32))      # (on the device: the bits of uint32 keys)
        return self._rays_call(self._lib.fw_render_rays, (C.byref(p), s.ptr(r)), p, s, stream, accum)

    def render_model(self, model, samples, first_sample=0, accum=None, key_base=0, seed=0, use_bvh=True, gamma=2.2, stream=None,
                     paths_per_batch=0, flags=0, chunk=None, on_device=False):
        """fw_render_model: samples [first_sample, first_sample + samples) of a camera model (an api.CameraModel or a fw_camera_model)
        whose rays are generated on the device, chunk samples at a time (None: the model's own setting; 0: automatic).  Bit for bit
        render_rays() over model_rays().  accum: (W * H, 4) float32 sums of the samples before first_sample, updated in place (None:
        zeros, only with first_sample 0).  Returns a RaysResult of host arrays, or — accum a device tensor on this scene's device, or
        on_device=True — of device tensors, rendered on `stream` (default: the current torch stream)."""
        m = _model_abi(model, chunk)
        p = A.fw_render_rays_params()
        p.n_rays, p.first_sample, p.samples, p.per_sample_rays = int(m.width) * int(m.height), int(first_sample), int(samples), 1
        p.key_base, p.seed, p.use_bvh, p.gamma = int(key_base), int(seed), int(bool(use_bvh)), float(gamma)
        p.paths_per_batch, p.flags = int(paths_per_batch), int(flags)
        return self._rays_call(self._lib.fw_render_model, (C.byref(m), C.byref(p)), p, _Side(accum, self.device, on_device), stream, accum)

    def model_aovs(self, model, samples, seed=0, use_bvh=True, out=None, stream=None):
        """fw_render_model_aovs: aovs() for a camera model (an api.CameraModel or a fw_camera_model) — the (W * H, 12) float32 first-hit
        guide records of the model's rays averaged over `samples` samples, keyed by `seed` as a render through the model keys its
        paths.  out: a contiguous (W * H, 12) float32 device tensor on this scene's device to fill instead, on `stream` (default: the
        current torch stream); returned.  stats: see aovs_stats after the call."""
        lib = self._lib
        m = _model_abi(model)
        n = int(m.width) * int(m.height)
        p = A.fw_render_params()
        p.samples, p.use_bvh, p.seed = int(samples), int(bool(use_bvh)), int(seed)
        st = A.fw_stats()
        if out is not None:
            import torch
            _check_device_tensor(out, (n, 12), torch.float32, self.device, "out")
            p.outputs_on_device = 1
            p.stream = _stream_arg(stream, torch.device("cuda", self.device))
            _check(lib, lib.fw_render_model_aovs(self.handle, C.byref(m), C.byref(p), out.data_ptr(), C.byref(st)))
            self.aovs_stats = st.as_dict()
            return out
        aov = np.empty((n, 12), np.float32)
        _check(lib, lib.fw_render_model_aovs(self.handle, C.byref(m), C.byref(p), aov.ctypes.data, C.byref(st)))
        self.aovs_stats = st.as_dict()
        return aov

    def _bake(self, fn, s, extra, shape, rounds, samples, first_round, sums, seed, use_bvh, stream, paths_per_batch, flags, on_device):
        """what bake_probes and bake_lightmap share: the bound C function `fn` over its ABI struct `s`, the rounds and the integers `extra`
        that follow them; sums and the result have `shape`.  Returns (result, sums, stats)."""
        p = A.fw_render_rays_params()
        p.samples, p.seed, p.use_bvh, p.gamma = int(samples), int(seed), int(bool(use_bvh)), 1.0
        p.paths_per_batch, p.flags = int(paths_per_batch), int(flags)
        st = A.fw_stats()
        side = _Side(sums, self.device, on_device)
        sums = side.out(sums, shape, "sums", fill=0.0)
        out = side.new(shape)
        side.params(p, stream)
        _check(self._lib, fn(self.handle, C.byref(s), C.byref(p), int(first_round), int(rounds), *extra, *side.ptrs(sums, out), C.byref(st)))
        return out, sums, st.as_dict()

    def bake_probes(self, probes, rounds, samples, first_round=0, sums=None, seed=0, use_bvh=True, stream=None, paths_per_batch=0, flags=0,
                    chunk=None, on_device=False):
        """fw_bake_probes: the rounds [first_round, first_round + rounds) of an api.ProbeSet, `samples` paths per direction and round,
        `chunk` probes at a time (None: the set's own setting; 0: automatic).  sums: (N, 9, 3) float32 running sums of the rounds
        before first_round, updated in place (None: zeros, only with first_round 0).  Returns (sh, sums, stats): host arrays, or —
        sums a device tensor on this scene's device, or on_device=True — device tensors, baked on `stream` (default: the current
        torch stream).  sh = sums / (first_round + rounds)."""
        s, _pos = _probe_abi(probes, chunk)
        return self._bake(self._lib.fw_bake_probes, s, (), (int(s.n_probes), 9, 3), rounds, samples, first_round, sums, seed, use_bvh, stream,
                          paths_per_batch, flags, on_device)

    def bake_probe_depth(self, probes, depth, rounds=1, first_round=0, sums=None, seed=0, use_bvh=True, stream=None, rays_per_batch=0, flags=0,
                         chunk=None, on_device=False):
        """fw_bake_probe_depth: the rounds [first_round, first_round + rounds) of the depth maps (an api.ProbeDepth) of an api.ProbeSet,
        `chunk` probes at a time (None: the set's own setting; 0: automatic).  sums: (N, R, R, 4) float32 running sums of the rounds
        before first_round, updated in place (None: zeros, only with first_round 0).  Returns (moments, sums, stats): moments (N, R, R,
        2) float32 (mu, mu2); host arrays, or — sums a device tensor on this scene's device, or on_device=True — device tensors, baked
        on `stream` (default: the current torch stream)."""
        s, _pos = _probe_abi(probes, chunk)
        pd = depth.to_abi()
        n, R = int(s.n_probes), int(pd.resolution)
        p = A.fw_trace_params()
        p.use_bvh, p.flags, p.seed, p.rays_per_batch = int(bool(use_bvh)), int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(rays_per_batch)
        st = A.fw_stats()
        side = _Side(sums, self.device, on_device)
        sums = side.out(sums, (n, R, R, 4), "sums", fill=0.0)
        out = side.new((n, R, R, 2))
        side.params(p, stream)
        _check(self._lib, self._lib.fw_bake_probe_depth(self.handle, C.byref(s), C.byref(pd), C.byref(p), int(first_round), int(rounds),
                                                        *side.ptrs(sums, out), C.byref(st)))
        return out, sums, st.as_dict()

    def bake_probe_radiance(self, probes, radiance, rounds, samples, first_round=0, sums=None, sh_sums=None, with_sh=False, seed=0, use_bvh=True,
                            stream=None, paths_per_batch=0, flags=0, chunk=None, on_device=False):
        """fw_bake_probe_radiance: the rounds [first_round, first_round + rounds) of the radiance maps (an api.ProbeRadiance) of an
        api.ProbeSet, `samples` paths per direction and round, `chunk` probes at a time (None: the set's own setting; 0: automatic).
        sums: (N, R, R, 4) float32 running sums of the rounds before first_round, updated in place (None: zeros, only with first_round
        0).  with_sh (or sh_sums, bake_probes' running sums): the same rendered rays are also projected onto SH as bake_probes does.
        Returns (maps, sums, stats), or with SH (maps, sums, sh, sh_sums, stats): maps (N, M, 4) float32; host arrays, or — sums a device
        tensor on this scene's device, or on_device=True — device tensors, baked on `stream` (default: the current torch stream)."""
        s, _pos = _probe_abi(probes, chunk)
        pr = radiance.to_abi()
        n, R, M = int(s.n_probes), int(pr.resolution), int(radiance.texels)
        with_sh = bool(with_sh) or sh_sums is not None
        p = A.fw_render_rays_params()
        p.samples, p.seed, p.use_bvh, p.gamma = int(samples), int(seed), int(bool(use_bvh)), 1.0
        p.paths_per_batch, p.flags = int(paths_per_batch), int(flags)
        st = A.fw_stats()
        side = _Side(sh_sums if sums is None else sums, self.device, on_device)
        sums = side.out(sums, (n, R, R, 4), "sums", fill=0.0)
        maps = side.new((n, M, 4))
        sh = None
        if with_sh:
            sh_sums = side.out(sh_sums, (n, 9, 3), "sh_sums", fill=0.0)
            sh = side.new((n, 9, 3))
        side.params(p, stream)
        _check(self._lib, self._lib.fw_bake_probe_radiance(self.handle, C.byref(s), C.byref(pr), C.byref(p), int(first_round), int(rounds),
                                                           *side.ptrs(sums, maps, sh_sums, sh), C.byref(st)))
        if with_sh:
            return maps, sums, sh, sh_sums, st.as_dict()
        return maps, sums, st.as_dict()

    def relocate_probes(self, probes, relocation, steps=None, first_step=0, placement=None, seed=0, use_bvh=True, stream=None, rays_per_batch=0,
                        flags=0, chunk=None):
        """fw_relocate_probes: the steps [first_step, first_step + steps) of an api.ProbeRelocation (steps None: its own count) over an
        api.ProbeSet at its nominal positions, then one classifying step; `chunk` probes at a time (None: the set's own setting; 0:
        automatic).  placement: (N, 4) float32 host records (ox, oy, oz, a), updated in place (None: the neutral (0, 0, 0, 1)).
        Returns (placement, survey, stats): host arrays always; survey (N, 3, 4) float32 is the classifying step's."""
        s, _pos = _probe_abi(probes, chunk)
        rl = relocation.to_abi(probes)
        n = int(s.n_probes)
        if placement is None:
            placement = np.zeros((n, 4), np.float32)
            placement[:, 3] = 1.0
        _host_f32(placement, (n, 4), "placement")
        survey = np.empty((n, 3, 4), np.float32)
        p = A.fw_trace_params()
        p.use_bvh, p.flags, p.seed, p.rays_per_batch = int(bool(use_bvh)), int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(rays_per_batch)
        if stream is not None:
            p.stream = C.c_void_p(stream) if stream else None
        st = A.fw_stats()
        k = int(relocation.steps if steps is None else steps)
        _check(self._lib, self._lib.fw_relocate_probes(self.handle, C.byref(s), C.byref(rl), C.byref(p), int(first_step), k, placement.ctypes.data,
                                                       survey.ctypes.data, C.byref(st)))
        return placement, survey, st.as_dict()

    def _bake_points(self, fn, desc, pts, floats, head, rounds, first_round, sums, out, seed, use_bvh, stream, rays_per_batch, flags, out_floats=None):
        """what the point bakers share: the bound C function `fn` over its description `desc`, the points `pts` with the arguments
        `head` that state them, and sums of `floats` and out of `out_floats` (None: `floats`) floats per point (None: zeros).  Returns
        (out, sums, stats)."""
        out_floats = floats if out_floats is None else out_floats
        p = A.fw_trace_params()
        p.use_bvh, p.flags, p.seed, p.rays_per_batch = int(bool(use_bvh)), int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(rays_per_batch)
        st = A.fw_stats()
        if sums is None and int(first_round) > 0:
            raise ValueError("first_round > 0 needs the sums of the rounds before it")
        pts.side.params(p, stream)
        sums = pts.side.new((pts.m, floats), fill=0.0) if sums is None else sums
        out = pts.side.new((pts.m, out_floats), fill=0.0) if out is None else out
        _check(self._lib, fn(self.handle, C.byref(desc), C.byref(p), *head, int(first_round), int(rounds), pts.records(sums, "sums", floats),
                             pts.records(out, "out", out_floats), C.byref(st)))
        return out, sums, st.as_dict()

    def bake_ao(self, ao, positions, normals, ids=None, rounds=1, first_round=0, sums=None, out=None, seed=0, use_bvh=True, stream=None,
                rays_per_batch=0, flags=0, chunk=None):
        """fw_bake_ao: the rounds [first_round, first_round + rounds) of an api.AmbientOcclusion around surface points (see _AoPoints:
        numpy arrays, or tensors on this scene's device, read in place), `chunk` points at a time (None: the description's own
        setting; 0: automatic).  sums: (M, 4) or (H, W, 4) float32 running sums (Bx, By, Bz, O) of the rounds before first_round,
        updated in place (None: zeros, only with first_round 0); out: an array of the same kind to receive (bent.xyz, ao) (None:
        zeros); both are indexed by id, entries outside ids are not touched.  Returns (out, sums, stats): host arrays for numpy
        points, device tensors — baked on `stream` (default: the current torch stream) — for device points."""
        a = ao.to_abi()
        if chunk is not None:
            a.chunk_points = int(chunk)
        pts = _AoPoints(positions, normals, ids, self.device)
        return self._bake_points(self._lib.fw_bake_ao, a, pts, 4, (pts.n, pts.pos, pts.nrm, pts.stride, pts.ids), rounds, first_round, sums, out,
                                 seed, use_bvh, stream, rays_per_batch, flags)

    def bake_direct(self, direct, positions, normals, ids=None, view=None, spec=None, rounds=1, first_round=0, sums=None, out=None, seed=0,
                    use_bvh=True, stream=None, rays_per_batch=0, flags=0, chunk=None):
        """fw_bake_direct: the rounds [first_round, first_round + rounds) of an api.DirectLight at surface points (see _DirectPoints:
        numpy arrays, or tensors on this scene's device, read in place) under this scene's own lights (set_lights), `chunk` points at a
        time (None: the description's own setting; 0: automatic).  sums: (M, 8) or (H, W, 8) float32 running sums (E.rgb, N, S.rgb, -)
        of the rounds before first_round, updated in place (None: zeros, only with first_round 0); out: an array of the same kind to
        receive sums / rounds (None: zeros); both are indexed by id, entries outside ids are not touched.  Returns (out, sums, stats):
        host arrays for numpy points, device tensors — baked on `stream` (default: the current torch stream) — for device points."""
        d = direct.to_abi()
        if chunk is not None:
            d.chunk_points = int(chunk)
        pts = _DirectPoints(positions, normals, ids, view, spec, self.device)
        head = (pts.n, pts.pos, pts.nrm, pts.stride, pts.ids, pts.view, pts.view_stride, pts.spec)
        return self._bake_points(self._lib.fw_bake_direct, d, pts, 8, head, rounds, first_round, sums, out, seed, use_bvh, stream, rays_per_batch,
                                 flags)

    def bake_gather(self, gather, grid, sh, positions, normals, ids=None, depth=None, moments=None, normal_bias=0.0, placement=None, rounds=1,
                    first_round=0, sums=None, out=None, seed=0, use_bvh=True, stream=None, rays_per_batch=0, flags=0, chunk=None):
        """fw_bake_gather: the rounds [first_round, first_round + rounds) of an api.FinalGather at surface points (see _AoPoints: numpy
        arrays, or tensors on this scene's device, read in place) against this scene and the baked probes (grid, sh; depth + moments:
        the visibility weight; placement: moved and classified probes), of the points' kind, `chunk` points at a time (None: the
        description's own setting; 0: automatic).  sums: (M, 4) or (H, W, 4) float32 running sums (Er, Eg, Eb, sky) of the rounds before
        first_round, updated in place (None: zeros, only with first_round 0); out: an array of the same kind to receive sums / rounds
        (None: zeros); both are indexed by id, entries outside ids are not touched.  Returns (out, sums, stats): host arrays for numpy
        points, device tensors — baked on `stream` (default: the current torch stream) — for device points."""
        g = gather.to_abi()
        if chunk is not None:
            g.chunk_points = int(chunk)
        pts = _AoPoints(positions, normals, ids, self.device)
        s = pts.side
        gr, n_probes = _grid_abi(grid)
        vis = _vis_of(depth, moments, normal_bias)
        head = (C.byref(gr), s.ptr(s.inp(sh, (n_probes, 9, 3), "sh")), *_vis_args(s, vis, n_probes), _placement_arg(s, placement, n_probes),
                pts.n, pts.pos, pts.nrm, pts.stride, pts.ids)
        return self._bake_points(self._lib.fw_bake_gather, g, pts, 4, head, rounds, first_round, sums, out, seed, use_bvh, stream, rays_per_batch,
                                 flags)

    def bake_reflect(self, reflect, grid, sh, positions, normals, view, spec, ids=None, depth=None, moments=None, normal_bias=0.0, placement=None,
                     rounds=1, first_round=0, sums=None, out=None, seed=0, use_bvh=True, stream=None, rays_per_batch=0, flags=0, chunk=None):
        """fw_bake_reflect: the rounds [first_round, first_round + rounds) of an api.ReflectionGather at glossy surface points (see
        _DirectPoints: numpy arrays, or tensors on this scene's device, read in place; view (M, 3) and spec (M, 4) are required)
        against this scene and the baked probes (grid, sh; depth + moments: the visibility weight; placement: moved and classified
        probes), `chunk` points at a time (None: the description's own setting; 0: automatic).  sums: (M, 8) or (H, W, 8) float32
        running sums (P.rgb, alive, Q.rgb, sky) of the rounds before first_round, updated in place (None: zeros, only with first_round
        0); out: (M, 4) or (H, W, 4) float32 to receive (S.rgb, alive) (None: zeros); both are indexed by id, entries outside ids are
        not touched.  Returns (out, sums, stats): host arrays for numpy points, device tensors — baked on `stream` (default: the
        current torch stream) — for device points."""
        g = reflect.to_abi()
        if chunk is not None:
            g.chunk_points = int(chunk)
        if view is None or spec is None:
            raise ValueError("a reflection gather needs view and spec")
        pts = _DirectPoints(positions, normals, ids, view, spec, self.device)
        s = pts.side
        gr, n_probes = _grid_abi(grid)
        vis = _vis_of(depth, moments, normal_bias)
        head = (C.byref(gr), s.ptr(s.inp(sh, (n_probes, 9, 3), "sh")), *_vis_args(s, vis, n_probes), _placement_arg(s, placement, n_probes),
                pts.n, pts.pos, pts.nrm, pts.stride, pts.ids, pts.view, pts.view_stride, pts.spec)
        return self._bake_points(self._lib.fw_bake_reflect, g, pts, 8, head, rounds, first_round, sums, out, seed, use_bvh, stream, rays_per_batch,
                                 flags, out_floats=4)

    def area_lights(self):
        """fw_scene_area_lights: the records of this resident scene's sampled area lights — every EmissiveMat sphere and axis-aligned
        rectangle, where fw_scene_update last put them — as (Ln, 16) float32 (object, kind, 12 geometry floats, area, p_pick), in
        ascending object order: what area_rays takes as `lights`."""
        n = C.c_uint32()
        _check(self._lib, self._lib.fw_scene_area_lights(self.handle, None, 0, C.byref(n)))
        out = np.zeros((n.value, A.FW_LIGHT_RECORD_FLOATS), np.float32)
        if n.value:
            _check(self._lib, self._lib.fw_scene_area_lights(self.handle, out.ctypes.data, n.value, C.byref(n)))
        return out

    def bake_area(self, area, positions, normals, ids=None, rounds=1, first_round=0, sums=None, out=None, seed=0, use_bvh=True, stream=None,
                  rays_per_batch=0, flags=0, chunk=None):
        """fw_bake_area: the rounds [first_round, first_round + rounds) of an api.AreaLight at surface points (see _AoPoints: numpy
        arrays, or tensors on this scene's device, read in place) under this scene's own sampled area lights (area_lights), `chunk`
        points at a time (None: the description's own setting; 0: automatic).  sums: (M, 4) or (H, W, 4) float32 running sums (Er, Eg,
        Eb, vis) of the rounds before first_round, updated in place (None: zeros, only with first_round 0); out: an array of the same
        kind to receive sums / rounds (None: zeros); both are indexed by id, entries outside ids are not touched.  Returns (out, sums,
        stats): host arrays for numpy points, device tensors — baked on `stream` (default: the current torch stream) — for device
        points."""
        a = area.to_abi()
        if chunk is not None:
            a.chunk_points = int(chunk)
        pts = _AoPoints(positions, normals, ids, self.device)
        return self._bake_points(self._lib.fw_bake_area, a, pts, 4, (pts.n, pts.pos, pts.nrm, pts.stride, pts.ids), rounds, first_round, sums, out,
                                 seed, use_bvh, stream, rays_per_batch, flags)

    def emitters(self):
        """fw_scene_emitters: (records (N, 16) float32, codes (N, 2) uint32) of this resident scene's emitter entries — every EmissiveMat
        sphere, rectangle, Rect3d face, disk and mesh triangle of positive power, where fw_scene_update last put them — in
        fw_selftest_emitters' order: what emitters_rays and emitters_reduce take."""
        n = C.c_uint32()
        _check(self._lib, self._lib.fw_scene_emitters(self.handle, None, None, 0, C.byref(n)))
        rec, codes = np.zeros((n.value, A.FW_EMITTERS_RECORD_FLOATS), np.float32), np.zeros((n.value, 2), np.uint32)
        if n.value:
            _check(self._lib, self._lib.fw_scene_emitters(self.handle, rec.ctypes.data, codes.ctypes.data, n.value, C.byref(n)))
        return rec, codes

    def bake_emitters(self, emitters, positions, normals, ids=None, rounds=1, first_round=0, sums=None, out=None, seed=0, use_bvh=True, stream=None,
                      rays_per_batch=0, flags=0, chunk=None):
        """fw_bake_emitters: the rounds [first_round, first_round + rounds) of an api.EmitterLights at surface points (see _AoPoints:
        numpy arrays, or tensors on this scene's device, read in place) under this scene's own emitter entries (emitters), picked by
        power, `chunk` points at a time (None: the description's own setting; 0: automatic).  sums, out and the return value as
        bake_area's: (out, sums, stats) with (Er, Eg, Eb, vis) per id."""
        a = emitters.to_abi()
        if chunk is not None:
            a.chunk_points = int(chunk)
        pts = _AoPoints(positions, normals, ids, self.device)
        return self._bake_points(self._lib.fw_bake_emitters, a, pts, 4, (pts.n, pts.pos, pts.nrm, pts.stride, pts.ids), rounds, first_round, sums, out,
                                 seed, use_bvh, stream, rays_per_batch, flags)

    def bake_lightmap(self, lightmap, rounds, samples, first_round=0, sums=None, dilate=2, seed=0, use_bvh=True, stream=None, paths_per_batch=0,
                      flags=0, chunk=None, on_device=False):
        """fw_bake_lightmap: the rounds [first_round, first_round + rounds) of an api.Lightmap, `samples` paths per direction and round,
        `chunk` covered texels at a time (None: the lightmap's own setting; 0: automatic).  sums: (H, W, 4) float32 running sums of the
        rounds before first_round, updated in place (None: zeros, only with first_round 0).  Returns (irradiance, sums, stats): host
        arrays, or — sums a device tensor on this scene's device, or on_device=True — device tensors, baked on `stream` (default: the
        current torch stream).  irradiance (H, W, 4): rgb = sums / (first_round + rounds) and a = 1 on covered texels, then `dilate`
        dilation passes (filled texels carry a = 0.5)."""
        s, _keep = _lightmap_abi(lightmap, chunk)
        return self._bake(self._lib.fw_bake_lightmap, s, (int(dilate),), (int(s.height), int(s.width), 4), rounds, samples, first_round, sums, seed,
                          use_bvh, stream, paths_per_batch, flags, on_device)

    def trace(self, rays, use_bvh, seed=0, key_base=0, rays_per_batch=0, time_kernels=False, stats=None):
        """fw_trace_rays: one root.hit(ray, 0.001, 2e9) per ray.  rays: (n, 6) origin + direction.
        - numpy (or anything array-like): returns a structured array of HIT_DTYPE (fw_hit's fields).
        - a contiguous float32 torch tensor on this scene's device: traced in place on the current torch stream; returns an (n, 12)
          float32 tensor on the device (columns: HIT_COLUMNS; hit_fields() gives the int32 views of material / object / prim).
        A ray with a non-finite component or a zero direction comes back as a miss (object == FW_NO_HIT).  Ray i's medium draws are
        keyed (seed, key_base + i).  stats: a dict to fill with fw_stats."""
        p = A.fw_trace_params()
        p.use_bvh = int(bool(use_bvh))
        p.flags = A.FW_FLAG_TIME_KERNELS if time_kernels else 0
        p.seed = int(seed)
        p.key_base = int(key_base)
        p.rays_per_batch = int(rays_per_batch)
        st = A.fw_stats()
        s = _Side(rays, self.device)
        n = s.count(rays, 6)
        r = s.inp(rays, (n, 6), "rays")
        out = s.new_hits(n)
        s.params(p)
        _check(self._lib, self._lib.fw_trace_rays(self.handle, C.byref(p), s.ptr(r), n, s.ptr(out), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def hit_surface(self, rays, hits, out=None, stream=None):
        """fw_hit_surface: the material at the hits `trace` returned for `rays` on this scene, as an (n, 16) float32 array (columns:
        SURFACE_COLUMNS): albedo, kind (the material's, -1 a miss, -2 a ray that was not traced), the normal facing the ray, distance,
        position, 0, the emitted radiance (an emitter's, or the environment's on a miss; not clamped), 0.  numpy rays with a HIT_DTYPE
        array, or device tensors ((n, 6) and (n, 12) float32) on this scene's device, evaluated on `stream` (default: the current torch
        stream) where they lie.  out: a contiguous (n, 16) float32 array or tensor of the rays' kind to fill instead; returned."""
        s = _Side(rays, self.device)
        n = s.count(rays, 6)
        r, h = s.inp(rays, (n, 6), "rays"), s.hits(hits, n)
        out = s.out(out, (n, 16), "out")
        _check(self._lib, self._lib.fw_hit_surface(self.handle, *s.ptrs(r, h), n, s.ptr(out), *s.tail(stream)))
        return out

    def aovs(self, renderer, samples, out=None, stream=None):
        """fw_render_aovs: first-hit guide buffers of the whole frame averaged over `samples` samples (the renderer's own sample count is
        not used), as an (N, 12) float32 array: albedo, coverage, normal, distance, position, 0 (AOV_COLUMNS).  out: a contiguous (N, 12)
        float32 device tensor on this scene's device to fill instead, launched on `stream` (default: the current torch stream); returned.
        stats: see aovs_stats after the call."""
        import copy
        lib = self._lib
        r = copy.copy(renderer); r.settings = dict(renderer.settings); r.settings["samples"] = int(samples)
        p = r.to_params(None)
        n = p.width * p.height
        st = A.fw_stats()
        if out is not None:
            import torch
            _check_device_tensor(out, (n, 12), torch.float32, self.device, "out")
            p.outputs_on_device = 1
            p.stream = _stream_arg(stream, torch.device("cuda", self.device))
            _check(lib, lib.fw_render_aovs(self.handle, C.byref(p), out.data_ptr(), C.byref(st)))
            self.aovs_stats = st.as_dict()
            return out
        aov = np.empty((n, 12), np.float32)
        _check(lib, lib.fw_render_aovs(self.handle, C.byref(p), aov.ctypes.data, C.byref(st)))
        self.aovs_stats = st.as_dict()
        return aov

    def camera_rays(self, renderer, sample=0, pixel_ids=None):
        """fw_camera_rays on this scene's device: see camera_rays()."""
        return camera_rays(renderer, sample, pixel_ids, self.device)

    def close(self):
        if self.handle:
            self._lib.fw_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_scene(scene_desc, renderer, pixel_ids=None, device=0):
    """fw_render_scene: the one-shot `Renderer::render(scene)` shape (conversion + BVH + render)."""
    from .api import RenderResult
    lib = load()
    p = renderer.to_params(pixel_ids)
    n = int(pixel_ids.shape[0]) if pixel_ids is not None else p.width * p.height
    rgb8 = np.empty((n, 3), np.uint8)
    gam = np.empty((n, 3), np.float32)
    lin = np.empty((n, 3), np.float32)
    st = A.fw_stats()
    _check(lib, lib.fw_render_scene(scene_desc.ptr(), C.byref(p), device, rgb8.ctypes.data, gam.ctypes.data,
                                    lin.ctypes.data, C.byref(st)))
    return RenderResult(rgb8, gam, lin, st.as_dict(), p.width, p.height)


def render_scene_tiled(scene_desc, renderer, devices):
    """fw_render_scene_tiled: one process, one host thread per listed device, tiles scattered into host buffers."""
    from .api import RenderResult
    lib = load()
    p = renderer.to_params(None)
    n = p.width * p.height
    rgb8 = np.empty((n, 3), np.uint8)
    gam = np.empty((n, 3), np.float32)
    lin = np.empty((n, 3), np.float32)
    st = A.fw_stats()
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    _check(lib, lib.fw_render_scene_tiled(scene_desc.ptr(), C.byref(p), devs, len(devices), rgb8.ctypes.data, gam.ctypes.data,
                                          lin.ctypes.data, C.byref(st)))
    return RenderResult(rgb8, gam, lin, st.as_dict(), p.width, p.height)


# columns of fw_render_aovs' (N, 12) records
AOV_COLUMNS = dict(albedo=slice(0, 3), coverage=3, normal=slice(4, 7), distance=7, position=slice(8, 11))
# column of each field in the (n, 16) float32 records DeviceScene.hit_surface returns
SURFACE_COLUMNS = dict(albedo=slice(0, 3), kind=3, normal=slice(4, 7), distance=7, position=slice(8, 11), emitted=slice(12, 15))


def denoise(color, aov, moments=None, width=None, height=None, iterations=A.FW_DENOISE_ITERATIONS, gamma=2.2, device=0, stream=None):
    """fw_denoise: the edge-avoiding a-trous filter (include/firework_hip.h) of a linear frame `color` (N, 3) guided by fw_render_aovs'
    records `aov` (N, 12), with fw_render_adaptive's `moments` (N, 4) for the luminance term, or None.  All host arrays (numpy): returns
    (rgb8, gamma, linear) host arrays of shape (N, 3).  All contiguous float32 torch tensors on cuda:`device`: filtered on `stream`
    (default: the current torch stream), returns device tensors.  width * height must be N."""
    lib = load()
    if width is None or height is None:
        raise ValueError("denoise needs width and height")
    n = int(width) * int(height)
    p = A.fw_denoise_params()
    p.width, p.height, p.iterations, p.gamma, p.device = int(width), int(height), int(iterations), float(gamma), int(device)
    s = _Side(color, device)
    c, a, m = s.inp(color, (n, 3), "color"), s.inp(aov, (n, 12), "aov"), s.inp(moments, (n, 4), "moments")
    rgb8, gam, lin = s.new((n, 3), "u8"), s.new((n, 3)), s.new((n, 3))
    s.params(p, stream)
    _check(lib, lib.fw_denoise(C.byref(p), *s.ptrs(c, a, m, lin, gam, rgb8)))
    return rgb8, gam, lin


def temporal(color, aov, moments=None, history=None, prev_position=None, width=None, height=None, camera=None, prev_camera=None, samples=0,
             max_history=float("inf"), device=0, stream=None):
    """fw_temporal: merges the linear frame `color` (N, 3) — with fw_render_adaptive's `moments` (N, 4), or None and the frame's `samples`
    — with the previous frame's `history` = (hist_color (N, 3), hist_moments (N, 4), hist_aov (N, 12)): the previous call's first two
    results and the previous frame's guides, reprojected with `prev_camera` through this frame's guides `aov` (N, 12) and tested
    geometrically (include/firework_hip.h).  history None = a first frame.  prev_position (N, 3): where each pixel's surface point was
    in the previous frame; None = a static scene.  camera / prev_camera: CameraSettings or fw_camera_settings (prev_camera defaults to
    camera).  Returns (out_color (N, 3), out_moments (N, 4), out_history (N,)): host arrays for host arrays; for contiguous float32
    torch tensors on cuda:`device`, merged on `stream` (default: the current torch stream), new device tensors."""
    lib = load()
    if width is None or height is None or camera is None:
        raise ValueError("temporal needs width, height and camera")
    n = int(width) * int(height)
    p = A.fw_temporal_params()
    p.width, p.height, p.samples, p.max_history, p.device = int(width), int(height), int(samples), float(max_history), int(device)
    p.camera = camera if isinstance(camera, A.fw_camera_settings) else camera.to_abi()
    prev_camera = camera if prev_camera is None else prev_camera
    p.prev_camera = prev_camera if isinstance(prev_camera, A.fw_camera_settings) else prev_camera.to_abi()
    hist = (None, None, None) if history is None else tuple(history)
    if len(hist) != 3:
        raise ValueError("history must be (hist_color, hist_moments, hist_aov) or None")
    names = ("color", "moments", "aov", "hist_color", "hist_moments", "hist_aov", "prev_position")
    cols = (3, 4, 12, 3, 4, 12, 3)
    s = _Side(color, device)
    ins = [s.inp(t, (n, c), name) for name, c, t in zip(names, cols, (color, moments, aov) + hist + (prev_position,))]
    out_c, out_m, out_h = s.new((n, 3)), s.new((n, 4)), s.new((n,))
    s.params(p, stream)
    _check(lib, lib.fw_temporal(C.byref(p), *s.ptrs(*ins, out_c, out_m, out_h)))
    return out_c, out_m, out_h
