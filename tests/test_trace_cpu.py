"""CPU-side checks of the ray-query ABI (v8): fw_trace_rays / fw_camera_rays are exported, fw_hit / fw_trace_params have the C
compiler's layout in ctypes and in the numpy dtype DeviceScene.trace returns, and the calls refuse bad arguments and a missing GPU
before they touch anything."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIT_FIELDS = ["t", "point", "normal", "u", "v", "material", "object", "prim"]
PARAM_FIELDS = ["use_bvh", "flags", "seed", "key_base", "rays_per_batch", "on_device", "stream"]


def _c_layout(tmp_path, struct, fields):
    """sizeof and offsetof of `struct`'s fields as the C compiler lays out include/firework_hip.h."""
    src = '#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(fields) + '\\n",sizeof(' + \
          struct + ")" + "".join(f",offsetof({struct},{f})" for f in fields) + ");return 0;}"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    return out[0], out[1:]


def test_trace_entry_points_are_exported_at_abi_8():
    lib = _lib.load()
    assert hasattr(lib, "fw_trace_rays") and hasattr(lib, "fw_camera_rays")
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION


def test_fw_hit_layout_matches_header(tmp_path):
    size, offs = _c_layout(tmp_path, "fw_hit", HIT_FIELDS)
    assert size == 48 == C.sizeof(A.fw_hit)
    assert offs == [getattr(A.fw_hit, f).offset for f in HIT_FIELDS]


def test_fw_trace_params_layout_matches_header(tmp_path):
    size, offs = _c_layout(tmp_path, "fw_trace_params", PARAM_FIELDS)
    assert size == C.sizeof(A.fw_trace_params)
    assert offs == [getattr(A.fw_trace_params, f).offset for f in PARAM_FIELDS]


def test_numpy_hit_dtype_matches_header(tmp_path):
    size, offs = _c_layout(tmp_path, "fw_hit", HIT_FIELDS)
    dt = _lib.HIT_DTYPE
    assert dt.itemsize == size == 48
    assert list(dt.names) == HIT_FIELDS
    assert [dt.fields[f][1] for f in HIT_FIELDS] == offs
    assert dt["point"].shape == (3,) and dt["normal"].shape == (3,)
    assert dt["material"] == np.uint32 and dt["object"] == np.uint32 and dt["prim"] == np.uint32
    # the (n, 12) column map of device records is the same layout
    assert [_lib.HIT_COLUMNS[f] if isinstance(_lib.HIT_COLUMNS[f], int) else _lib.HIT_COLUMNS[f].start for f in HIT_FIELDS] == [o // 4 for o in offs]


def _trace(scene, rays, n, hits):
    lib = _lib.load()
    p = A.fw_trace_params()
    return lib.fw_trace_rays(scene, C.byref(p), rays, n, hits, None)


def test_trace_argument_checks():
    """Checked before the scene is looked at: a NULL scene, NULL rays or hits with n > 0.  n = 0 writes nothing and succeeds."""
    rays = np.zeros((4, 6), np.float32)
    hits = np.zeros(4, _lib.HIT_DTYPE)
    assert _trace(None, rays.ctypes.data, 4, hits.ctypes.data) == A.FW_ERR_BAD_ARG
    lib = _lib.load()
    assert lib.fw_trace_rays(C.c_void_p(1), None, rays.ctypes.data, 4, hits.ctypes.data, None) == A.FW_ERR_BAD_ARG   # NULL params
    not_a_scene = C.create_string_buffer(64)      # never dereferenced: every one of these calls fails or returns first
    assert _trace(C.addressof(not_a_scene), None, 4, hits.ctypes.data) == A.FW_ERR_BAD_ARG
    assert _trace(C.addressof(not_a_scene), rays.ctypes.data, 4, None) == A.FW_ERR_BAD_ARG
    assert _trace(C.addressof(not_a_scene), None, 0, None) == A.FW_OK


def test_camera_rays_argument_checks():
    lib = _lib.load()
    _s, r = scenes.cornell_box()
    p = r.width(8).height(8).to_params()
    out = np.zeros((64, 6), np.float32)
    assert lib.fw_camera_rays(None, 0, 0, out.ctypes.data) == A.FW_ERR_BAD_ARG
    assert lib.fw_camera_rays(C.byref(p), 0, 0, None) == A.FW_ERR_BAD_ARG


def test_camera_rays_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    _s, r = scenes.cornell_box()
    with pytest.raises(_lib.FireworkError) as e:
        _lib.camera_rays(r.width(8).height(8))
    assert e.value.status == A.FW_ERR_NO_DEVICE
    assert not out_written_without_device()


def out_written_without_device():
    """fw_camera_rays leaves the caller's buffer as it was when it fails."""
    lib = _lib.load()
    _s, r = scenes.cornell_box()
    p = r.width(4).height(4).to_params()
    out = np.full((16, 6), 7.0, np.float32)
    assert lib.fw_camera_rays(C.byref(p), 0, 0, out.ctypes.data) == A.FW_ERR_NO_DEVICE
    return bool((out != 7.0).any())
