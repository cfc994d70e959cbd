"""CPU-side checks of the direct light of point, spot and directional lights at surface points (fw_direct_rays, fw_direct_reduce,
fw_bake_direct): the exports and their ctypes signatures against the header, the struct's layout at ABI 8; every argument
error of the three calls in the header's order (they come before HIP is called), and the no-device error with the caller's buffers
untouched; DirectLight's validation; material_direct_table on all six material kinds; the CLI's refusals; and the numpy statements' own
properties against closed forms, tests/delta_lights_ref.py and tests/ggx_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import DirectionalLight, DirectLight, PointLight, SpotLight

import delta_lights_ref as DL
import direct_ref as R
import ggx_ref as GGX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
UP = np.array([[0.0, 1.0, 0.0]], np.float32)
ORIGIN = np.zeros((1, 3), np.float32)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- exports and layout ---------------------------------------------------------------------------------------------------------------
def _ctype_of(param):
    """the ctypes type _abi uses for a C parameter of the header"""
    param = param.strip()
    if "*" in param:
        for name, t in (("fw_direct", A.fw_direct), ("fw_trace_params", A.fw_trace_params), ("fw_stats", A.fw_stats)):
            if re.search(rf"\b{name}\b", param):
                return C.POINTER(t)
        return C.c_void_p
    if param.startswith("uint32_t"):
        return C.c_uint32
    assert param.startswith("int "), param
    return C.c_int


def test_exports_and_signatures_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.DIRECT_PROTOTYPES) == ["fw_bake_direct", "fw_direct_rays", "fw_direct_reduce"]
    for name, argtypes in A.DIRECT_PROTOTYPES.items():
        assert hasattr(lib, name), name
        found = re.findall(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert len(found) == 1, name
        want = [_ctype_of(p) for p in found[0].replace("\n", " ").split(",")]
        assert argtypes == want, (name, argtypes, want)
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == C.c_int


def test_struct_layout(tmp_path):
    """ctypes' fw_direct equals the C compiler's, size and every field offset"""
    names = ["lobe", "face_view", "bias", "chunk_points"]
    assert [f for f, _ in A.fw_direct._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 1) + '\\n",sizeof(fw_direct)' +
           "".join(f",offsetof(fw_direct,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_direct)] + [getattr(A.fw_direct, f).offset for f in names]
    d = DirectLight(0.25, "renderer", False)
    d.chunk_points = 9
    a = d.to_abi()
    assert (a.lobe, a.face_view, a.bias, a.chunk_points) == (1, 0, 0.25, 9)
    a = DirectLight().to_abi()
    assert (a.lobe, a.face_view, a.bias, a.chunk_points) == (0, 1, float(np.float32(1e-3)), 0)


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def _d(lobe=0, face_view=1, bias=1e-3):
    d = A.fw_direct()
    d.lobe, d.face_view, d.bias = lobe, face_view, bias
    return d


BAD_DIRECTS = [("lobe", _d(lobe=2)), ("face_view", _d(face_view=2)), ("bias", _d(bias=-0.5)), ("bias", _d(bias=NAN)), ("bias", _d(bias=INF))]
LIGHTS = [PointLight((0.0, 2.0, 0.0), (1.0, 1.0, 1.0)), SpotLight((0.0, 3.0, 0.0), (0.0, -1.0, 0.0), (2.0, 2.0, 2.0), 10.0, 30.0),
          DirectionalLight((0.0, -1.0, 0.0), (1.0, 1.0, 1.0))]


def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _bad_light(**kw):
    l = LIGHTS[1].to_abi()
    for k, v in kw.items():
        setattr(l, k, v)
    return (A.fw_light * 3)(LIGHTS[0].to_abi(), l, LIGHTS[2].to_abi())


def _order_inside_the_description(lib, call):
    for word, d in BAD_DIRECTS:
        assert _said(lib, call(d, n=0), word) == A.FW_ERR_BAD_ARG, word                                 # the description before n
    assert _said(lib, call(_d(lobe=2, face_view=2, bias=-1.0)), "lobe") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_d(face_view=2, bias=-1.0)), "face_view") == A.FW_ERR_BAD_ARG


def _lights_are_checked_like_fw_check_lights(lib, call):
    """after the description, before n: n_lights == 0, then fw_check_lights' refusals with its messages"""
    assert _said(lib, call(_d(bias=-1.0), n_lights=0), "bias") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n_lights=0, n=0), "n_lights") == A.FW_ERR_BAD_ARG
    for kw, word in ((dict(kind=7), "lights[1]: unknown kind"), (dict(cos_inner=NAN), "lights[1]: a field is not finite"),
                     (dict(intensity=A.vec3((1.0, -1.0, 1.0))), "lights[1]: negative intensity"),
                     (dict(direction=A.vec3((0.0, 0.0, 0.0))), "lights[1]: zero direction"), (dict(cos_inner=0.5, cos_outer=0.6), "lights[1]: spot cosines")):
        arr = _bad_light(**kw)
        assert _said(lib, call(lights=arr, n=0), word) == A.FW_ERR_BAD_ARG, word
        assert lib.fw_check_lights(arr, 3) == A.FW_ERR_BAD_ARG and word in lib.fw_last_error().decode()     # the same message
    assert _said(lib, call(n_lights=A.FW_MAX_LIGHTS + 1, n=0), "FW_MAX_LIGHTS") == A.FW_ERR_BAD_ARG


def _points_checks(lib, call, good):
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, view_stride=2), "stride_floats") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(view_stride=2, view=good["view"]), "view_stride_floats") == A.FW_ERR_BAD_ARG
    assert call(view_stride=2, view=None, spec=None, device=-1) in (A.FW_ERR_NO_DEVICE, A.FW_ERR_BAD_ARG) and "view_stride" not in lib.fw_last_error().decode()
    assert _said(lib, call(view=None, spec=good["spec"]), "spec needs view") == A.FW_ERR_BAD_ARG


def _buffers(n=4, ln=3):
    return dict(pos=np.full((n, 3), 7.0, np.float32), nrm=np.full((n, 3), 7.0, np.float32), view=np.full((n, 3), 7.0, np.float32),
                spec=np.full((n, 4), 7.0, np.float32), rays=np.full((n * ln, 6), 7.0, np.float32), hits=np.zeros(n * ln, _lib.HIT_DTYPE),
                sums=np.full((n, 8), 7.0, np.float32), out=np.full((n, 8), 7.0, np.float32))


def test_direct_rays_argument_checks():
    lib = _lib.load()
    buf = _buffers()
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    arr3, _ = _lib._light_array(LIGHTS)

    def call(d=None, n=4, stride=3, view_stride=3, device=0, on_device=0, null_d=False, ids_p=None, lights=arr3, n_lights=3, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_direct_rays(None if null_d else C.byref(d if d is not None else _d()), lights, n_lights, device, n, a["pos"], a["nrm"], stride,
                                  ids_p, a["view"], view_stride, a["spec"], a["rays"], on_device, None)

    assert _said(lib, call(null_d=True), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_d(lobe=2), lights=None), "null") == A.FW_ERR_BAD_ARG
    for name in ("pos", "nrm", "rays"):
        assert _said(lib, call(_d(lobe=2), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name           # NULL before the description
    _order_inside_the_description(lib, call)
    _lights_are_checked_like_fw_check_lights(lib, call)
    _points_checks(lib, call, good)
    for name in ("pos", "nrm", "view", "rays"):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + 2)}), "aligned") == A.FW_ERR_BAD_ARG, name
    for off in (4, 8):
        assert _said(lib, call(on_device=1, spec=C.c_void_p(good["spec"] + off)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    many = (A.fw_light * 2048)(*([LIGHTS[0].to_abi()] * 2048))
    big = dict(lights=many, n_lights=2048, n=1 << 20)
    assert _said(lib, call(stride=2, **big), "stride") == A.FW_ERR_BAD_ARG                               # bad arguments before the size
    assert _said(lib, call(on_device=1, rays=C.c_void_p(good["rays"] + 2), **big), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(**big), "must be below") == A.FW_ERR_UNSUPPORTED                             # n Ln = 2^31
    assert _said(lib, call(device=-1, **big), "must be below") == A.FW_ERR_UNSUPPORTED                  # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert call(view=None, spec=None) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for k, v in buf.items() if k != "hits")
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_direct_reduce_argument_checks():
    lib = _lib.load()
    buf = _buffers()
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    arr3, _ = _lib._light_array(LIGHTS)

    def call(d=None, n=4, stride=3, view_stride=3, device=0, on_device=0, null_d=False, ids_p=None, lights=arr3, n_lights=3, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_direct_reduce(device, None if null_d else C.byref(d if d is not None else _d()), lights, n_lights, n, a["pos"], a["nrm"], stride,
                                    ids_p, a["view"], view_stride, a["spec"], a["rays"], a["hits"], a["sums"], on_device, None)

    assert _said(lib, call(null_d=True), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_d(lobe=2), lights=None), "null") == A.FW_ERR_BAD_ARG
    for name in ("pos", "nrm", "rays", "hits", "sums"):
        assert _said(lib, call(_d(lobe=2), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    _order_inside_the_description(lib, call)
    _lights_are_checked_like_fw_check_lights(lib, call)
    _points_checks(lib, call, good)
    for name, off in (("sums", 4), ("sums", 8), ("hits", 4), ("hits", 8), ("spec", 4), ("spec", 8), ("rays", 2), ("pos", 2), ("nrm", 2), ("view", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    many = (A.fw_light * 2048)(*([LIGHTS[0].to_abi()] * 2048))
    big = dict(lights=many, n_lights=2048, n=1 << 20)
    assert _said(lib, call(on_device=1, sums=C.c_void_p(good["sums"] + 4), **big), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(**big), "must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(device=-1, **big), "must be below") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for k, v in buf.items() if k != "hits")
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_bake_direct_argument_checks():
    """every refusal comes before the scene is looked at, so a scene handle that is never dereferenced will do; without a device the
    call ends there, before the scene's light count is read"""
    lib = _lib.load()
    buf = _buffers()
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call

    def call(d=None, n=4, stride=3, view_stride=3, first=0, rounds=1, on_device=0, null=None, ids_p=None, **ptrs):
        a = dict(good, **ptrs)
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, d=C.byref(d if d is not None else _d()), tp=C.byref(tp))
        if null:
            args[null] = None
        return lib.fw_bake_direct(args["scene"], args["d"], args["tp"], n, a["pos"], a["nrm"], stride, ids_p, a["view"], view_stride, a["spec"], first,
                                  rounds, a["sums"], a["out"], None)

    for null in ("scene", "d", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("pos", "nrm"):
        assert _said(lib, call(_d(lobe=2), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    _order_inside_the_description(lib, call)
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, view_stride=2), "stride_floats") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(view_stride=2, rounds=0), "view_stride_floats") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(view=None, rounds=0), "spec needs view") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(rounds=0, first=0xFFFFFFFF), "rounds must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1, sums=None), "overflows") == A.FW_ERR_BAD_ARG
    assert call(first=0xFFFFFFFE, rounds=1, on_device=1, sums=C.c_void_p(good["sums"] + 4)) == A.FW_ERR_BAD_ARG and "aligned" in lib.fw_last_error().decode()
    assert _said(lib, call(first=2, sums=None, on_device=1, out=C.c_void_p(good["out"] + 4)), "first_round > 0") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("out", 4), ("out", 8), ("spec", 4), ("spec", 8), ("pos", 2), ("nrm", 2), ("view", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(sums=None, out=None) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert call(view=None, spec=None) == A.FW_ERR_NO_DEVICE and call(n=1 << 31) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for k, v in buf.items() if k != "hits")


def test_python_entry_points_check_and_fail_loudly():
    pos, nrm = R.points(6, np.random.default_rng(0), unusable=False)
    d = DirectLight()
    with pytest.raises(ValueError, match="id"):
        _lib.direct_rays(d, LIGHTS, pos, nrm, ids=np.array([0, 6], np.uint32))            # an id past the points is refused in Python
    with pytest.raises(ValueError, match="shape"):
        _lib.direct_rays(d, LIGHTS, pos, nrm[:5])
    with pytest.raises(ValueError, match="spec needs view"):
        _lib.direct_rays(d, LIGHTS, pos, nrm, spec=np.zeros((6, 4), np.float32))
    with pytest.raises(ValueError, match="spec needs view"):
        api.direct_rays(d, LIGHTS, pos, nrm, spec=np.zeros((6, 4), np.float32))
    with pytest.raises(ValueError, match="view"):
        _lib.direct_rays(d, LIGHTS, pos, nrm, view=np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match="sums"):
        _lib.direct_reduce(d, LIGHTS, pos, nrm, np.zeros((18, 6), np.float32), np.zeros(18, _lib.HIT_DTYPE), np.zeros((6, 4), np.float32))
    for bad, word in ((DirectLight(lobe="phong"), "lobe"), (DirectLight(face_view=2), "face_view"), (DirectLight(-1.0), "bias"),
                      (DirectLight(NAN), "bias"), (DirectLight(INF), "bias")):
        with pytest.raises(ValueError, match=word):
            bad.check()
        with pytest.raises(ValueError, match=word):
            bad.to_abi()
    assert DirectLight(0.0, "renderer", False).check().bias == 0.0
    if _lib.device_count() == 0:
        with pytest.raises(_lib.FireworkError) as e:
            _lib.direct_rays(d, LIGHTS, pos, nrm)
        assert e.value.status == A.FW_ERR_NO_DEVICE
        with pytest.raises(_lib.FireworkError) as e:
            _lib.direct_reduce(d, LIGHTS, pos, nrm, np.zeros((18, 6), np.float32), np.zeros(18, _lib.HIT_DTYPE), np.zeros((6, 8), np.float32))
        assert e.value.status == A.FW_ERR_NO_DEVICE


def test_material_direct_table_on_all_six_kinds():
    from firework_amd.api import (ColorEnv, ConstantTexture, DielectricMat, EmissiveMat, GgxMat, IsotropicMat, LambertianMat, MetalMat, RenderObject, Scene, Sphere)
    scene = Scene.new()
    mats = [LambertianMat.with_color((0.6, 0.5, 0.4)), MetalMat.new((0.9, 0.8, 0.7), 0.2), DielectricMat.new(1.5),
            EmissiveMat.with_color((3.0, 3.0, 3.0)), IsotropicMat.new(ConstantTexture((0.2, 0.3, 0.4))), GgxMat.new((0.95, 0.64, 0.54), 0.3)]
    for k, m in enumerate(mats):
        scene.add_object(RenderObject.new(Sphere.new(0.5, scene.add_material(m))).position(2.0 * k, 0.0, 0.0))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    desc = scene.to_desc()
    assert [desc.materials[i].kind for i in range(6)] == [A.FW_MAT_LAMBERTIAN, A.FW_MAT_METAL, A.FW_MAT_DIELECTRIC, A.FW_MAT_EMISSIVE,
                                                           A.FW_MAT_ISOTROPIC, A.FW_MAT_GGX]
    table = api.material_direct_table(desc)
    assert table.dtype == np.float32 and table.shape == (7, 4)
    want = np.array([[0, 0, 0, 0], [0, 0, 0, -1], [0, 0, 0, -1], [0, 0, 0, -1], [0, 0, 0, 0], [0.95, 0.64, 0.54, 0.3], [0, 0, 0, -1]], np.float32)
    assert np.array_equal(table, want)


# ---- the CLI's refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--direct-light"], "-o FILE.png"), (["--direct-light", "-o", "x.png", "--aov-samples", "0"], "--aov-samples"),
    (["--direct-light", "-o", "x.png", "--direct-bias", "-1"], "B >= 0"), (["--direct-light", "-o", "x.png", "--direct-bias", "nan"], "B >= 0"),
    (["--direct-light", "-o", "x.png", "--direct-bias", "inf"], "B >= 0"),
    (["--direct-light", "-o", "x.png", "--denoise"], "cannot be combined"), (["--direct-light", "-o", "x.png", "--orbit", "2"], "cannot be combined"),
    (["--direct-light", "-o", "x.png", "--adaptive", "0.1"], "cannot be combined"), (["--direct-light", "-o", "x.png", "--camera", "panorama"], "cannot be combined"),
    (["--direct-light", "-o", "x.png", "--ao", "2"], "cannot be combined"), (["--direct-light", "-o", "x.png", "--bake-lightmap", "0,4,4"], "cannot be combined"),
    (["--direct-light", "-o", "x.png", "--bake-probes", "1,1,1"], "cannot be combined"), (["--direct-light", "-o", "x.png", "--progressive", "2"], "cannot be combined"),
    (["--direct-bias", "0.01", "-o", "x.png"], "needs --direct-light or --lightmap-direct"), (["--lightmap-direct", "-o", "x.npz"], "needs --bake-lightmap"),
    (["--bake-lightmap", "0,4,4", "--lightmap-direct", "--direct-bias", "-2", "-o", "x.npz"], "B >= 0")])
def test_cli_refusals_come_before_the_device(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args


# ---- the numpy statements -------------------------------------------------------------------------------------------------------------
def _reduce_all_visible(d, lights, pos, nrm, view=None, spec=None, ids=None):
    rays = api.direct_rays(d, lights, pos, nrm, ids, view, spec)
    m = rays.shape[0]
    return rays, api.direct_reduce(d, lights, pos, nrm, rays, np.zeros(m, np.float32), np.full(m, R.MISS), ids, view, spec)


@pytest.mark.parametrize("h", [0.5, 2.0, 3.0, 1e3])
def test_a_point_light_overhead_gives_I_over_h_squared(h):
    """normal up, light straight above at a height that float32 holds exactly: d = (0, h, 0), w = (0, 1, 0), c = 1, E = I / h^2 with no
    rounding but the division's"""
    I = np.array([9.0, 6.0, 3.0])
    for lobe, g in (("cosine", 1.0), ("renderer", 2.0)):
        rays, acc = _reduce_all_visible(DirectLight(0.0, lobe), [PointLight((0.0, h, 0.0), I)], ORIGIN, UP)
        assert np.array_equal(rays, np.array([[0, 0, 0, 0, h, 0]], np.float32))
        assert np.array_equal(acc[0, 0:3], (I / (h * h)) * g) and acc[0, 3] == 1.0 and np.all(acc[0, 4:] == 0.0)
    # with a bias the origin moves up and the light comes nearer: E = I / (h - b)^2 to float64 rounding of the stored float32 ray
    b = 0.25
    rays, acc = _reduce_all_visible(DirectLight(b), [PointLight((0.0, h, 0.0), I)], ORIGIN, UP)
    assert np.array_equal(rays, np.array([[0, b, 0, 0, np.float32(h - b), 0]], np.float32))
    assert np.all(np.abs(acc[0, 0:3] - I / float(np.float32(h - b)) ** 2) <= 4 * R.U * acc[0, 0:3])


def test_zero_rays_are_exactly_where_the_rules_put_them():
    d = DirectLight(0.0)
    # the light in the tangent plane, axis-aligned: c = 0 exactly; below it: c < 0; a directional light travelling along the surface
    for light in (PointLight((3.0, 0.0, 0.0), (1, 1, 1)), PointLight((0.0, 0.0, -2.0), (1, 1, 1)), PointLight((1.0, -1.0, 0.0), (1, 1, 1)),
                  DirectionalLight((1.0, 0.0, 0.0), (1, 1, 1)), DirectionalLight((0.0, 1.0, 0.0), (1, 1, 1))):
        rays, t = api.direct_rays(d, [light], ORIGIN, UP, terms=True)
        assert t["c"][0, 0] <= 0.0 and np.all(rays == 0.0), light
    # a spot outside its outer cone, on its edge (s = 0 at t = 0) and inside; a hard-edged one either side
    spot = lambda deg, inner, outer: SpotLight((0.0, 2.0, 0.0), (np.sin(np.radians(deg)), -np.cos(np.radians(deg)), 0.0), (4, 4, 4), inner, outer)    # noqa: E731
    for deg, inner, outer, lit in ((50.0, 10.0, 40.0, False), (39.0, 10.0, 40.0, True), (0.0, 10.0, 40.0, True), (31.0, 30.0, 30.0, False),
                                   (29.0, 30.0, 30.0, True)):
        rays = api.direct_rays(d, [spot(deg, inner, outer)], ORIGIN, UP)
        assert bool(np.any(rays != 0.0)) == lit, (deg, inner, outer)
    # the light at the point itself, a dark light, an unusable point, a point that takes no light sample
    assert np.all(api.direct_rays(d, [PointLight((0, 0, 0), (1, 1, 1))], ORIGIN, UP) == 0.0)
    assert np.all(api.direct_rays(d, [PointLight((0, 2, 0), (0, 0, 0))], ORIGIN, UP) == 0.0)
    assert np.all(api.direct_rays(d, [PointLight((0, 2, 0), (0, 1e-30, 0))], ORIGIN, UP)[0, 3:] == (0, 2, 0))
    pos, nrm = R.points(20, np.random.default_rng(3))
    top = [PointLight((0.0, 50.0, 0.0), (1, 1, 1)), DirectionalLight((0.0, -1.0, 0.0), (1, 1, 1))]
    rays = api.direct_rays(d, top, pos, nrm).reshape(20, 2, 6)
    ok = api.ao_usable(pos, nrm)
    assert ok.sum() == 17 and np.all(rays[~ok] == 0.0)
    up = ok & (nrm[:, 1] > 0)
    assert up.sum() >= 10 and np.all(np.any(rays[up] != 0.0, axis=-1))
    view = np.tile(np.float32([0.0, -1.0, 0.0]), (20, 1))
    spec = np.zeros((20, 4), np.float32)
    spec[::2, 3] = -1.0
    rays = api.direct_rays(d, top, pos, nrm, None, view, spec).reshape(20, 2, 6)
    assert np.all(rays[::2] == 0.0) and np.all(np.any(rays[1::2][ok[1::2]] != 0.0, axis=-1))     # (face_view: every usable normal now faces up)
    # bias 0: the origin has the position's bits
    sel = np.any(rays != 0.0, axis=-1)
    assert np.array_equal(_u32(rays[sel][:, 0:3]), _u32(np.repeat(pos[:, None, :], 2, axis=1)[sel]))
    # all-zero rays, whatever the hits say, reduce to nothing; an unusable point resolves to zeros
    acc = api.direct_reduce(d, top, pos, nrm, np.zeros((40, 6), np.float32), np.ones(40, np.float32), np.zeros(40, np.uint32))
    assert np.all(acc == 0.0) and np.all(api.direct_resolve(np.zeros((20, 8), np.float32), 3) == 0.0)


def test_lobe_renderer_is_pi_times_the_renderers_light_sample():
    """at a Lambertian vertex with unit albedo §9l's light sample adds scatter_pdf x L = (2 c^3 / pi) L: delta_lights_ref.contribution"""
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3.0, 3.0, size=(40, 3)).astype(np.float32)
    pts[:, 1] = 0.0
    nrm = np.tile(UP, (40, 1))
    lights = [PointLight((0.3, 2.0, -0.2), (9.0, 6.0, 3.0)), SpotLight((0.0, 3.0, 0.0), (0.2, -1.0, 0.1), (30.0, 20.0, 10.0), 10.0, 50.0),
              DirectionalLight((0.3, -1.0, 0.2), (2.0, 1.5, 1.0))]
    for light in lights:
        _rays, acc = _reduce_all_visible(DirectLight(0.0, "renderer"), [light], pts, nrm)
        want = np.array([np.pi * DL.contribution(light, p.astype(np.float64), (0.0, 1.0, 0.0), (1.0, 1.0, 1.0)) for p in pts])
        # the two differ by the float32 rounding of the stored direction (2^-24 relative per component, entering L ~ 1 / d^2 twice and
        # c^3 three times: 5 x 2^-24 sqrt(3) < 2^-20) and by float64 roundings
        assert np.all(np.abs(acc[:, 0:3] - want) <= 2.0 ** -20 * want + 1e-300), light
        assert np.all((acc[:, 3] == 1.0) == (want[:, 0] > 0))
    # the cosine lobe is the irradiance: L c
    _rays, acc = _reduce_all_visible(DirectLight(0.0), [lights[2]], pts, nrm)
    w, L, _ = DL.incident(lights[2], (0, 0, 0))
    assert np.all(np.abs(acc[:, 0:3] - L * w[1]) <= 2.0 ** -23 * L)          # (the record's direction is unit to its float32 rounding; w is unit)


@pytest.mark.parametrize("rho", [0.03, 0.3, 1.0])
def test_the_glossy_term_is_ggx_ref_times_the_incident_light(rho):
    rng = np.random.default_rng(11)
    n = 60
    pts = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(np.float32)
    pts[:, 1] = 0.0
    nrm = rng.normal(size=(n, 3)) * 0.2
    nrm[:, 1] += 1.0
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    eye = np.array([0.5, 2.5, 4.0])
    view = (pts.astype(np.float64) - eye).astype(np.float32)
    f0 = np.array([0.95, 0.64, 0.54], np.float32)
    spec = np.tile(np.concatenate([f0, np.float32([rho])]), (n, 1)).astype(np.float32)
    nh = nrm.astype(np.float64) / np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True)
    for light in (PointLight((0.3, 2.0, -3.0), (9.0, 6.0, 3.0)), SpotLight((0.0, 3.0, -2.0), (0.1, -1.0, 0.5), (30.0, 20.0, 10.0), 20.0, 60.0),
                  DirectionalLight((0.3, -1.0, 0.8), (2.0, 1.5, 1.0))):
        rays, acc = _reduce_all_visible(DirectLight(0.0), [light], pts, nrm, view, spec)
        assert np.all(acc[:, 0:3] == 0.0)                                                    # a conductor has no diffuse term
        seen = 0
        for q in range(n):
            if not np.any(rays[q] != 0.0):
                assert acc[q, 3] == 0.0 and np.all(acc[q, 4:] == 0.0)
                continue
            w, L, _ = DL.incident(light, pts[q].astype(np.float64))
            fcos = GGX.evaluate(nh[q], view[q].astype(np.float64), rho, f0.astype(np.float64), w)[0]
            want = fcos * L
            # the stored direction's float32 rounding moves w by 2^-24 sqrt(3): D changes by up to 4 / alpha of that relative (the
            # lobe's width), Smith's tangent tan^2 = (1 - c^2) / c^2 by 2 / c^2, L and the rest by a few times; float64 roundings are
            # far below
            c = float(nh[q] @ w) if nh[q] @ (-view[q].astype(np.float64)) > 0 else -float(nh[q] @ w)
            tol = (8.0 + 8.0 / float(np.float32(rho) ** 2) + 4.0 / (c * c)) * 2.0 ** -24
            assert np.all(np.abs(acc[q, 4:7] - want) <= tol * want + 1e-300), (q, acc[q, 4:7], want)
            seen += 1
        assert seen >= 30


def test_face_view_flips_exactly_the_back_facing_points():
    rng = np.random.default_rng(2)
    n = 50
    pos = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    view = rng.normal(size=(n, 3)).astype(np.float32)
    back = np.sum(nrm.astype(np.float64) * view.astype(np.float64), axis=1) > 0
    assert 10 <= back.sum() <= 40
    sun = [DirectionalLight((0.2, -1.0, 0.1), (1, 1, 1))]
    plain = api.direct_rays(DirectLight(0.0, face_view=False), sun, pos, nrm, None, view)
    none = api.direct_rays(DirectLight(0.0), sun, pos, nrm)
    faced = api.direct_rays(DirectLight(0.0), sun, pos, nrm, None, view)
    flipped = api.direct_rays(DirectLight(0.0, face_view=False), sun, pos, np.where(back[:, None], -nrm, nrm), None, view)
    assert np.array_equal(_u32(plain), _u32(none))                                           # without face_view the view changes nothing
    assert np.array_equal(_u32(faced), _u32(flipped))
    lit_plain, lit_faced = np.any(plain != 0, axis=1), np.any(faced != 0, axis=1)
    assert np.array_equal(lit_plain[~back], lit_faced[~back]) and np.all(lit_plain[back] != lit_faced[back])
    # with a bias the origin moves to the lit side
    biased = api.direct_rays(DirectLight(0.5), sun, pos, nrm, None, view)
    side = np.sum((biased[:, 0:3].astype(np.float64) - pos) * view, axis=1)
    assert np.all(side[lit_faced] < 0)                                                       # towards the eye


def test_N_counts_the_visible_entries_and_the_visibility_rule():
    lights = [PointLight((0.0, 2.0, 0.0), (1, 1, 1)), SpotLight((0.5, 3.0, 0.0), (0.0, -1.0, 0.0), (2, 2, 2), 20.0, 40.0),
              DirectionalLight((0.0, -1.0, 0.0), (1, 1, 1)), PointLight((1.0, 1.0, 1.0), (3, 3, 3))] * 20
    d = DirectLight(0.0)
    pos = np.zeros((3, 3), np.float32)
    nrm = np.tile(UP, (3, 1))
    rays = api.direct_rays(d, lights, pos, nrm)
    assert np.all(np.any(rays != 0.0, axis=1))
    Ln = len(lights)
    kind = np.tile(np.arange(Ln) % 4, 3)
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    for t, sees_near, sees_far in ((0.5, False, False), (below, False, False), (1.0, True, False), (7.0, True, False)):
        acc = api.direct_reduce(d, lights, pos, nrm, rays, np.full(3 * Ln, t, np.float32), np.zeros(3 * Ln, np.uint32))
        assert np.all(acc[:, 3] == (60 if sees_near else 0) + (20 if sees_far else 0)), t
        assert np.all((acc[:, 0] > 0) == sees_near)
    acc, T, vis = api.direct_reduce(d, lights, pos, nrm, rays, np.full(3 * Ln, 0.25, np.float32), np.full(3 * Ln, R.MISS), terms=True)
    assert np.all(acc[:, 3] == Ln) and np.all(vis)
    # a mixture: N is the number of entries the rule lets through, and E the sum over exactly those
    rng = np.random.default_rng(4)
    hits = R.hand_hits(3 * Ln, kind, rng)
    acc, T, vis = api.direct_reduce(d, lights, pos, nrm, rays, hits["t"], hits["object"], terms=True)
    want = (hits["object"] == A.FW_NO_HIT) | ((kind != 2) & (hits["t"] >= np.float32(1.0)))
    assert np.array_equal(vis.reshape(-1), want) and np.array_equal(acc[:, 3], want.reshape(3, Ln).sum(axis=1))
    each = np.array([api.direct_reduce(d, [lights[i]], pos[:1], nrm[:1], rays[i:i + 1], np.zeros(1, np.float32), np.full(1, R.MISS))[0, 0] for i in range(Ln)])
    assert np.all(np.abs(acc[0, 0] - each[want[:Ln]].sum()) <= Ln * R.U * T[0, 0])
    # the sums resolve by the number of rounds, the eighth float 0
    sums = np.arange(16, dtype=np.float32).reshape(2, 8)
    out = api.direct_resolve(sums, 3)
    assert out.dtype == np.float32 and np.array_equal(out[:, :7], (sums[:, :7].astype(np.float64) / 3.0).astype(np.float32)) and np.all(out[:, 7] == 0.0)
