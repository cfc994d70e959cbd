"""CPU-side checks of ambient occlusion (fw_ao_rays, fw_ao_reduce, fw_bake_ao): the exports and the struct's layout at
ABI 8; every argument error of the three calls in the header's order (they come before HIP is called), and the no-device error with the
caller's buffers untouched; the CLI's refusals; the numpy statements — api.ao_rays on a lightmap's records against Lightmap.rays bit
for bit, unit rays in the normal's hemisphere, unusable points; known answers through api.ao_reduce and api.ao_resolve; and the occluder
in closed form."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import AmbientOcclusion

import ao_ref as R
import lightmap_ref as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
MISS = R.MISS


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.AO_PROTOTYPES) == ["fw_ao_rays", "fw_ao_reduce", "fw_bake_ao"]
    for name in A.AO_PROTOTYPES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name


def test_struct_layout(tmp_path):
    """ctypes' fw_ao equals the C compiler's, size and every field offset"""
    names = ["directions", "falloff", "radius", "bias", "jitter", "chunk_points", "seed"]
    assert [f for f, _ in A.fw_ao._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 1) + '\\n",sizeof(fw_ao)' +
           "".join(f",offsetof(fw_ao,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_ao)] + [getattr(A.fw_ao, f).offset for f in names]
    a = AmbientOcclusion(2.5, 33, 1, 0.25).seed(7).jitter(False).to_abi()
    assert (a.directions, a.falloff, a.radius, a.bias, a.jitter, a.chunk_points, a.seed) == (33, 1, 2.5, 0.25, 0, 0, 7)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _ao(directions=5, falloff=0, radius=2.0, bias=1e-3):
    a = A.fw_ao()
    a.directions, a.falloff, a.radius, a.bias, a.jitter = directions, falloff, radius, bias, 1
    return a


# (the word the detail string must hold, the description), in the header's order
BAD_AOS = [("directions", _ao(directions=0)), ("directions", _ao(directions=(1 << 20) + 1)), ("falloff", _ao(falloff=2)),
           ("radius must", _ao(radius=0.0)), ("radius must", _ao(radius=-1.0)), ("radius must", _ao(radius=NAN)), ("radius must", _ao(radius=-INF)),
           ("infinite radius", _ao(radius=INF, falloff=1)), ("bias", _ao(bias=-0.5)), ("bias", _ao(bias=NAN)), ("bias", _ao(bias=INF))]


def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _order_inside_the_description(lib, call):
    for word, ao in BAD_AOS:
        assert _said(lib, call(ao, n=0), word) == A.FW_ERR_BAD_ARG, word                                # the description before n
    assert _said(lib, call(_ao(directions=0, falloff=2, radius=NAN, bias=-1.0)), "directions") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_ao(falloff=2, radius=NAN, bias=-1.0)), "falloff") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_ao(radius=NAN, bias=-1.0)), "radius must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_ao(radius=INF, falloff=1, bias=-1.0)), "infinite radius") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_ao(radius=INF), n=0), "n must") == A.FW_ERR_BAD_ARG                        # infinite with falloff 0 is allowed


def test_ao_rays_argument_checks():
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, np.float32), nrm=np.full((4, 3), 7.0, np.float32), rays=np.full((4 * 5, 6), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(ao=None, n=4, stride=3, device=0, on_device=0, null_ao=False, ids_p=None, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_ao_rays(None if null_ao else C.byref(ao if ao is not None else _ao()), device, 0, n, a["pos"], a["nrm"], stride, ids_p, a["rays"],
                              on_device, None)

    assert _said(lib, call(null_ao=True), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(_ao(directions=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name   # NULL before the description
    _order_inside_the_description(lib, call)
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, device=-1), "stride") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + 2)}), "aligned") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    big = _ao(directions=1 << 20)
    assert _said(lib, call(big, n=1 << 11, stride=2), "stride") == A.FW_ERR_BAD_ARG                     # bad arguments before the size
    assert _said(lib, call(big, n=1 << 11, on_device=1, rays=C.c_void_p(good["rays"] + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(big, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED          # n D = 2^31
    assert _said(lib, call(big, n=1 << 11, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_ao_reduce_argument_checks():
    lib = _lib.load()
    rays = np.zeros((4 * 5, 6), np.float32)
    rays[:, 4] = 1.0
    hits = np.zeros(4 * 5, _lib.HIT_DTYPE)
    sums = np.full((4, 4), 7.0, np.float32)
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = dict(rays=rays.ctypes.data, hits=hits.ctypes.data, sums=sums.ctypes.data)

    def call(ao=None, n=4, device=0, on_device=0, null_ao=False, ids_p=None, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_ao_reduce(device, None if null_ao else C.byref(ao if ao is not None else _ao()), n, ids_p, a["rays"], a["hits"], a["sums"],
                                on_device, None)

    assert _said(lib, call(null_ao=True), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(_ao(directions=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    _order_inside_the_description(lib, call)
    assert _said(lib, call(n=0, device=-1), "n must") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("hits", 4), ("hits", 8), ("rays", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    big = _ao(directions=1 << 20)
    assert _said(lib, call(big, n=1 << 11, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(big, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(big, n=1 << 11, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0)
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_bake_ao_argument_checks():
    """every refusal comes before the scene is looked at, so a scene handle that is never dereferenced will do"""
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, np.float32), nrm=np.full((4, 3), 7.0, np.float32), sums=np.full((4, 4), 7.0, np.float32),
               out=np.full((4, 4), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call

    def call(ao=None, n=4, stride=3, first=0, rounds=1, on_device=0, null=None, ids_p=None, **ptrs):
        a = dict(good, **ptrs)
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, ao=C.byref(ao if ao is not None else _ao()), tp=C.byref(tp))
        if null:
            args[null] = None
        return lib.fw_bake_ao(args["scene"], args["ao"], args["tp"], n, a["pos"], a["nrm"], stride, ids_p, first, rounds, a["sums"], a["out"], None)

    for null in ("scene", "ao", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("pos", "nrm"):
        assert _said(lib, call(_ao(directions=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    _order_inside_the_description(lib, call)
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, rounds=0), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(rounds=0, first=0xFFFFFFFF), "rounds must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1, sums=None), "overflows") == A.FW_ERR_BAD_ARG
    assert call(first=0xFFFFFFFE, rounds=1, on_device=1, sums=C.c_void_p(good["sums"] + 4)) == A.FW_ERR_BAD_ARG and "aligned" in lib.fw_last_error().decode()
    assert _said(lib, call(first=2, sums=None, on_device=1, out=C.c_void_p(good["out"] + 4)), "first_round > 0") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("out", 4), ("out", 8), ("pos", 2), ("nrm", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    big = _ao(directions=1 << 20)
    assert _said(lib, call(big, n=1 << 11, rounds=0), "rounds must") == A.FW_ERR_BAD_ARG                 # bad arguments before the size
    assert _said(lib, call(big, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(sums=None, out=None) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())


def test_python_entry_points_check_and_fail_loudly():
    pos, nrm = R.points(6, np.random.default_rng(0), unusable=False)
    ao = AmbientOcclusion(1.0, 4)
    with pytest.raises(ValueError, match="id"):
        _lib.ao_rays(ao, pos, nrm, ids=np.array([0, 6], np.uint32))                      # an id past the points is refused in Python
    with pytest.raises(ValueError, match="shape"):
        _lib.ao_rays(ao, pos, nrm[:5])
    for bad, word in ((AmbientOcclusion(0.0), "radius"), (AmbientOcclusion(1.0, 0), "directions"), (AmbientOcclusion(1.0, 4, 2), "falloff"),
                      (AmbientOcclusion(INF, 4, 1), "infinite"), (AmbientOcclusion(1.0, 4, 0, -1.0), "bias")):
        with pytest.raises(ValueError, match=word):
            bad.check()
    assert AmbientOcclusion(INF, 4).check().radius == INF
    if _lib.device_count() == 0:
        with pytest.raises(_lib.FireworkError) as e:
            _lib.ao_rays(ao, pos, nrm)
        assert e.value.status == A.FW_ERR_NO_DEVICE
        with pytest.raises(_lib.FireworkError) as e:
            _lib.ao_reduce(ao, np.zeros((8, 6), np.float32), np.zeros(8, _lib.HIT_DTYPE), np.zeros((2, 4), np.float32))
        assert e.value.status == A.FW_ERR_NO_DEVICE


# ---- the CLI's refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--ao", "0", "-o", "x.png"], "RADIUS > 0"), (["--ao", "nan", "-o", "x.png"], "RADIUS > 0"), (["--ao", "inf", "-o", "x.png"], "RADIUS > 0"),
    (["--ao", "2"], "-o FILE.png"), (["--ao", "2", "-o", "x.png", "--ao-dirs", "0"], "--ao-dirs"),
    (["--ao", "2", "-o", "x.png", "--ao-dirs", str((1 << 20) + 1)], "--ao-dirs"), (["--ao", "2", "-o", "x.png", "--ao-rounds", "0"], "--ao-rounds"),
    (["--ao", "2", "-o", "x.png", "--aov-samples", "0"], "--aov-samples"),
    (["--ao", "2", "-o", "x.png", "--denoise"], "cannot be combined"), (["--ao", "2", "-o", "x.png", "--orbit", "2"], "cannot be combined"),
    (["--ao", "2", "-o", "x.png", "--adaptive", "0.1"], "cannot be combined"), (["--ao", "2", "-o", "x.png", "--camera", "panorama"], "cannot be combined"),
    (["--ao", "2", "-o", "x.png", "--probe-lit", "p.npz"], "cannot be combined"), (["--ao", "2", "-o", "x.png", "--bake-lightmap", "0,4,4"], "cannot be combined"),
    (["--ao", "2", "-o", "x.png", "--bake-probes", "1,1,1"], "cannot be combined"), (["--ao", "2", "-o", "x.png", "--progressive", "2"], "cannot be combined"),
    (["--ao-dirs", "8", "-o", "x.png"], "need --ao"), (["--ao-rounds", "2", "-o", "x.png"], "need --ao"), (["--ao-falloff", "-o", "x.png"], "--ao-falloff needs"),
    (["--lightmap-ao", "2", "-o", "x.npz"], "needs --bake-lightmap"), (["--bake-lightmap", "0,4,4", "--lightmap-ao", "0", "-o", "x.npz"], "RADIUS > 0"),
    (["--bake-lightmap", "0,4,4", "--lightmap-ao", "inf", "-o", "x.npz"], "RADIUS > 0")])
def test_cli_refusals_come_before_the_device(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args


# ---- the numpy statements -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout, placement", [("quad", "rotated"), ("overlap", "flip")])
def test_rays_on_a_lightmaps_records_are_the_lightmaps_rays(layout, placement):
    for D, bias, jitter, rnd in ((7, 1e-3, True, 0), (65, 0.0, True, 5), (16, 0.25, False, 2)):
        lm = LM.lightmap(layout, 9, 7, True, placement, D).seed(77).jitter(jitter).bias(bias)
        rec, _own = lm.texels()
        ao = AmbientOcclusion(1.0, D, 0, bias).seed(77).jitter(jitter)
        got = api.ao_rays(ao, rec[:, 0:3], rec[:, 4:7], lm.covered(), rnd)
        assert got.dtype == np.float32 and np.array_equal(_u32(got), _u32(lm.rays(rnd))), (layout, D)
        # a permuted list permutes the rays: a point's rays depend on its id alone
        perm = np.random.default_rng(D).permutation(lm.covered().size)
        shuffled = api.ao_rays(ao, rec[:, 0:3], rec[:, 4:7], lm.covered()[perm], rnd)
        assert np.array_equal(_u32(shuffled.reshape(-1, D, 6)), _u32(got.reshape(-1, D, 6)[perm]))


@pytest.mark.parametrize("D", [1, 3, 64, 200])
def test_rays_are_unit_in_the_hemisphere_and_unusable_points_get_none(D):
    rng = np.random.default_rng(D)
    pos, nrm = R.points(20, rng)
    ok = api.ao_usable(pos, nrm)
    assert ok.sum() == 17 and not ok[4] and not ok[9] and not ok[14]
    for bias in (0.0, 0.125):
        ao = AmbientOcclusion(1.0, D, 0, bias).seed(3)
        rays = api.ao_rays(ao, pos, nrm, None, 1).reshape(20, D, 6)
        assert np.all(rays[~ok] == 0.0)
        d = rays[ok][..., 3:].astype(np.float64)
        n64 = nrm[ok].astype(np.float64)
        nh = n64 / np.linalg.norm(n64, axis=1, keepdims=True)
        # unit to one float32 rounding per component (sqrt(3) 2^-24 in length) and the frame's float64 arithmetic
        assert np.all(np.abs(np.linalg.norm(d, axis=-1) - 1.0) <= 2.0 * 2.0 ** -24)
        xi = api.texel_jitter(3, 1, np.nonzero(ok)[0])
        c = np.sqrt(np.maximum(0.0, 1.0 - (np.arange(D)[None, :] + xi[:, 0:1]) / D))
        dot = (d * nh[:, None, :]).sum(axis=-1)
        assert np.all(np.abs(dot - c) <= 4.0 * 2.0 ** -24) and np.all(c > 0.0) and np.all(dot > -4.0 * 2.0 ** -24)
        o = rays[ok][..., :3]
        if bias == 0.0:
            assert np.array_equal(_u32(o), _u32(np.repeat(pos[ok][:, None, :], D, axis=1)))
        else:
            assert np.all(np.abs(o.astype(np.float64) - (pos[ok].astype(np.float64) + bias * nh)[:, None, :]) <= 2.0 ** -23 * 4.0)
    # an unusable point resolves to (0, 0, 0, 1): nothing was ever added to its sums
    hits_t, hits_o = np.zeros(20 * D, np.float32), np.zeros(20 * D, np.uint32)
    sums = api.ao_reduce(AmbientOcclusion(1.0, D), rays.reshape(-1, 6), hits_t, hits_o).astype(np.float32)
    assert np.all(sums[~ok] == 0.0) and np.all(api.ao_resolve(sums, 1)[~ok] == np.array([0.0, 0.0, 0.0, 1.0], np.float32))


@pytest.mark.parametrize("D", [16, 64, 256, 4096])
def test_known_answers_through_the_reduction(D):
    pos = np.array([[0.5, -1.0, 2.0], [0.0, 0.0, 0.0]], np.float32)
    nrm = np.array([[0.0, 0.0, 2.0], [1.0, -2.0, 0.5]], np.float32)
    nh = nrm.astype(np.float64) / np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True)
    ao = AmbientOcclusion(4.0, D, 0, 0.0).seed(9)
    rays = api.ao_rays(ao, pos, nrm)
    n = 2 * D
    # all misses: ao = 1 and the bent normal is the normal, within the lattice's own error: the mean of cosine-weighted directions is
    # (2/3) n, its c-term off by at most 1 / D (a rectangle rule, one node per cell) and its tangential part by at most
    # 2 / (D sin(pi g)) (tests/lightmap_ref.py's summation by parts), so the direction is off by at most (3/2)(1 + 2 / sin(pi g)) / D
    sums = api.ao_reduce(ao, rays, np.zeros(n, np.float32), np.full(n, MISS))
    assert np.all(sums[:, 3] == 0.0)
    out = api.ao_resolve(sums.astype(np.float32), 1)
    assert np.all(out[:, 3] == 1.0)
    lattice = 1.5 * (1.0 + 2.0 / abs(np.sin(np.pi * LM.G))) / D
    assert np.all(np.linalg.norm(out[:, :3].astype(np.float64) - nh, axis=1) <= 2.0 * lattice / (1.0 - lattice) + 1e-6), D
    # every ray hit inside the radius, falloff 0: (0, 0, 0, 0)
    sums = api.ao_reduce(ao, rays, np.full(n, 1.5, np.float32), np.zeros(n, np.uint32))
    assert np.all(sums[:, :3] == 0.0) and np.all(sums[:, 3] == 1.0)
    assert np.all(api.ao_resolve(sums.astype(np.float32), 1) == 0.0)
    # a hit at or beyond the radius does not occlude; an infinite radius makes every hit occlude
    sums = api.ao_reduce(ao, rays, np.full(n, 4.5, np.float32), np.zeros(n, np.uint32))
    assert np.all(sums[:, 3] == 0.0)
    sums = api.ao_reduce(AmbientOcclusion(INF, D), rays, np.full(n, 1e30, np.float32), np.zeros(n, np.uint32))
    assert np.all(sums[:, 3] == 1.0)
    # falloff 1 with every hit at dist = radius / 2: O = 1/2 exactly — directions of length exactly 2 (0.5 x 2 = 1 = radius / 2 of 2)
    unit = np.zeros((n, 6), np.float32)
    unit[np.arange(n), 3 + np.arange(n) % 3] = 2.0
    half = api.ao_reduce(AmbientOcclusion(2.0, D, 1), unit, np.full(n, 0.5, np.float32), np.zeros(n, np.uint32))
    assert np.all(half[:, 3] == 0.5)
    assert np.all(api.ao_resolve(half.astype(np.float32), 1)[:, 3] == 0.5)
    # progressive sums: R rounds of O = 1/2 resolve to the same ao
    assert np.all(api.ao_resolve((3.0 * half).astype(np.float32), 3)[:, 3] == 0.5)


@pytest.mark.parametrize("D", [16, 64, 256, 4096])
@pytest.mark.parametrize("jitter", [False, True])
def test_occluder_in_closed_form(D, jitter):
    """a sphere of radius rho at height h on the normal is hit iff u_j < rho^2 / h^2 (tests/ao_ref.py): ao = 1 - rho^2 / h^2 within 1 / D;
    with radius < h - rho no hit is near enough: ao = 1 exactly"""
    rho, h = 1.0, 1.6
    pos = np.array([[0.25, 0.0, -0.5]], np.float32)
    nrm = np.array([[0.0, 1.0, 0.0]], np.float32)
    centre = pos[0].astype(np.float64) + h * nrm[0]
    for rnd in (0, 3):
        ao = AmbientOcclusion(10.0, D, 0, 0.0).seed(5).jitter(jitter)
        rays = api.ao_rays(ao, pos, nrm, None, rnd)
        t, obj = R.sphere_hits(rays, centre, rho)
        out = api.ao_resolve(api.ao_reduce(ao, rays, t, obj).astype(np.float32), 1)
        print(f"D {D} jitter {jitter} round {rnd}: ao {out[0, 3]:.6f}, closed form {1.0 - rho * rho / (h * h):.6f}")
        assert abs(float(out[0, 3]) - (1.0 - rho * rho / (h * h))) <= 1.0 / D
        # the unoccluded rays are the outer ring, symmetric around the normal up to the lattice: the bent normal leans nowhere far
        assert out[0, 1] > 0.5
        near = AmbientOcclusion(np.float32(0.999 * (h - rho)), D, 0, 0.0).seed(5).jitter(jitter)
        for falloff in (0, 1):
            near.falloff = falloff
            sums = api.ao_reduce(near, rays, t, obj)
            assert sums[0, 3] == 0.0 and api.ao_resolve(sums.astype(np.float32), 1)[0, 3] == 1.0
