"""CPU-side checks of the final gather (fw_hit_surface, fw_gather_reduce, fw_bake_gather): the exports and fw_gather's
layout at ABI 8; every argument error of the three calls in the header's order (they come before the scene is looked at or HIP is called)
and the no-device error with the caller's buffers untouched; FinalGather.check; the numpy statements — api.gather_reduce against
hand-computed cases and against a plain loop written from the statement, at D = 1, 3 and 65 (the group size, the tail, the butterfly's
order), api.gather_resolve, api.surface_facing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import FinalGather

import gather_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
PI = 3.141592653589793


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.GATHER_PROTOTYPES) == ["fw_bake_gather", "fw_gather_reduce", "fw_hit_surface"]
    for name in A.GATHER_PROTOTYPES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name
    assert _lib.SURFACE_COLUMNS == dict(albedo=slice(0, 3), kind=3, normal=slice(4, 7), distance=7, position=slice(8, 11), emitted=slice(12, 15))


def test_struct_layout(tmp_path):
    """ctypes' fw_gather equals the C compiler's, size and every field offset"""
    names = ["directions", "jitter", "bias", "direct_bias", "flags", "chunk_points", "seed"]
    assert [f for f, _ in A.fw_gather._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 2) + '\\n",sizeof(fw_gather)' +
           "".join(f",offsetof(fw_gather,{f})" for f in names) + ",(size_t)FW_GATHER_DIRECT);return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_gather)] + [getattr(A.fw_gather, f).offset for f in names] + [A.FW_GATHER_DIRECT]
    g = FinalGather(33, 0.25, True, 0.5).seed(7).jitter(False).to_abi()
    assert (g.directions, g.jitter, g.bias, g.direct_bias, g.flags, g.chunk_points, g.seed) == (33, 0, 0.25, 0.5, A.FW_GATHER_DIRECT, 0, 7)
    a = FinalGather(33, 0.25).seed(7).ao()
    assert (a.radius, a.directions, a.falloff, a.bias, a._seed, a._jitter) == (INF, 33, 0, 0.25, 7, True)


# ---- the numpy statements -----------------------------------------------------------------------------------------------------------
def _record(kind, albedo=(0, 0, 0), emitted=(0, 0, 0)):
    r = np.full(16, NAN, np.float32)
    r[0:3], r[3], r[12:15] = albedo, kind, emitted
    return r


def test_gather_reduce_by_hand():
    # D = 1: one diffuse ray: (pi / 1) ((a E) (1 / pi)) per channel; a negative E is clamped; sky 0
    s = _record(0, (0.5, 0.25, 1.0))[None]
    out = api.gather_reduce(s, [[2.0, 4.0, -3.0]], 1)
    assert out.shape == (1, 4) and out.dtype == np.float64
    assert np.array_equal(out[0], [PI * ((0.5 * 2.0) * (1.0 / PI)), PI * ((0.25 * 4.0) * (1.0 / PI)), 0.0, 0.0])
    # ... with direct: T = max(E, 0) + Ed, Ed added after the clamp
    ed = np.array([[1.0, 0.5, 2.0, NAN, NAN, NAN, NAN, NAN]], np.float32)
    out = api.gather_reduce(s, [[2.0, 4.0, -3.0]], 1, direct=ed)
    assert np.array_equal(out[0], [PI * ((0.5 * 3.0) * (1.0 / PI)), PI * ((0.25 * 4.5) * (1.0 / PI)), PI * ((1.0 * 2.0) * (1.0 / PI)), 0.0])
    # D = 4, one of each: an emitter (not clamped, its albedo and E ignored), the environment (counts as sky), a ray that was not traced
    s = np.stack([_record(3, (9, 9, 9), (15.0, 0.0, 2.0)), _record(-1, (9, 9, 9), (1.0, 2.0, 3.0)), _record(-2, (9, 9, 9), (7.0, 7.0, 7.0)),
                  _record(5, (1.0, 1.0, 0.0))])
    E = np.array([[NAN, NAN, NAN], [NAN, NAN, NAN], [NAN, NAN, NAN], [PI, 2 * PI, 5.0]], np.float32)
    out = api.gather_reduce(s, E, 4)
    e = E.astype(np.float64)
    # G = 4: lane l holds ray l; the butterfly adds (0 + 2) + (1 + 3)
    want = [(PI / 4) * ((15.0 + 0.0) + (1.0 + (1.0 * e[3, 0]) * (1.0 / PI))), (PI / 4) * ((0.0 + 0.0) + (2.0 + (1.0 * e[3, 1]) * (1.0 / PI))),
            (PI / 4) * ((2.0 + 0.0) + (3.0 + 0.0)), 0.25]
    assert np.array_equal(out[0], want)
    # two points: each is its own
    both = api.gather_reduce(np.concatenate([s, s[::-1]]), np.concatenate([E, E[::-1]]), 4)
    assert np.array_equal(both[0], out[0]) and both[1, 3] == 0.25


@pytest.mark.parametrize("D", [1, 3, 65, 64, 200])
def test_gather_reduce_keeps_the_statements_order(D):
    """bit for bit a plain loop over Python floats: G partial sums in ascending j, then the xor butterfly"""
    rng = np.random.default_rng(D)
    s, E, Ed = R.synthetic_records(6, D, rng, unusable=1)
    for direct in (None, Ed):
        got, want = api.gather_reduce(s, E, D, direct), R.reduce_loop(s, E, D, direct)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (D, direct is None)
        assert np.all(got[-1] == 0.0) and np.all(np.isfinite(got))


def test_gather_resolve_and_surface_facing():
    sums = np.array([[3.0, 1.0, 0.5, 2.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    out = api.gather_resolve(sums, 3)
    assert out.dtype == np.float32 and np.array_equal(out, (sums.astype(np.float64) / 3.0).astype(np.float32)) and np.all(out[1] == 0.0)
    n = np.array([[0.0, 2.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 4.0], [1.0, 1.0, 1.0]], np.float32)
    d = np.array([[0.0, -1.0, 0.0], [0.3, 5.0, 0.0], [1.0, 1.0, 1.0], [-1.0, 0.0, 1.0], [1.0, -1.0, 0.0]], np.float32)
    f = api.surface_facing(n, d)
    assert f.dtype == np.float32
    assert np.array_equal(f[0], [0.0, 1.0, 0.0]) and np.array_equal(f[1], [-0.0, -1.0, -0.0]) and np.signbit(f[1, 0])
    assert np.array_equal(R.u32(f[2]), R.u32(np.zeros(3, np.float32)))                            # a zero normal stays (+0, +0, +0)
    assert np.array_equal(f[3], [np.float32(-3.0) / np.float32(5.0), -0.0, np.float32(-4.0) / np.float32(5.0)])      # dot = 1 > 0: negated
    inv = np.float32(1.0) / np.sqrt(np.float32(3.0))
    assert np.array_equal(f[4], [inv, inv, inv])                                                  # dot = 0: not negated


def test_final_gather_check():
    for bad, word in ((FinalGather(0), "directions"), (FinalGather((1 << 20) + 1), "directions"), (FinalGather(4, -1.0), "bias"),
                      (FinalGather(4, NAN), "bias"), (FinalGather(4, 0.0, True, -1.0), "direct_bias"), (FinalGather(4, 0.0, True, INF), "direct_bias")):
        with pytest.raises(ValueError, match=word):
            bad.check()
    g = FinalGather(1 << 20, 0.0).check()
    assert g.directions == 1 << 20 and g.to_abi().flags == 0


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def test_hit_surface_argument_checks():
    """fw_trace_rays' pattern: every refusal comes before the scene is looked at, so a handle that is never dereferenced will do"""
    lib = _lib.load()
    buf = dict(rays=np.full((4, 6), 7.0, np.float32), hits=np.full((4, 12), 7.0, np.float32), surface=np.full((4, 16), 7.0, np.float32))
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)

    def call(scene=scene, n=4, on_device=0, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_hit_surface(scene, a["rays"], a["hits"], n, a["surface"], on_device, None)

    assert _said(lib, call(scene=None, n=0), "null") == A.FW_ERR_BAD_ARG
    assert call(n=0, rays=None, hits=None, surface=None) == A.FW_OK                              # nothing to do, nothing looked at
    for name in good:
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(rays=C.c_void_p(good["rays"] + 2)), "aligned") == A.FW_ERR_BAD_ARG     # host rays too, as fw_trace_rays
    for name, off in (("hits", 4), ("hits", 8), ("surface", 4), ("surface", 8), ("rays", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(on_device=1) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())


def test_gather_reduce_argument_checks():
    lib = _lib.load()
    buf = dict(surface=np.full((4 * 5, 16), 7.0, np.float32), irr=np.full((4 * 5, 3), 7.0, np.float32), direct=np.full((4 * 5, 8), 7.0, np.float32),
               sums=np.full((4, 4), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(D=5, n=4, device=0, on_device=0, ids_p=None, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_gather_reduce(device, D, n, ids_p, a["surface"], a["irr"], a["direct"], a["sums"], on_device, None)

    for name in ("surface", "irr", "sums"):
        assert _said(lib, call(D=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name           # NULL before the directions
    for D in (0, (1 << 20) + 1):
        assert _said(lib, call(D=D, n=0), "directions") == A.FW_ERR_BAD_ARG                      # the directions before n
    assert _said(lib, call(n=0, device=-1), "n must") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("surface", 4), ("surface", 8), ("irr", 2), ("direct", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(D=1 << 20, n=1 << 11, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(D=1 << 20, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(D=1 << 20, n=1 << 11, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED    # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data, direct=None) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def _gather(directions=5, bias=1e-3, direct_bias=1e-3, flags=0):
    g = A.fw_gather()
    g.directions, g.jitter, g.bias, g.direct_bias, g.flags = directions, 1, bias, direct_bias, flags
    return g


def _grid(counts=(2, 2, 2), lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), flags=A.FW_PROBE_WRAP):
    g = A.fw_probe_grid()
    for k in range(3):
        g.lo[k], g.hi[k], g.counts[k] = lo[k], hi[k], counts[k]
    g.flags = flags
    return g


def _depth(resolution=8):
    d = A.fw_probe_depth()
    d.resolution, d.sharpness_log2, d.max_distance = resolution, 0, 10.0
    return d


def test_bake_gather_argument_checks():
    """fw_bake_ao's order, then fw_probe_irradiance_placed's checks of the probes, then the flags, then the sizes, then the device"""
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, np.float32), nrm=np.full((4, 3), 7.0, np.float32), sums=np.full((4, 4), 7.0, np.float32),
               out=np.full((4, 4), 7.0, np.float32), sh=np.full((8, 9, 3), 7.0, np.float32), moments=np.full((8, 8, 8, 2), 7.0, np.float32),
               placement=np.full((8, 4), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call

    def call(g=None, n=4, stride=3, first=0, rounds=1, on_device=0, null=None, ids_p=None, grid=None, pd=None, normal_bias=0.0, with_moments=False,
             with_placement=False, **ptrs):
        a = dict(good, **ptrs)
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, g=C.byref(g if g is not None else _gather()), tp=C.byref(tp), grid=C.byref(grid if grid is not None else _grid()))
        if null:
            args[null] = None
        return lib.fw_bake_gather(args["scene"], args["g"], args["tp"], args["grid"], a["sh"], None if pd is None else C.byref(pd),
                                  a["moments"] if with_moments else None, normal_bias, a["placement"] if with_placement else None, n, a["pos"],
                                  a["nrm"], stride, ids_p, first, rounds, a["sums"], a["out"], None)

    for null in ("scene", "g", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("pos", "nrm"):
        assert _said(lib, call(_gather(directions=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, g in (("directions", _gather(directions=0)), ("directions", _gather(directions=(1 << 20) + 1)), ("bias", _gather(bias=-0.5)),
                    ("bias", _gather(bias=NAN)), ("direct_bias", _gather(direct_bias=-1.0)), ("direct_bias", _gather(direct_bias=INF))):
        assert _said(lib, call(g, n=0), word) == A.FW_ERR_BAD_ARG, word                           # the description before n
    assert _said(lib, call(_gather(directions=0, bias=-1.0, direct_bias=-1.0)), "directions") == A.FW_ERR_BAD_ARG
    assert "direct_bias" not in lib.fw_last_error().decode()
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, rounds=0), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(rounds=0, first=0xFFFFFFFF), "rounds must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1, sums=None), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=2, sums=None, on_device=1, out=C.c_void_p(good["out"] + 4)), "first_round > 0") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("out", 4), ("out", 8), ("pos", 2), ("nrm", 2)):
        assert _said(lib, call(on_device=1, null="grid", **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2), null="grid"), "aligned") == A.FW_ERR_BAD_ARG
    # the probes, after the points: NULL grid or sh, one of pd / moments without the other, the depth description, normal_bias, the grid
    flagged = _gather(flags=2)
    assert _said(lib, call(flagged, null="grid"), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, sh=None), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, pd=_depth()), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, with_moments=True), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, pd=_depth(5), with_moments=True), "resolution") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, pd=_depth(), with_moments=True, normal_bias=-1.0), "normal_bias") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, grid=_grid(counts=(0, 2, 2))), "count") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, grid=_grid(flags=8)), "flags") == A.FW_ERR_BAD_ARG and "probe grid" in lib.fw_last_error().decode()
    for name in ("sh", "moments", "placement"):
        st = call(flagged, on_device=1, pd=_depth(), with_moments=True, with_placement=True, **{name: C.c_void_p(good[name] + 2)})
        assert _said(lib, st, "aligned") == A.FW_ERR_BAD_ARG, name
    # unknown flag bits, after the probes and before the sizes
    big = _gather(directions=1 << 20, flags=2)
    assert _said(lib, call(big, n=1 << 11), "gather flags") == A.FW_ERR_BAD_ARG
    big.flags = A.FW_GATHER_DIRECT
    assert _said(lib, call(big, n=1 << 11, rounds=0), "rounds must") == A.FW_ERR_BAD_ARG          # bad arguments before the size
    assert _said(lib, call(big, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(grid=_grid(counts=(1 << 11, 1 << 10, 1 << 10))), "below 2^31") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(sums=None, out=None) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert call(_gather(flags=A.FW_GATHER_DIRECT), pd=_depth(), with_moments=True, with_placement=True) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())


def test_python_entry_points_check_and_fail_loudly():
    s, E, Ed = R.synthetic_records(2, 4, np.random.default_rng(0), unusable=0)
    with pytest.raises(ValueError, match="surface"):
        _lib.gather_reduce(s[:7], E[:7], 4, np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="sums"):
        _lib.gather_reduce(s, E, 4, np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="irradiance"):
        _lib.gather_reduce(s, E[:7], 4, np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="id"):
        _lib.gather_reduce(s, E, 4, np.zeros((2, 4), np.float32), ids=np.array([0, 2], np.uint32))
    if _lib.device_count() == 0:
        with pytest.raises(_lib.FireworkError) as e:
            _lib.gather_reduce(s, E, 4, np.zeros((2, 4), np.float32), direct=Ed)
        assert e.value.status == A.FW_ERR_NO_DEVICE


# ---- the CLI's refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--probe-gather", "64", "-o", "x.png"], "needs --probe-lit"), (["--gather-bias", "0.1", "--probe-lit", "p.npz", "-o", "x.png"], "needs --probe-gather"),
    (["--probe-lit", "p.npz", "--probe-gather", "64", "--ao", "2", "-o", "x.png"], "cannot be combined with --ao"),
    (["--probe-lit", "p.npz", "--probe-gather", "64", "--probe-split-sum", "-o", "x.png"], "cannot be combined with --probe-split-sum"),
    (["--probe-lit", "p.npz", "--probe-gather", "0", "-o", "x.png"], "D[,ROUNDS]"), (["--probe-lit", "p.npz", "--probe-gather", "x", "-o", "x.png"], "D[,ROUNDS]"),
    (["--probe-lit", "p.npz", "--probe-gather", str((1 << 20) + 1), "-o", "x.png"], "D[,ROUNDS]"),
    (["--probe-lit", "p.npz", "--probe-gather", "64,0", "-o", "x.png"], "D[,ROUNDS]"), (["--probe-lit", "p.npz", "--probe-gather", "64,2,1", "-o", "x.png"], "D[,ROUNDS]"),
    (["--probe-lit", "p.npz", "--probe-gather", "64", "--gather-bias", "-1", "-o", "x.png"], "--gather-bias"),
    (["--probe-lit", "p.npz", "--probe-gather", "64", "--gather-bias", "inf", "-o", "x.png"], "--gather-bias"),
    (["--probe-lit", "p.npz", "--probe-gather", "64"], "-o FILE.png")])
def test_cli_refusals_come_before_the_device(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args


def test_cli_refuses_a_files_radiance_maps_in_use(tmp_path, capsys):
    """the probes file is looked at before the device is: radiance maps in use and --probe-gather are a message and exit status 2"""
    from firework_amd.__main__ import main
    from firework_amd.api import ProbeRadiance
    pr = ProbeRadiance(4, 2, [0.5])
    npz = str(tmp_path / "p.npz")
    np.savez(npz, sh=np.zeros((1, 9, 3), np.float32), grid_lo=np.zeros(3), grid_hi=np.ones(3), grid_counts=np.ones(3, np.int64),
             radiance=np.zeros((1, pr.texels, 4), np.float32), radiance_res=np.int64(4), radiance_sharpness=np.int64(2),
             radiance_roughness=np.array([0.5], np.float32))
    assert main(["--scene-file", "none.yml", "-s", "1", "--probe-lit", npz, "--probe-gather", "8", "-o", str(tmp_path / "x.png")]) == 2
    assert "--probe-no-radiance" in capsys.readouterr().err
