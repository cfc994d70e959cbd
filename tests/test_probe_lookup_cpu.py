"""CPU-side checks of the probe lookup (fw_probe_irradiance, fw_probe_shade): the exports and the two structs' layouts at
ABI 8, every argument error of both calls in the header's order (before HIP is called), the no-device error with the caller's buffers
left as they were, ProbeSet.grid's memory, the numpy statement's known answers (api.probe_lookup, api.probe_shade_ref) and the CLI's
refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import ProbeGrid, ProbeSet

import probe_lookup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    for name, args in (("fw_probe_irradiance", r"const fw_probe_grid \*grid, const float \*sh, int device, uint32_t n, const float \*positions, "
                                               r"const float \*normals,\s+uint32_t stride_floats, float \*irradiance, int on_device, void \*stream"),
                       ("fw_probe_shade", r"const fw_probe_grid \*grid, const float \*sh, const fw_probe_shade_params \*p, const float \*aov, "
                                          r"float \*linear_rgb,\s+float \*gamma_rgb, uint8_t \*rgb8")):
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\s*\({args}\);", text), name
    assert re.search(r"#define FW_PROBE_WRAP 1u\b", text) and A.FW_PROBE_WRAP == 1


@pytest.mark.parametrize("struct,names", [(A.fw_probe_grid, ["lo", "hi", "counts", "flags"]),
                                          (A.fw_probe_shade_params, ["width", "height", "gamma", "device", "on_device", "stream"])])
def test_struct_layouts(tmp_path, struct, names):
    """ctypes' struct equals the C compiler's, size and every field offset"""
    assert [f for f, _ in struct._fields_] == names
    t = struct.__name__
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(names) +
           f'\\n",sizeof({t})' + "".join(f",offsetof({t},{f})" for f in names) + ');return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out[0] == C.sizeof(struct)
    assert out[1:] == [getattr(struct, f).offset for f in names]


def _grid(lo=(0.0, 0.0, 0.0), hi=(1.0, 2.0, 3.0), counts=(2, 3, 2), flags=1):
    g = A.fw_probe_grid()
    for k in range(3):
        g.lo[k], g.hi[k], g.counts[k] = lo[k], hi[k], counts[k]
    g.flags = flags
    return g


def _bad_grids():
    """(what, grid) for every grid error of the header, in its order"""
    out = [(f"count {k}", _grid(counts=tuple(0 if j == k else 2 for j in range(3)))) for k in range(3)]
    out += [("lo nan", _grid(lo=(0.0, NAN, 0.0))), ("hi inf", _grid(hi=(1.0, 2.0, INF))), ("lo -inf", _grid(lo=(-INF, 0.0, 0.0))),
            ("hi == lo", _grid(lo=(0.0, 2.0, 0.0))), ("hi - lo overflows", _grid(lo=(0.0, -1.7e308, 0.0), hi=(1.0, 1.7e308, 3.0))),
            ("hi - lo overflows on a flat axis", _grid(lo=(0.0, 0.0, -1.7e308), hi=(1.0, 2.0, 1.7e308), counts=(2, 3, 1))), ("flags", _grid(flags=2)), ("flags", _grid(flags=0x80000001))]
    return out


BIG = (1 << 11, 1 << 10, 1 << 10)        # nx ny nz = 2^31 (sh is never read: the count comes first)


def test_a_flat_axis_may_have_equal_corners():
    lib = _lib.load()
    sh = np.zeros((2, 9, 3), np.float32)
    pts = np.zeros((1, 3), np.float32)
    nrm = np.ones((1, 3), np.float32)
    out = np.full((1, 3), 7.0, np.float32)
    st = lib.fw_probe_irradiance(C.byref(_grid(lo=(0.0, 5.0, 1.0), hi=(1.0, 5.0, 1.0), counts=(2, 1, 1))), sh.ctypes.data, 0, 1, pts.ctypes.data,
                                 nrm.ctypes.data, 3, out.ctypes.data, 0, None)
    assert st == (A.FW_ERR_NO_DEVICE if _lib.device_count() == 0 else A.FW_OK)


def test_probe_irradiance_argument_checks():
    lib = _lib.load()
    sh = np.full((12, 9, 3), 7.0, np.float32)
    pts = np.full((5, 3), 7.0, np.float32)
    nrm = np.full((5, 3), 7.0, np.float32)
    out = np.full((5, 3), 7.0, np.float32)
    good = dict(sh=sh.ctypes.data, pos=pts.ctypes.data, nrm=nrm.ctypes.data, out=out.ctypes.data)

    def call(g=None, device=0, n=5, stride=3, on_device=0, null_grid=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_irradiance(None if null_grid else C.byref(g if g is not None else _grid()), a["sh"], device, n, a["pos"], a["nrm"], stride,
                                       a["out"], on_device, None)

    assert call(null_grid=True) == A.FW_ERR_BAD_ARG
    for name in good:
        assert call(**{name: None}) == A.FW_ERR_BAD_ARG, name
    for what, g in _bad_grids():
        assert call(g) == A.FW_ERR_BAD_ARG, what
    assert call(n=0) == A.FW_ERR_BAD_ARG
    assert call(stride=0) == A.FW_ERR_BAD_ARG and call(stride=2) == A.FW_ERR_BAD_ARG
    assert call(device=-1) == A.FW_ERR_BAD_ARG
    for name in good:
        assert call(on_device=1, **{name: C.c_void_p(good[name] + 2)}) == A.FW_ERR_BAD_ARG, name
    # the order: bad arguments before the size limit, the size limit before the device
    big = _grid(counts=BIG)
    assert call(big, n=0) == A.FW_ERR_BAD_ARG and call(big, stride=2) == A.FW_ERR_BAD_ARG and call(big, device=-1) == A.FW_ERR_BAD_ARG
    assert call(_grid(counts=BIG, flags=4)) == A.FW_ERR_BAD_ARG
    assert call(big) == A.FW_ERR_UNSUPPORTED
    assert call(_grid(counts=(1 << 16, 1 << 16, 1))) == A.FW_ERR_UNSUPPORTED                 # nx ny alone is past the limit
    assert call(_grid(counts=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))) == A.FW_ERR_UNSUPPORTED   # (no 64-bit wrap)
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE
        assert call(device=5) == A.FW_ERR_NO_DEVICE                                          # the device index is looked at after the device count
        assert call(_grid(flags=0), stride=12, n=1) == A.FW_ERR_NO_DEVICE
        assert np.all(out == 7.0) and np.all(pts == 7.0) and np.all(nrm == 7.0) and np.all(sh == 7.0)
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG


def _params(**kw):
    p = A.fw_probe_shade_params()
    p.width, p.height, p.gamma, p.device = 4, 2, 2.2, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_probe_shade_argument_checks():
    lib = _lib.load()
    sh = np.full((12, 9, 3), 7.0, np.float32)
    aov = np.full((8, 12), 7.0, np.float32)
    lin = np.full((8, 3), 7.0, np.float32)
    gam = np.full((8, 3), 7.0, np.float32)
    rgb8 = np.full((8, 3), 7, np.uint8)
    assert aov.ctypes.data % 16 == 0
    good = dict(sh=sh.ctypes.data, aov=aov.ctypes.data, lin=lin.ctypes.data, gam=gam.ctypes.data, rgb8=rgb8.ctypes.data)

    def call(g=None, p=None, null_grid=False, null_p=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_shade(None if null_grid else C.byref(g if g is not None else _grid()), a["sh"],
                                  None if null_p else C.byref(p if p is not None else _params()), a["aov"], a["lin"], a["gam"], a["rgb8"])

    assert call(null_grid=True) == A.FW_ERR_BAD_ARG and call(null_p=True) == A.FW_ERR_BAD_ARG
    assert call(sh=None) == A.FW_ERR_BAD_ARG and call(aov=None) == A.FW_ERR_BAD_ARG
    assert call(lin=None, gam=None, rgb8=None) == A.FW_ERR_BAD_ARG                             # all three outputs NULL
    for what, g in _bad_grids():
        assert call(g) == A.FW_ERR_BAD_ARG, what
    assert call(p=_params(width=0)) == A.FW_ERR_BAD_ARG and call(p=_params(height=0)) == A.FW_ERR_BAD_ARG
    for gamma in (0.0, -1.0, NAN, INF):
        assert call(p=_params(gamma=gamma)) == A.FW_ERR_BAD_ARG, gamma
    assert call(p=_params(device=-1)) == A.FW_ERR_BAD_ARG
    for name, off in (("aov", 4), ("aov", 8), ("sh", 2), ("lin", 2), ("gam", 1)):
        assert call(p=_params(on_device=1), **{name: C.c_void_p(good[name] + off)}) == A.FW_ERR_BAD_ARG, name
    # the order
    big = _grid(counts=BIG)
    huge = dict(width=1 << 16, height=1 << 16)                                                 # W x H = 2^32
    assert call(big, _params(width=0)) == A.FW_ERR_BAD_ARG and call(big, _params(gamma=0.0)) == A.FW_ERR_BAD_ARG
    assert call(p=_params(gamma=NAN, **huge)) == A.FW_ERR_BAD_ARG and call(p=_params(device=-1, **huge)) == A.FW_ERR_BAD_ARG
    assert call(big) == A.FW_ERR_UNSUPPORTED
    assert call(p=_params(**huge)) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE
        assert call(p=_params(device=5)) == A.FW_ERR_NO_DEVICE
        for only in ("lin", "gam", "rgb8"):                                                    # any single output will do
            assert call(**{k: None for k in ("lin", "gam", "rgb8") if k != only}) == A.FW_ERR_NO_DEVICE, only
        assert call(p=_params(width=0xFFFFFFFF, height=1)) == A.FW_ERR_NO_DEVICE               # the largest frame that is not refused
        assert np.all(lin == 7.0) and np.all(gam == 7.0) and np.all(rgb8 == 7) and np.all(aov == 7.0)
    else:
        assert call(p=_params(device=_lib.device_count())) == A.FW_ERR_BAD_ARG


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    probes = ProbeSet.grid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    sh = np.zeros((8, 9, 3), np.float32)
    pts = np.zeros((3, 3), np.float32)
    aov = np.zeros((6, 12), np.float32)
    for call in (lambda: _lib.probe_irradiance(probes, sh, pts, pts + 1), lambda: _lib.probe_shade(probes, sh, aov, 3, 2)):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


def test_probe_set_grid_remembers_its_corners():
    g = ProbeSet.grid((0.1, -1.0, 10.0), (3.0, 1.0, 10.5), (4, 3, 2), directions=32)
    assert g.grid_lo == (0.1, -1.0, 10.0) and g.grid_hi == (3.0, 1.0, 10.5) and g.grid_counts == (4, 3, 2)
    assert all(type(v) is float for v in g.grid_lo + g.grid_hi) and all(type(n) is int for n in g.grid_counts)      # float64, not float32
    free = ProbeSet(g.positions, 32)
    assert free.grid_lo is None and free.grid_hi is None and free.grid_counts is None
    assert np.array_equal(free.positions, g.positions) and free.to_abi()[0].n_probes == g.to_abi()[0].n_probes == 24
    with pytest.raises(ValueError, match="no grid"):
        ProbeGrid.of(free)
    with pytest.raises(ValueError, match="no grid"):
        api.probe_lookup(free, np.zeros((24, 9, 3), np.float32), np.zeros((1, 3)), np.ones((1, 3)))
    with pytest.raises(ValueError, match="no grid"):
        api.Renderer.default().render_probe_lit(None, free, np.zeros((24, 9, 3), np.float32))      # before the scene or the device is looked at
    pg = ProbeGrid.of(g, wrap=False)
    abi = pg.to_abi()
    assert (list(abi.lo), list(abi.hi), list(abi.counts), abi.flags) == ([0.1, -1.0, 10.0], [3.0, 1.0, 10.5], [4, 3, 2], 0)
    assert ProbeGrid.of(g).to_abi().flags == A.FW_PROBE_WRAP and pg.n_probes == 24 and ProbeGrid.of(pg) is pg


RNG = np.random.default_rng(20)
NORMALS = np.array([[0.0, 1.0, 0.0], [0.0, -2.0, 0.0], [0.6, 0.0, -0.8], [1.0, 2.0, -2.0], [-0.25, 0.25, 0.25]], np.float32)


def _unit(n):
    n = np.asarray(n, np.float32).astype(np.float64)
    return n / np.sqrt((n * n).sum(axis=1, keepdims=True))


def _own(sh, which, normals):
    """api.sh_irradiance of probe `which[i]` for normal i: (N, 3)"""
    return np.stack([api.sh_irradiance(sh[p], _unit(normals[i:i + 1]))[0] for i, p in enumerate(which)])


@pytest.mark.parametrize("wrap", [False, True])
def test_lookup_at_a_probe_is_that_probes_irradiance(wrap):
    """positions that float32 holds exactly: at a probe every other corner's trilinear weight is exactly 0 (and stays 0 under wrap), so
    the lookup is sh_irradiance of that one probe up to the float64 roundings of two different summation orders"""
    probes = ProbeSet.grid((0.0, -1.0, 8.0), (3.0, 1.0, 10.0), (4, 3, 5))
    sh = RNG.normal(size=(probes.n_probes, 9, 3)).astype(np.float32)
    which = [0, 3, 7, 30, 59]
    E, T = api.probe_lookup(ProbeGrid.of(probes, wrap), sh, probes.positions[which], NORMALS, terms=True)
    assert np.all(np.abs(E - _own(sh, which, NORMALS)) <= 40 * 2.0 ** -53 * T)


@pytest.mark.parametrize("wrap", [False, True])
def test_equal_probes_give_a_position_independent_result(wrap):
    one = RNG.normal(size=(9, 3)).astype(np.float32)
    probes = ProbeSet.grid((-1.0, 0.0, 2.0), (2.0, 1.5, 3.0), (3, 2, 4))
    sh = np.broadcast_to(one, (probes.n_probes, 9, 3))
    pts = RNG.uniform(-3.0, 5.0, size=(64, 3)).astype(np.float32)                             # inside and outside
    nrm = np.tile(NORMALS, (13, 1))[:64]
    E, T = api.probe_lookup(ProbeGrid.of(probes, wrap), sh, pts, nrm, terms=True)
    want = _own(sh, [0] * 64, nrm)
    assert np.all(np.abs(E - want) <= R.rounding_count(wrap) * 2.0 ** -53 * T)                # the weights sum to 1 within their roundings


def test_a_linear_c0_is_reproduced_inside_and_held_outside():
    lo, hi, nx = 1.0, 4.0, 7
    probes = ProbeSet.grid((lo, 0.0, 0.0), (hi, 1.0, 1.0), (nx, 2, 2))
    c0 = lambda x: np.stack([2.0 + 0.5 * x, 1.0 - 0.125 * x, 0.25 * x], axis=-1)            # noqa: E731
    sh = np.zeros((probes.n_probes, 9, 3), np.float32)
    sh[:, 0] = c0(probes.positions[:, 0].astype(np.float64))                                   # (exact in float32: multiples of 1/16)
    assert np.array_equal(sh[:, 0].astype(np.float64), c0(probes.positions[:, 0].astype(np.float64)))
    x = np.array([1.0, 1.3, 2.71, 3.999, 4.0, 0.5, -100.0, 4.5, 1e6], np.float32)
    pts = np.stack([x, RNG.uniform(-1, 2, x.size).astype(np.float32), RNG.uniform(-1, 2, x.size).astype(np.float32)], axis=1)
    nrm = np.tile(NORMALS, (2, 1))[:x.size]
    E = api.probe_lookup(ProbeGrid.of(probes, False), sh, pts, nrm)
    want = np.pi * api._SH_Y0 * c0(np.clip(x.astype(np.float64), lo, hi))
    assert np.all(np.abs(E - want) <= 64 * 2.0 ** -53 * np.abs(want).max())


def test_flat_axes():
    """a 1 x 3 x 1 grid interpolates along y only; a 1 x 1 x 1 grid is its one probe everywhere"""
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (9.0, 2.0, 9.0), (1, 3, 1))
    sh = RNG.normal(size=(3, 9, 3)).astype(np.float32)
    pts = np.array([[100.0, 0.5, -7.0], [4.5, 1.0, 4.5], [0.0, 1.75, 0.0], [0.0, 9.0, 0.0]], np.float32)
    nrm = NORMALS[:4]
    for wrap in (False, True):
        E = api.probe_lookup(ProbeGrid.of(probes, wrap), sh, pts, nrm)
        assert np.all(np.isfinite(E))
        assert np.allclose(E[1], _own(sh, [1], nrm[1:2])[0], rtol=0, atol=1e-13)
        assert np.allclose(E[3], _own(sh, [2], nrm[3:4])[0], rtol=0, atol=1e-13)
    E = api.probe_lookup(ProbeGrid.of(probes, False), sh, pts, nrm)
    assert np.allclose(E[0], 0.5 * _own(sh, [0], nrm[0:1])[0] + 0.5 * _own(sh, [1], nrm[0:1])[0], rtol=0, atol=1e-13)
    assert np.allclose(E[2], 0.25 * _own(sh, [1], nrm[2:3])[0] + 0.75 * _own(sh, [2], nrm[2:3])[0], rtol=0, atol=1e-13)
    single = ProbeGrid((5.0, 5.0, 5.0), (5.0, 5.0, 5.0), (1, 1, 1))
    E = api.probe_lookup(single, sh[:1], pts, nrm)
    assert np.allclose(E, _own(sh, [0] * 4, nrm), rtol=0, atol=1e-13)
    E = api.probe_lookup(single, sh[:1], np.array([[5.0, 5.0, 5.0]], np.float32), nrm[:1])      # r = 0: the factor 1.2 cancels
    assert np.allclose(E, _own(sh, [0], nrm[:1]), rtol=0, atol=1e-13)


def test_constant_radiance_closed_form():
    """probes that hold the projection of a constant radiance L (c0 = 2 sqrt(pi) L): E = pi L for every point and normal"""
    L = np.array([0.25, 1.5, 3.0], np.float32)
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2))
    sh = np.zeros((8, 9, 3))
    sh[:, 0] = 2.0 * np.sqrt(np.pi) * L
    sh32 = sh.astype(np.float32)
    pts = RNG.uniform(-0.5, 1.5, size=(40, 3)).astype(np.float32)
    nrm = np.tile(NORMALS, (8, 1))
    for wrap in (False, True):
        E = api.probe_lookup(ProbeGrid.of(probes, wrap), sh32, pts, nrm)
        assert np.all(np.abs(E - np.pi * L.astype(np.float64)) <= (2.0 ** -24 + 200 * 2.0 ** -53) * np.pi * L)      # (sh32's own rounding)


def test_invalid_points_give_zeros():
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2))
    sh = RNG.normal(size=(8, 9, 3)).astype(np.float32)
    pts = np.array([[0.5, 0.5, 0.5], [NAN, 0.5, 0.5], [0.5, INF, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.25, 0.5, 0.5]], np.float32)
    nrm = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0], [0, NAN, 1], [0, 1e-30, 0]], np.float32)
    for wrap in (False, True):
        E = api.probe_lookup(ProbeGrid.of(probes, wrap), sh, pts, nrm)
        assert np.all(E[1:5] == 0.0) and np.all(E[0] != 0.0) and np.all(np.isfinite(E))
        assert np.all(E[5] != 0.0)                                                            # a tiny normal is still a direction


def test_shade_statement():
    """out = a (v max(E, 0) / pi + (1 - v)) in float32: v = 0 passes the albedo, a negative lookup is clamped, the given irradiance is used"""
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2))
    sh = np.zeros((8, 9, 3), np.float32)
    sh[:, 0] = (1.0, -2.0, 0.5)
    aov = np.zeros((3, 12), np.float32)
    aov[:, 0:3] = (0.5, 0.25, 1.0)
    aov[:, 3] = (0.0, 0.25, 1.0)
    aov[1:, 4:7] = (0.0, 0.0, 1.0)
    aov[:, 8:11] = 0.5
    out = api.probe_shade_ref(probes, sh, aov)
    assert out.dtype == np.float32 and np.array_equal(out[0], aov[0, 0:3])
    E = np.float32(np.pi * api._SH_Y0) * np.array([1.0, 0.0, 0.5], np.float32)                 # the green lookup is negative: clamped
    for i, v in ((1, 0.25), (2, 1.0)):
        want = aov[i, 0:3].astype(np.float64) * (v * E.astype(np.float64) / np.pi + (1.0 - v))
        assert np.all(np.abs(out[i] - want) <= 4 * 2.0 ** -24 * np.abs(want) + 1e-9)
    assert np.array_equal(out[2, 1], np.float32(0.0))
    given = np.array([[9.0, 9.0, 9.0], [-1.0, np.pi, 0.0], [np.pi, np.pi, np.pi]], np.float32)
    out = api.probe_shade_ref(probes, sh, aov, given)
    assert np.array_equal(out[0], aov[0, 0:3]) and np.allclose(out[2], aov[2, 0:3], rtol=1e-6)
    assert np.allclose(out[1], aov[1, 0:3] * np.array([0.75, 1.0, 0.75]), rtol=1e-6)


def _npz(path, **kw):
    with open(path, "wb") as f:
        np.savez(f, **kw)
    return str(path)


def test_cli_probe_lit_checks(capsys, tmp_path):
    from firework_amd.__main__ import main
    base = ["--scene-file", "s.yml", "-s", "4", "--probe-lit", "p.npz", "-o", "x.png"]
    for extra in (["--camera", "panorama"], ["--denoise"], ["--orbit", "3"], ["--adaptive", "0.05"], ["--progressive", "2"],
                  ["--checkpoint", "c.npz"], ["--temporal"], ["--bake-probes", "2,2,2", "--probe-min", "0,0,0", "--probe-max", "1,1,1"],
                  ["--bake-lightmap", "0,8,8"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
        assert "--probe-lit cannot be combined" in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as e:
        main(base[:-2])
    assert e.value.code == 2 and "-o" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "s.yml", "-s", "4", "-o", "x.png", "--probe-no-wrap"])
    assert e.value.code == 2 and "needs --probe-lit" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(base + ["--aov-samples", "0"])
    assert e.value.code == 2 and "--aov-samples" in capsys.readouterr().err
    # files that cannot be looked up: a message and status 2 before the scene file or the device is looked for (s.yml does not exist)
    sh = np.zeros((8, 9, 3), np.float32)
    old = _npz(tmp_path / "old.npz", positions=np.zeros((8, 3), np.float32), sh=sh, sums=sh, rounds=np.int64(1), directions=np.int64(8),
               samples=np.int64(1))
    wrong = _npz(tmp_path / "wrong.npz", sh=sh, grid_lo=np.zeros(3), grid_hi=np.ones(3), grid_counts=np.array([2, 2, 3]))
    for path, word in ((old, "grid_lo"), (wrong, "sh has shape"), (str(tmp_path / "missing.npz"), "missing.npz")):
        assert main(["--scene-file", "s.yml", "-s", "4", "--probe-lit", path, "-o", str(tmp_path / "x.png")]) == 2
        err = capsys.readouterr().err
        assert "--probe-lit" in err and word in err, (path, err)
    assert not os.path.exists(tmp_path / "x.png")



CPP = r"""
#include "firework.hpp"
#include <cstdio>
int main() {
    using namespace firework;
    ProbeSet g = ProbeSet::grid({0.5f, -1.0f, 10.0f}, {3.0f, 1.0f, 10.5f}, 4, 3, 2, 32);
    const fw_probe_grid a = g.grid_abi(), b = g.grid_abi(false);
    bool threw = false;
    try { ProbeSet::new_({{0, 0, 0}}).grid_abi(); } catch (std::runtime_error &) { threw = true; }
    std::printf("%d %g %g %g %g %g %g %u %u %u %u %u %d %zu\n", (int)g.has_grid, a.lo[0], a.lo[1], a.lo[2], a.hi[0], a.hi[1], a.hi[2], a.counts[0],
                a.counts[1], a.counts[2], a.flags, b.flags, (int)threw, g.n_probes());
    auto probe_lit = &Renderer::probe_lit;      // the preview is declared (it needs a device to run)
    return probe_lit ? 0 : 1;
}
"""


def test_cpp_probe_set_keeps_its_grid(tmp_path):
    (tmp_path / "t.cpp").write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.cpp"),
                           "-L", os.path.join(ROOT, "firework_amd", "lib"), "-lfirework_hip", "-Wl,-rpath," + os.path.join(ROOT, "firework_amd", "lib")])
    out = subprocess.check_output([str(tmp_path / "t")], text=True).split()
    assert out == ["1", "0.5", "-1", "10", "3", "1", "10.5", "4", "3", "2", "1", "0", "1", "24"]
