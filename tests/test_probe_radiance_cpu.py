"""CPU-side checks of the probe radiance maps (fw_probe_radiance_reduce, fw_probe_radiance_prefilter, fw_bake_probe_radiance,
fw_probe_radiance_lookup, fw_probe_shade_glossy): the exports and the struct's layout at ABI 8; ProbeRadiance's offsets
and validation; the numpy statements' own properties (a constant map stays constant, a prefiltered texel lies within level 0's range, one
level ignores roughness, a neutral placement reproduces probe_lookup_vis' weights, the hot texel's known answers); and every argument
error of the five calls in the header's order (they come before HIP is called)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import ProbeDepth, ProbeGrid, ProbeRadiance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.PROBE_RADIANCE_PROTOTYPES) == ["fw_bake_probe_radiance", "fw_probe_radiance_lookup", "fw_probe_radiance_prefilter",
                                                   "fw_probe_radiance_reduce", "fw_probe_shade_glossy"]
    for name, argtypes in A.PROBE_RADIANCE_PROTOTYPES.items():
        assert hasattr(lib, name), name
        found = re.findall(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert len(found) == 1, name
        assert len(found[0].split(",")) == len(argtypes), name                               # one ctypes entry per C parameter
        assert getattr(lib, name).argtypes == argtypes
    assert A.FW_PROBE_RADIANCE_MAX_LEVELS == 4 and "#define FW_PROBE_RADIANCE_MAX_LEVELS 4" in text


def test_struct_layout(tmp_path):
    """ctypes' fw_probe_radiance equals the C compiler's, size and every field offset"""
    names = ["resolution", "sharpness_log2", "levels", "roughness"]
    assert [f for f, _ in A.fw_probe_radiance._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n",sizeof(fw_probe_radiance)' +
           "".join(f",offsetof(fw_probe_radiance,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_probe_radiance)] + [getattr(A.fw_probe_radiance, f).offset for f in names]


# ---- ProbeRadiance ------------------------------------------------------------------------------------------------------------------
def test_probe_radiance_offsets_and_defaults():
    pr = ProbeRadiance(32)
    assert (pr.levels, pr.resolutions, pr.offsets, pr.texels) == (4, (32, 16, 8, 4), (0, 1024, 1280, 1344), 1360)
    assert np.array_equal(np.float32(pr.roughness), np.linspace(0.1, 1.0, 4).astype(np.float32)) and pr.sharpness_log2 == 2
    assert [ProbeRadiance(R).levels for R in (4, 8, 16, 32)] == [1, 2, 3, 4]
    assert ProbeRadiance(4).roughness == (float(np.float32(0.1)),) and ProbeRadiance(4).texels == 16
    pr = ProbeRadiance(16, 5, (0.0, 0.5))
    assert (pr.levels, pr.offsets, pr.texels) == (2, (0, 256), 320)
    d = pr.to_abi()
    assert (d.resolution, d.sharpness_log2, d.levels, list(d.roughness)) == (16, 5, 2, [0.0, 0.5, 0.0, 0.0])


@pytest.mark.parametrize("args", [(5,), (64,), (0,), (8, 9), (8, -1), (4, 2, (0.1, 0.5)), (8, 2, (0.1, 0.5, 1.0)), (32, 2, (0.1, 0.2, 0.3, 0.4, 0.5)),
                                  (8, 2, ()), (8, 2, (0.5, 0.5)), (8, 2, (0.6, 0.5)), (8, 2, (-0.1, 0.5)), (8, 2, (0.1, 1.5)), (8, 2, (0.1, NAN))])
def test_probe_radiance_validation(args):
    with pytest.raises(ValueError):
        ProbeRadiance(*args)


# ---- the numpy statements -----------------------------------------------------------------------------------------------------------
def _sums(n, R, rng, lo=0.0, hi=4.0, holes=0):
    s = np.empty((n, R, R, 4), np.float32)
    s[..., 3] = rng.uniform(0.5, 3.0, size=(n, R, R))
    s[..., 0:3] = rng.uniform(lo, hi, size=(n, R, R, 3)) * s[..., 3:4]
    flat = s.reshape(n, R * R, 4)
    for p in range(n):
        flat[p, rng.choice(R * R, holes, replace=False)] = 0.0
    return s


def _points(n, rng, lo, hi):
    pts = (np.asarray(lo) + rng.uniform(-0.2, 1.2, size=(n, 3)) * (np.asarray(hi) - np.asarray(lo))).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]).astype(np.float32)
    dirs = (rng.normal(size=(n, 3)) * np.array([1.0, 2.0, 0.25])[np.arange(n) % 3, None]).astype(np.float32)
    return pts, nrm, dirs


def test_reduce_statement_known_answers():
    """one ray straight at a texel centre at k = 0: w = 1 there, A = L; samples divide; the back hemisphere sees nothing; a NaN radiance
    reaches exactly the texels with w > 0"""
    R = 4
    T = api.probe_depth_dirs(R)
    pr = ProbeRadiance(R, 0)
    rays = np.zeros((2, 6), np.float32)
    rays[:, 3:] = T[1, 2]
    accum = np.array([[8.0, 4.0, 2.0, 1.0], [4.0, 4.0, 4.0, 1.0]], np.float32)
    out = api.probe_radiance_reduce(pr, rays, accum, 4, 2)
    assert out.shape == (1, R, R, 4)
    assert np.all(np.abs(out[0, 1, 2] - np.array([3.0, 2.0, 1.5, 2.0])) <= 1e-6)
    lobe = (T.reshape(-1, 3) @ rays[0, 3:].astype(np.float64)) > 0
    assert np.all(out.reshape(-1, 4)[~lobe] == 0.0) and np.all(out.reshape(-1, 4)[lobe, 3] > 0.0)
    accum[1, 0] = NAN
    bad = api.probe_radiance_reduce(pr, rays, accum, 4, 2).reshape(-1, 4)
    assert np.array_equal(np.isnan(bad[:, 0]), lobe) and not np.isnan(bad[:, 1:]).any()
    sharp = api.probe_radiance_reduce(ProbeRadiance(R, 6), rays[:1], accum[:1], 1, 1)
    assert sharp[0, 1, 2, 3] > 0.99 and np.sort(sharp[0, :, :, 3].ravel())[-2] < 1e-3


def test_solid_angles_sum_to_the_sphere():
    for R, tol in ((4, 1.6e-2), (32, 1.3e-7)):
        _S, omega = api.probe_radiance_sources(R)
        assert abs(omega.sum() / (4.0 * np.pi) - 1.0) <= tol, R
    assert abs(api.probe_radiance_sources(4)[1].sum() / (4.0 * np.pi) - 1.0) > 1.4e-2


@pytest.mark.parametrize("R", [8, 16, 32])
def test_a_constant_level_0_stays_constant_at_every_level_and_in_every_lookup(R):
    rng = np.random.default_rng(R)
    pr = ProbeRadiance(R)
    c = np.array([0.75, 2.5, 0.125])
    sums = np.empty((12, R, R, 4), np.float32)
    sums[..., 3] = rng.uniform(0.5, 3.0, size=(12, R, R))
    sums[..., 0:3] = c * sums[..., 3:4]                       # c and W are dyadic enough: the quotient is c exactly where the product is
    maps = api.probe_radiance_prefilter(pr, sums)
    assert maps.shape == (12, pr.texels, 4) and np.all(maps[..., 3] == 1.0)
    assert np.all(np.abs(maps[..., 0:3] - c) <= 2.0 ** -22 * c)                           # float32 products and quotients of c: a few ulps
    grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (2, 3, 2), True)
    pts, nrm, dirs = _points(64, rng, grid.lo, grid.hi)
    rough = rng.uniform(-0.2, 1.2, size=64).astype(np.float32)
    E = api.probe_radiance_lookup(grid, pr, maps, pts, nrm, dirs, rough)
    assert np.all(np.abs(E - c) <= 2.0 ** -21 * c)


@pytest.mark.parametrize("R,holes", [(8, 0), (16, 40), (32, 300)])
def test_every_prefiltered_texel_lies_within_level_0s_range(R, holes):
    rng = np.random.default_rng(R + 1)
    pr = ProbeRadiance(R)
    maps = api.probe_radiance_prefilter(pr, _sums(2, R, rng, -3.0, 5.0, holes))
    for p in range(2):
        lv0 = maps[p, :R * R]
        data = lv0[lv0[:, 3] == 1.0, 0:3]
        assert len(data) == R * R - holes and np.all(lv0[lv0[:, 3] == 0.0] == 0.0)
        up = maps[p, R * R:]
        assert np.all(up[:, 3] == 1.0)                                                    # every output texel sees some flagged source
        # a convex combination, rounded: within a float32 ulp of the range
        assert np.all(up[:, 0:3] >= data.min(axis=0) - 2.0 ** -22 * np.abs(data.min(axis=0)))
        assert np.all(up[:, 0:3] <= data.max(axis=0) + 2.0 ** -22 * np.abs(data.max(axis=0)))


def test_an_empty_level_0_gives_empty_levels():
    pr = ProbeRadiance(8)
    assert np.all(api.probe_radiance_prefilter(pr, np.zeros((1, 8, 8, 4), np.float32)) == 0.0)


def test_with_one_level_the_lookup_ignores_roughness():
    rng = np.random.default_rng(5)
    pr = ProbeRadiance(8, 2, (0.3,))
    grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (2, 3, 2), False)
    maps = api.probe_radiance_prefilter(pr, _sums(12, 8, rng))
    pts, nrm, dirs = _points(50, rng, grid.lo, grid.hi)
    a = api.probe_radiance_lookup(grid, pr, maps, pts, nrm, dirs, np.full(50, 0.0, np.float32))
    b = api.probe_radiance_lookup(grid, pr, maps, pts, nrm, dirs, rng.uniform(0.0, 1.0, 50).astype(np.float32))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.any(a != 0.0)


def test_the_level_pair_and_the_blend():
    pr = ProbeRadiance(32, 2, (0.1, 0.25, 0.5, 1.0))
    rho = [float(np.float32(v)) for v in pr.roughness]
    l, t = api.probe_radiance_level(pr, np.array([-1.0, rho[0], 0.2, rho[1], 0.3, rho[2], 0.75, rho[3], 7.0]))
    assert l.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2]
    assert t[[0, 1, 3, 5]].tolist() == [0.0, 0.0, 0.0, 0.0] and t[[7, 8]].tolist() == [1.0, 1.0]
    assert abs(t[6] - 0.5) <= 1e-12 and 0.0 < t[2] < 1.0 and 0.0 < t[4] < 1.0


@pytest.mark.parametrize("wrap", [True, False])
def test_a_neutral_placement_reproduces_probe_lookup_vis_weights(wrap):
    """with depth maps the lookup's corner weights are probe_lookup_vis' own, bit for bit: checked through the lookup of maps that hold
    the probe's index, against the same sum formed from probe_lookup_vis' weights"""
    rng = np.random.default_rng(9)
    grid = ProbeGrid((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5), wrap)
    pd = ProbeDepth(8, 4, 20.0)
    moments = np.empty((60, 8, 8, 2), np.float32)
    moments[..., 0] = rng.uniform(0.5, 4.0, size=(60, 8, 8))
    moments[..., 1] = moments[..., 0] ** 2 * rng.uniform(1.05, 1.5, size=(60, 8, 8))
    pr = ProbeRadiance(4)
    maps = np.ones((60, 16, 4), np.float32)
    maps[..., 0] = np.arange(60)[:, None]
    maps[..., 1] = np.arange(60)[:, None] ** 2
    pts, nrm, dirs = _points(120, rng, grid.lo, grid.hi)
    _E, _T, V = api.probe_lookup_vis(grid, np.zeros((60, 9, 3), np.float32), pd, moments, pts, nrm, 0.05, terms=True)
    E, _T2, X = api.probe_radiance_lookup(grid, pr, maps, pts, nrm, dirs, np.full(120, 0.5, np.float32), pd, moments, 0.05, terms=True)
    assert np.array_equal(X["w"].view(np.uint64), V["w"].view(np.uint64))
    assert np.all(np.abs(E[:, 0] - (V["w"] * X["probe"]).sum(axis=1)) <= 1e-9) and np.all(np.abs(E[:, 2] - 1.0) <= 1e-12)


def test_the_hot_texel():
    """One texel of 1000 nearest +x in an otherwise black R = 32 map: the level maxima fall strictly with the level, sit at the texel of
    their level nearest +x, and are the figures the statement gives"""
    pr = ProbeRadiance(32, 2, (0.1, 0.25, 0.5, 1.0))
    T = api.probe_depth_dirs(32).reshape(-1, 3)
    hot = int(np.argmax(T[:, 0]))
    sums = np.zeros((1, 32, 32, 4), np.float32)
    sums[..., 3] = 1.0
    sums.reshape(-1, 4)[hot, 0:3] = 1000.0
    maps = api.probe_radiance_prefilter(pr, sums)
    peaks = [1000.0]
    for l in range(1, 4):
        o, R = pr.offsets[l], pr.resolutions[l]
        lv = maps[0, o:o + R * R, 0]
        Tl = api.probe_depth_dirs(R).reshape(-1, 3)
        nearest = np.flatnonzero(Tl[:, 0] >= Tl[:, 0].max() - 1e-12)
        assert int(np.argmax(lv)) in nearest, l
        assert np.array_equal(maps[0, o:o + R * R, 0], maps[0, o:o + R * R, 2])
        peaks.append(float(lv.max()))
    assert peaks[0] > peaks[1] > peaks[2] > peaks[3]
    assert abs(peaks[1] - 78.6) <= 0.05 and abs(peaks[2] - 6.53) <= 0.005 and abs(peaks[3] - 1.31) <= 0.005, peaks


def test_glossy_statement():
    """head-on view: r = -view, S = 0, F = f0; grazing: S -> 1, F -> 1; rho <= 0 and NaN take the diffuse input"""
    aov = np.zeros((4, 12), np.float32)
    aov[:, 0:3], aov[:, 3], aov[:, 4:7], aov[:, 8:11] = 0.5, 1.0, (0.0, 2.0, 0.0), (0.1, 0.2, 0.3)
    view = np.array([[0.0, -3.0, 0.0], [1.0, -1e-4, 0.0], [0.0, -1.0, 0.0], [0.0, -1.0, 0.0]], np.float32)
    spec = np.array([[0.9, 0.5, 0.1, 0.3], [0.9, 0.5, 0.1, 0.3], [0.9, 0.5, 0.1, 0.0], [0.9, 0.5, 0.1, NAN]], np.float32)
    r, S, ok = api.probe_glossy_dirs(aov, view)
    assert ok.all() and r[0].tolist() == [0.0, 1.0, 0.0] and S[0] == 0.0 and S[1] > 0.999
    diffuse = np.full((4, 3), 0.25, np.float32)
    rad = np.array([[2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0]], np.float32)
    out = api.probe_glossy_ref(aov, spec, view, diffuse, rad)
    assert out.dtype == np.float32 and np.array_equal(out[0], np.float32([0.9, 0.5, 0.1]) * np.float32(2.0))
    assert np.all(np.abs(out[1] - 2.0) <= 2e-3) and np.all(out[2:] == 0.25)
    neg = api.probe_glossy_ref(aov, spec, view, diffuse, -rad)
    assert np.all(neg[:2] == 0.0)                                                         # max(Ls, 0), full coverage: no albedo left


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _rad(resolution=8, sharpness_log2=2, levels=2, roughness=(0.1, 1.0, 0.0, 0.0)):
    d = A.fw_probe_radiance()
    d.resolution, d.sharpness_log2, d.levels = resolution, sharpness_log2, levels
    for l in range(4):
        d.roughness[l] = roughness[l]
    return d


BAD_RADIANCE = [("resolution", _rad(resolution=0)), ("resolution", _rad(resolution=12)), ("resolution", _rad(resolution=64)),
                ("sharpness_log2", _rad(sharpness_log2=9)), ("levels", _rad(levels=0)), ("levels", _rad(levels=3)), ("levels", _rad(levels=5)),
                ("levels", _rad(resolution=4, levels=2)), ("levels", _rad(resolution=32, levels=5)),
                ("roughness", _rad(roughness=(-0.1, 1.0, 0.0, 0.0))), ("roughness", _rad(roughness=(0.1, 1.5, 0.0, 0.0))),
                ("roughness", _rad(roughness=(NAN, 1.0, 0.0, 0.0))), ("roughness", _rad(roughness=(0.5, 0.5, 0.0, 0.0))),
                ("roughness", _rad(roughness=(0.5, 0.25, 0.0, 0.0)))]


def _depth(resolution=8, sharpness_log2=6, max_distance=10.0):
    d = A.fw_probe_depth()
    d.resolution, d.sharpness_log2, d.max_distance = resolution, sharpness_log2, max_distance
    return d


def _grid(lo=(0.0, 0.0, 0.0), hi=(1.0, 2.0, 3.0), counts=(2, 3, 2), flags=1):
    g = A.fw_probe_grid()
    for k in range(3):
        g.lo[k], g.hi[k], g.counts[k] = lo[k], hi[k], counts[k]
    g.flags = flags
    return g


BIG = (1 << 11, 1 << 10, 1 << 10)        # nx ny nz = 2^31
BAD_GRIDS = [("count", _grid(counts=(2, 0, 2))), ("finite", _grid(lo=(0.0, NAN, 0.0))), ("hi != lo", _grid(lo=(0.0, 2.0, 0.0))), ("flags", _grid(flags=2))]


def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def test_entries_not_read_past_levels_are_not_checked():
    lib = _lib.load()
    sums, maps = np.zeros((1, 8, 8, 4), np.float32), np.zeros((1, 80, 4), np.float32)
    st = lib.fw_probe_radiance_prefilter(0, C.byref(_rad(levels=1, roughness=(0.0, NAN, -5.0, 9.0))), 0, sums.ctypes.data, maps.ctypes.data, 0, None)
    assert _said(lib, st, "n_probes") == A.FW_ERR_BAD_ARG


def test_probe_radiance_reduce_argument_checks():
    lib = _lib.load()
    rays = np.zeros((2 * 5, 6), np.float32)
    accum = np.zeros((2 * 5, 4), np.float32)
    sums = np.full((2, 8, 8, 4), 7.0, np.float32)
    good = dict(rays=rays.ctypes.data, accum=accum.ctypes.data, sums=sums.ctypes.data)

    def call(pr=None, n=2, d=5, samples=1, device=0, on_device=0, null_pr=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_radiance_reduce(device, None if null_pr else C.byref(pr if pr is not None else _rad()), n, d, samples, a["rays"],
                                            a["accum"], a["sums"], on_device, None)

    assert _said(lib, call(null_pr=True), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, pr in BAD_RADIANCE:
        assert _said(lib, call(pr, n=0), word) == A.FW_ERR_BAD_ARG, word
    # the order inside the description, then n_probes, directions, samples, alignment, the two size limits, the device
    assert _said(lib, call(_rad(resolution=5, sharpness_log2=9, levels=0, roughness=(NAN,) * 4)), "resolution") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_rad(sharpness_log2=9, levels=0, roughness=(NAN,) * 4)), "sharpness_log2") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_rad(levels=3, roughness=(NAN,) * 4)), "levels") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=0, d=0), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(d=0, samples=0), "directions") == A.FW_ERR_BAD_ARG and _said(lib, call(d=(1 << 20) + 1), "directions") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(samples=0), "samples") == A.FW_ERR_BAD_ARG and _said(lib, call(samples=(1 << 24) + 1), "samples") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("accum", 4), ("accum", 8), ("rays", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(samples=0, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "samples") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=1 << 11, d=1 << 20, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=1 << 11, d=1 << 20), "directions must be below") == A.FW_ERR_UNSUPPORTED          # n D = 2^31
    assert _said(lib, call(_rad(resolution=32), n=1 << 21, d=1), "resolution^2") == A.FW_ERR_UNSUPPORTED       # n R^2 = 2^31
    assert _said(lib, call(n=1 << 11, d=1 << 20, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0)
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_probe_radiance_prefilter_argument_checks():
    lib = _lib.load()
    sums = np.full((2, 8, 8, 4), 7.0, np.float32)
    maps = np.full((2, 80, 4), 7.0, np.float32)
    good = dict(sums=sums.ctypes.data, maps=maps.ctypes.data)

    def call(pr=None, n=2, device=0, on_device=0, null_pr=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_radiance_prefilter(device, None if null_pr else C.byref(pr if pr is not None else _rad()), n, a["sums"], a["maps"],
                                               on_device, None)

    assert _said(lib, call(null_pr=True), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, pr in BAD_RADIANCE:
        assert _said(lib, call(pr, n=0), word) == A.FW_ERR_BAD_ARG, word
    assert _said(lib, call(n=0, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "n_probes") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("maps", 4), ("maps", 8)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    full = _rad(resolution=32, levels=4, roughness=(0.1, 0.25, 0.5, 1.0))                 # M = 1360
    assert _said(lib, call(full, n=(1 << 31) // 1360 + 1, on_device=1, maps=C.c_void_p(good["maps"] + 8)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(full, n=(1 << 31) // 1360 + 1, device=-1), "texels") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(maps == 7.0)
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_bake_probe_radiance_argument_checks():
    """every refusal comes before the scene is looked at, so a scene handle that is never dereferenced will do"""
    lib = _lib.load()
    pos = np.zeros((3, 3), np.float32)
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call
    buf = dict(sums=np.zeros((3, 8, 8, 4), np.float32), maps=np.zeros((3, 80, 4), np.float32), sh_sums=np.zeros((3, 9, 3), np.float32),
               sh=np.zeros((3, 9, 3), np.float32))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def pset(n=3, d=65, positions=pos):
        s = A.fw_probe_set()
        s.n_probes, s.directions, s.jitter, s.seed, s.chunk_probes = n, d, 1, 0, 0
        s.positions = None if positions is None else positions.ctypes.data_as(C.POINTER(C.c_float))
        return s

    def call(s=None, pr=None, first=0, rounds=1, samples=1, on_device=0, null=None, **ptrs):
        a = dict(good, **ptrs)
        rp = A.fw_render_rays_params()
        rp.samples, rp.use_bvh, rp.on_device, rp.gamma = samples, 1, on_device, 1.0
        args = dict(scene=scene, s=C.byref(s if s is not None else pset()), pr=C.byref(pr if pr is not None else _rad()), rp=C.byref(rp))
        if null:
            args[null] = None
        return lib.fw_bake_probe_radiance(args["scene"], args["s"], args["pr"], args["rp"], first, rounds, a["sums"], a["maps"], a["sh_sums"], a["sh"],
                                          None)

    for null in ("scene", "s", "pr", "rp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    assert _said(lib, call(pset(positions=None)), "null positions") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(n=0)), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(d=0)), "directions") == A.FW_ERR_BAD_ARG
    bad = pos.copy()
    bad[1, 2] = NAN
    assert _said(lib, call(pset(positions=bad), _rad(resolution=5)), "probe 1") == A.FW_ERR_BAD_ARG               # the set before the description
    for word, pr in BAD_RADIANCE:
        assert _said(lib, call(pr=pr, rounds=0), word) == A.FW_ERR_BAD_ARG, word                                   # the description before the rounds
    assert _said(lib, call(rounds=0, samples=0), "rounds") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1, samples=0), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(samples=0, first=2, sums=None), "samples") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=2, sums=None, sh_sums=None), "needs the sums") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=2, sh_sums=None), "needs the sh_sums") == A.FW_ERR_BAD_ARG                       # sh is asked for
    assert _said(lib, call(first=2, sh_sums=None, sh=None, on_device=1, maps=C.c_void_p(good["maps"] + 8)), "aligned") == A.FW_ERR_BAD_ARG   # SH not in use
    for name, off in (("sums", 8), ("maps", 4), ("sh_sums", 2), ("sh", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, name
    big = np.zeros(((1 << 11), 3), np.float32)
    assert _said(lib, call(pset(n=1 << 11, d=1 << 20, positions=big), rounds=0), "rounds") == A.FW_ERR_BAD_ARG   # bad arguments before the size
    assert _said(lib, call(pset(n=1 << 11, d=1 << 20, positions=big)), "directions must be below") == A.FW_ERR_UNSUPPORTED
    wide = np.zeros(((1 << 21), 3), np.float32)
    full = _rad(resolution=32, levels=4, roughness=(0.1, 0.25, 0.5, 1.0))
    assert _said(lib, call(pset(n=1 << 21, d=1, positions=wide), full), "texels") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(sums=None, maps=None, sh_sums=None, sh=None) == A.FW_ERR_NO_DEVICE


def test_probe_radiance_lookup_argument_checks():
    lib = _lib.load()
    buf = dict(maps=np.full((12, 80, 4), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32), pl=np.full((12, 4), 7.0, np.float32),
               pos=np.full((5, 3), 7.0, np.float32), nrm=np.full((5, 3), 7.0, np.float32), dirs=np.full((5, 3), 7.0, np.float32),
               rough=np.full((5,), 7.0, np.float32), out=np.full((5, 3), 7.0, np.float32))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(g=None, pr=None, pd=None, bias=0.0, device=0, n=5, stride=3, on_device=0, null=None, **ptrs):
        a = dict(good, **ptrs)
        gp = None if null == "grid" else C.byref(g if g is not None else _grid())
        rp = None if null == "pr" else C.byref(pr if pr is not None else _rad())
        pp = None if null == "pd" else C.byref(pd if pd is not None else _depth())
        return lib.fw_probe_radiance_lookup(gp, rp, a["maps"], pp, a["mom"], bias, a["pl"], device, n, a["pos"], a["nrm"], stride, a["dirs"],
                                            a["rough"], a["out"], on_device, None)

    for null in ("grid", "pr"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("maps", "pos", "nrm", "dirs", "rough", "out"):
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(null="pd"), "null") == A.FW_ERR_BAD_ARG and _said(lib, call(mom=None), "null") == A.FW_ERR_BAD_ARG   # exactly one of the two
    for word, pr in BAD_RADIANCE:
        assert _said(lib, call(pr=pr, pd=_depth(resolution=5)), word) == A.FW_ERR_BAD_ARG, word                    # pr before pd
    assert _said(lib, call(pd=_depth(resolution=5), bias=-1.0), "resolution") == A.FW_ERR_BAD_ARG
    for bias in (-0.5, NAN, INF):
        assert _said(lib, call(_grid(flags=2), bias=bias), "normal_bias") == A.FW_ERR_BAD_ARG, bias                 # the bias before the grid
    for word, g in BAD_GRIDS:
        assert _said(lib, call(g, n=0), word) == A.FW_ERR_BAD_ARG, word                                             # the grid before n
    assert _said(lib, call(n=0, stride=0), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, device=-1), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(device=-1), "device") == A.FW_ERR_BAD_ARG
    for name in ("mom", "pl", "pos", "nrm", "dirs", "rough", "out"):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + 2)}), "aligned") == A.FW_ERR_BAD_ARG, name
    for off in (4, 8):
        assert _said(lib, call(on_device=1, maps=C.c_void_p(good["maps"] + off)), "aligned") == A.FW_ERR_BAD_ARG, off
    assert _said(lib, call(_grid(counts=BIG), stride=2), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_grid(counts=BIG)), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_grid(counts=(1 << 7, 1 << 7, 1 << 7)), pd=_depth(resolution=32)), "resolution^2") == A.FW_ERR_UNSUPPORTED
    full = _rad(resolution=32, levels=4, roughness=(0.1, 0.25, 0.5, 1.0))
    assert _said(lib, call(_grid(counts=(1 << 7, 1 << 7, 1 << 7)), pr=full, pd=_depth(resolution=4)), "texels") == A.FW_ERR_UNSUPPORTED   # 2^21 x 1360
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert call(null="pd", mom=None, pl=None) == A.FW_ERR_NO_DEVICE                                             # all three are optional
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG


def test_probe_shade_glossy_argument_checks():
    lib = _lib.load()
    buf = dict(sh=np.full((12, 9, 3), 7.0, np.float32), maps=np.full((12, 80, 4), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32),
               pl=np.full((12, 4), 7.0, np.float32), aov=np.full((6, 12), 7.0, np.float32), spec=np.full((6, 4), 7.0, np.float32),
               view=np.full((6, 3), 7.0, np.float32), lin=np.full((6, 3), 7.0, np.float32), gam=np.full((6, 3), 7.0, np.float32),
               rgb8=np.full((6, 3), 7, np.uint8))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def params(**kw):
        p = A.fw_probe_shade_params()
        p.width, p.height, p.gamma = 3, 2, 2.2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(g=None, pr=None, pd=None, bias=0.0, p=None, vstride=3, null=None, **ptrs):
        a = dict(good, **ptrs)
        gp = None if null == "grid" else C.byref(g if g is not None else _grid())
        rp = None if null == "pr" else C.byref(pr if pr is not None else _rad())
        dp = None if null == "pd" else C.byref(pd if pd is not None else _depth())
        pp = None if null == "p" else C.byref(p if p is not None else params())
        return lib.fw_probe_shade_glossy(gp, a["sh"], rp, a["maps"], dp, a["mom"], bias, a["pl"], pp, a["aov"], a["spec"], a["view"], vstride,
                                         a["lin"], a["gam"], a["rgb8"])

    for null in ("grid", "pr", "pd", "p"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("sh", "maps", "mom", "aov", "spec", "view"):
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(pr=_rad(resolution=5), lin=None, gam=None, rgb8=None), "output") == A.FW_ERR_BAD_ARG     # the outputs first
    for word, pr in BAD_RADIANCE:
        assert _said(lib, call(pr=pr, pd=_depth(resolution=5)), word) == A.FW_ERR_BAD_ARG, word
    assert _said(lib, call(pd=_depth(resolution=5), bias=-1.0), "resolution") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_grid(flags=2), bias=-0.5), "normal_bias") == A.FW_ERR_BAD_ARG
    for word, g in BAD_GRIDS:
        assert _said(lib, call(g, p=params(width=0)), word) == A.FW_ERR_BAD_ARG, word
    assert _said(lib, call(p=params(width=0, gamma=0.0)), "width") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(gamma=NAN, device=-1), vstride=2), "gamma") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(device=-1), vstride=2), "view_stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(device=-1)), "device") == A.FW_ERR_BAD_ARG
    for name, off in (("aov", 8), ("spec", 4), ("maps", 8), ("sh", 2), ("view", 2), ("lin", 2), ("gam", 2), ("mom", 2), ("pl", 2)):
        assert _said(lib, call(p=params(on_device=1), **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(_grid(counts=BIG)), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(p=params(width=0x10000, height=0x10000)), "image too large") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(null="pd", mom=None, pl=None) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7) for v in buf.values())
    else:
        assert call(p=params(device=_lib.device_count())) == A.FW_ERR_BAD_ARG


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("needs a machine without a GPU")
    grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))
    pr = ProbeRadiance(8)
    maps = np.ones((2, pr.texels, 4), np.float32)
    one = np.ones((1, 3), np.float32)
    calls = [lambda: _lib.probe_radiance_reduce(pr, np.zeros((2, 6), np.float32), np.zeros((2, 4), np.float32), 1, 1),
             lambda: _lib.probe_radiance_prefilter(pr, np.zeros((2, 8, 8, 4), np.float32)),
             lambda: _lib.probe_radiance_lookup(grid, pr, maps, one, one, one, np.ones(1, np.float32)),
             lambda: _lib.probe_shade_glossy(grid, np.zeros((2, 9, 3), np.float32), pr, maps, np.zeros((1, 12), np.float32), np.zeros((1, 4), np.float32),
                                             one, 1, 1)]
    for fn in calls:
        with pytest.raises(_lib.FireworkError) as e:
            fn()
        assert e.value.status == A.FW_ERR_NO_DEVICE
