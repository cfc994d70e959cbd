"""CPU-side checks of probe relocation and classification (fw_probe_survey, fw_probe_relocate_step, fw_relocate_probes,
fw_probe_irradiance_placed, fw_probe_shade_placed): the exports and the struct's layout at ABI 8; the numpy statements on
closed forms (a probe inside a sphere, above and below a floor, in open space; a rejected move); the placed lookup against probe_lookup
and probe_lookup_vis; every argument error of the five calls in the header's order (they come before HIP is called); and the command
line's refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import probe_place_ref as REF
from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import ProbeDepth, ProbeGrid, ProbeRelocation, ProbeSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
MISS = np.uint32(0xFFFFFFFF)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.PROBE_PLACE_PROTOTYPES) == ["fw_probe_irradiance_placed", "fw_probe_relocate_step", "fw_probe_shade_placed", "fw_probe_survey",
                                                "fw_relocate_probes"]
    for name in A.PROBE_PLACE_PROTOTYPES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name
    for name in ("probe_survey", "probe_relocate_step", "probe_irradiance_placed", "probe_shade_placed"):
        assert callable(getattr(_lib, name)), name
    assert callable(_lib.DeviceScene.relocate_probes) and callable(api.Renderer.relocate_probes)


def test_struct_layout(tmp_path):
    """ctypes' fw_probe_relocate equals the C compiler's, size and every field offset"""
    names = ["min_front", "back_fraction", "max_offset"]
    assert [f for f, _ in A.fw_probe_relocate._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(fw_probe_relocate)' +
           "".join(f",offsetof(fw_probe_relocate,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_probe_relocate)] + [getattr(A.fw_probe_relocate, f).offset for f in names]
    assert C.sizeof(A.fw_probe_relocate) == 20


# ---- the statements on closed forms ---------------------------------------------------------------------------------------------------
D_SET = (63, 64, 65, 200)
ROUNDS = (0, 1, 2, 3)


def _one_probe(position, D, round_, hits, seed=7):
    """(rays, t, normal, object) of one probe at `position`: the set's own rays of `round_`, and the hits `hits` reports for them"""
    probes = ProbeSet([position], D).seed(seed)
    rays = probes.rays(round_)
    return (rays,) + tuple(hits(rays))


def _stepped(position, D, round_, hits, rl, placement=None):
    """one survey at position + offset and one moving step: (survey float64, placement after the step)"""
    pl = api.neutral_placement(1) if placement is None else placement
    rays, t, nrm, obj = _one_probe(np.asarray(position, np.float32) + pl[0, 0:3], D, round_, hits)
    assert REF.survey_gap(rays, t, nrm, obj, D) > REF.argmin_gap
    sv = api.probe_survey(rays, t, nrm, obj, D)
    return sv, api.probe_relocate_step(rl, sv.astype(np.float32), pl, D)


@pytest.mark.parametrize("D", D_SET)
def test_probe_inside_a_sphere_is_pushed_out(D):
    """Inside a closed sphere every ray meets a back face: n_back = D.  The nearest of D lattice directions is within 6e-3 of the true
    1 - |e|, and one step along it by dist + min_front / 2 leaves the probe outside by at most that half."""
    e = np.array([0.3, 0.2, -0.1], np.float32)
    rl = ProbeRelocation(0.25, max_offset=(2.0, 2.0, 2.0))
    for r in ROUNDS:
        sv, pl = _stepped(e, D, r, REF.sphere_hits, rl)
        assert sv[0, 2].tolist() == [float(D), 0.0, 0.0, 0.0]
        true = 1.0 - float(np.linalg.norm(e.astype(np.float64)))
        assert 0.0 <= sv[0, 0, 3] - true <= 6e-3 and abs(true - 0.6258) < 1e-4
        assert sv[0, 1].tolist() == [0.0, 0.0, 0.0, INF]
        where = np.linalg.norm(e.astype(np.float64) + pl[0, 0:3].astype(np.float64))
        assert 1.0 < where <= 1.125 and pl[0, 3] == 0.0                          # moved; classified where the survey was taken: inside


@pytest.mark.parametrize("D", D_SET)
def test_probe_above_a_floor_is_lifted(D):
    rl = ProbeRelocation(0.25, max_offset=(1.0, 1.0, 1.0))
    for r in ROUNDS:
        sv, pl = _stepped((0.0, 0.1, 0.0), D, r, REF.floor_hits, rl)
        assert sv[0, 2, 0] == 0.0 and sv[0, 2, 1] > 0.0 and sv[0, 2, 1] + sv[0, 2, 2] == D      # only front hits, and misses above
        height = 0.1 + float(pl[0, 1])
        assert 0.24 <= height <= 0.25 and pl[0, 3] == 1.0, height


@pytest.mark.parametrize("D", D_SET)
def test_probe_below_a_floor_is_brought_up(D):
    rl = ProbeRelocation(0.25, max_offset=(1.0, 1.0, 1.0))
    for r in ROUNDS:
        sv, pl = _stepped((0.0, -0.1, 0.0), D, r, REF.floor_hits, rl)
        assert sv[0, 2, 0] >= 31.0 * D / 63.0 and sv[0, 2, 0] > D / 4.0 and sv[0, 2, 1] == 0.0
        y = -0.1 + float(pl[0, 1])
        assert 0.12 <= y <= 0.125 and pl[0, 3] == 0.0, y
    # the next survey, taken from where it went, classifies it active, and it stays (already min_front / 2 above: it is lifted further)
    sv2, pl2 = _stepped((0.0, -0.1, 0.0), D, 1, REF.floor_hits, rl, pl)
    assert sv2[0, 2, 0] == 0.0 and pl2[0, 3] == 1.0 and 0.24 <= -0.1 + float(pl2[0, 1]) <= 0.25


def test_open_space_keeps_the_neutral_record():
    rl = ProbeRelocation(0.25, max_offset=(1.0, 1.0, 1.0))
    for D in D_SET:
        rays, t, nrm, obj = _one_probe((0.5, 0.5, 0.5), D, 0, REF.no_hits)
        sv = api.probe_survey(rays, t, nrm, obj, D)
        assert sv[0, 2].tolist() == [0.0, 0.0, float(D), 0.0] and sv[0, 0].tolist() == sv[0, 1].tolist() == [0.0, 0.0, 0.0, INF]
        for move in (True, False):
            pl = api.probe_relocate_step(rl, sv, api.neutral_placement(1), D, move)
            assert np.array_equal(_u32(pl), _u32(api.neutral_placement(1)))


def test_a_rejected_move_stays_and_ends_inactive():
    """max_offset 0.3 < the 0.75 the sphere asks for: the offset is kept, bit for bit, and the classifying step marks the probe inactive"""
    e = np.array([0.3, 0.2, -0.1], np.float32)
    rl = ProbeRelocation(0.25, max_offset=0.3)
    start = np.array([[0.0625, -0.03125, 0.0, 1.0]], np.float32)
    sv, pl = _stepped(e, 65, 0, REF.sphere_hits, rl, start)
    assert np.array_equal(_u32(pl[:, 0:3]), _u32(start[:, 0:3])) and pl[0, 3] == 0.0
    cls = api.probe_relocate_step(rl, sv, start, 65, move=False)
    assert np.array_equal(_u32(cls[:, 0:3]), _u32(start[:, 0:3])) and cls[0, 3] == 0.0
    # rejected, not clamped: one axis over its limit is enough
    one = api.probe_relocate_step(ProbeRelocation(0.25, max_offset=(2.0, 2.0, 1e-3)), sv, start, 65)
    assert np.array_equal(_u32(one[:, 0:3]), _u32(start[:, 0:3]))


def test_survey_statement_details():
    """zero rays count nowhere; ties go to the lowest j; the class follows the stored normal; a medium's +Y normal counts as what it is"""
    rays = np.zeros((6, 6), np.float32)
    rays[:, 3:] = [(0, 2, 0), (0, 0, 0), (0, -1, 0), (0, 1, 0), (1, 0, 0), (0, -0.5, 0)]
    t = np.array([1.0, 5.0, 3.0, 2.0, 9.0, 4.0], np.float32)             # distances 2, -, 3, 2, miss, 2
    nrm = np.zeros((6, 3), np.float32)
    nrm[:, 1] = 1.0                                                          # +Y everywhere: rays going up are back hits, going down front
    obj = np.array([0, 0, 0, 0, MISS, 0], np.uint32)
    sv, J = api.probe_survey(rays, t, nrm, obj, 6, terms=True)
    assert sv[0, 2].tolist() == [2.0, 2.0, 1.0, 0.0]
    assert J[0].tolist() == [0, 5] and sv[0, 0].tolist() == [0.0, 2.0, 0.0, 2.0] and sv[0, 1].tolist() == [0.0, -0.5, 0.0, 2.0]


def test_probe_relocation_defaults_and_moved_set():
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (4.0, 0.0, 1.0), (3, 1, 2), 16).seed(5)
    rl = ProbeRelocation(0.1).resolved(probes)
    assert rl.back_fraction == 0.25 and rl.steps == 4
    assert np.allclose(rl.max_offset, (0.45 * 2.0, 0.45 * 1.0, 0.45 * 1.0))                # the flat axis takes the smallest spacing
    with pytest.raises(ValueError):
        ProbeRelocation(0.1).resolved()
    pl = api.neutral_placement(6)
    pl[2] = (0.25, -0.5, 0.125, 0.0)
    moved = probes.moved(pl)
    assert moved.grid_counts == probes.grid_counts and moved.grid_lo == probes.grid_lo and moved._seed == 5 and moved.directions == 16
    assert np.array_equal(moved.positions[2], probes.positions[2] + pl[2, 0:3]) and np.array_equal(np.delete(moved.positions, 2, 0), np.delete(probes.positions, 2, 0))
    abi = ProbeRelocation(0.1, 0.5, (1.0, 2.0, 3.0)).to_abi()
    assert (abi.min_front, abi.back_fraction, list(abi.max_offset)) == (np.float32(0.1), 0.5, [1.0, 2.0, 3.0])


# ---- the placed lookup ----------------------------------------------------------------------------------------------------------------
def _points(n, rng, lo, hi):
    pts = (np.asarray(lo) + rng.uniform(-0.2, 1.2, size=(n, 3)) * (np.asarray(hi) - np.asarray(lo))).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]).astype(np.float32)
    return pts, nrm


def _case(wrap, seed=3):
    rng = np.random.default_rng(seed)
    grid = ProbeGrid((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5), wrap)
    sh = rng.normal(size=(60, 9, 3)).astype(np.float32)
    pd = ProbeDepth(8, 6, 100.0)
    moments = np.empty((60, 8, 8, 2), np.float32)
    moments[..., 0] = rng.uniform(0.3, 3.0, size=(60, 8, 8))
    moments[..., 1] = moments[..., 0] ** 2 * rng.uniform(1.0, 1.5, size=(60, 8, 8))
    pts, nrm = _points(200, rng, grid.lo, grid.hi)
    pts[7], nrm[11] = (NAN, 0.0, 0.0), (0.0, 0.0, 0.0)                       # two points the statement answers with zeros
    return rng, grid, sh, pd, moments, pts, nrm


def test_neutral_placement_equals_the_counterparts():
    for wrap in (True, False):
        _rng, grid, sh, pd, moments, pts, nrm = _case(wrap)
        neutral = api.neutral_placement(60)
        ref, Tref = api.probe_lookup(grid, sh, pts, nrm, terms=True)
        E, T, X = api.probe_lookup_placed(grid, sh, neutral, pts, nrm, terms=True)
        assert np.all(X["active"])
        if wrap:
            assert np.array_equal(_u64(E), _u64(ref)) and np.array_equal(_u64(T), _u64(Tref))
        else:
            assert np.all(np.abs(E - ref) <= 16 * 2.0 ** -53 * Tref)      # the division of (iii) alone: weights that sum to 1 to a few ulps
        vis = api.probe_lookup_vis(grid, sh, pd, moments, pts, nrm, 0.125)
        placed = api.probe_lookup_placed(grid, sh, neutral, pts, nrm, pd, moments, 0.125)
        assert np.array_equal(_u64(placed), _u64(vis))
        assert np.all(placed[7] == 0.0) and np.all(placed[11] == 0.0)


def test_inactive_probes_never_reach_the_output():
    for wrap in (True, False):
        rng, grid, sh, pd, moments, pts, nrm = _case(wrap, 5)
        pl = api.neutral_placement(60)
        off = rng.random(60) < 0.25
        pl[off, 3] = 0.0
        pl[:, 0:3] = rng.uniform(-0.2, 0.2, size=(60, 3))
        bad_sh, bad_mom = sh.copy(), moments.copy()
        bad_sh[off], bad_mom[off] = NAN, NAN
        for vis in ((), (pd, moments, 0.0625)):
            clean = api.probe_lookup_placed(grid, sh, pl, pts, nrm, *vis)
            dirty = api.probe_lookup_placed(grid, bad_sh, pl, pts, nrm, *((pd, bad_mom, 0.0625) if vis else ()))
            assert np.all(np.isfinite(dirty)) and np.array_equal(_u64(clean), _u64(dirty))
        none = pl.copy()
        none[:, 3] = 0.0
        assert np.all(api.probe_lookup_placed(grid, bad_sh, none, pts, nrm) == 0.0)
        assert np.all(api.probe_lookup_placed(grid, bad_sh, none, pts, nrm, pd, bad_mom) == 0.0)


def test_a_single_active_corner_gives_that_probe_alone():
    """one active corner: its weight cancels in the normalisation, and the answer is that probe's own irradiance for the normal — the
    1 x 1 x 1 lookup of its coefficients, bit for bit"""
    rng, grid, sh, pd, moments, _pts, _nrm = _case(True, 9)
    pts = np.array([[0.1, 0.9, 3.3], [1.2, 0.4, 5.9]], np.float32)            # strictly inside cells
    nrm = np.array([[0.0, 1.0, 0.2], [0.3, -1.0, 0.5]], np.float32)
    for probe in (0 + 4 * (0 + 3 * 1) + 1, 2 + 4 * (1 + 3 * 3)):               # a corner of the first point's cell, one of the second's
        pl = api.neutral_placement(60)
        pl[:, 3] = 0.0
        pl[probe] = (0.05, -0.1, 0.2, 1.0)
        own = api.probe_lookup(ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), False), sh[probe:probe + 1], pts, nrm)
        for vis in ((), (pd, moments, 0.0)):
            E, _T, X = api.probe_lookup_placed(grid, sh, pl, pts, nrm, *vis, terms=True)
            hit = X["active"].any(axis=1)
            assert hit.sum() == 1 and np.all(X["w"][hit].sum(axis=1) == 1.0)
            assert np.array_equal(_u64(E[hit]), _u64(own[hit])) and np.all(E[~hit] == 0.0)


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def _relocate(min_front=0.25, back_fraction=0.25, max_offset=(1.0, 1.0, 1.0)):
    r = A.fw_probe_relocate()
    r.min_front, r.back_fraction = min_front, back_fraction
    for k in range(3):
        r.max_offset[k] = max_offset[k]
    return r


BAD_RELOCATIONS = [("min_front", _relocate(min_front=0.0)), ("min_front", _relocate(min_front=-1.0)), ("min_front", _relocate(min_front=INF)),
                   ("min_front", _relocate(min_front=NAN)), ("back_fraction", _relocate(back_fraction=-0.1)),
                   ("back_fraction", _relocate(back_fraction=1.5)), ("back_fraction", _relocate(back_fraction=NAN)),
                   ("max_offset", _relocate(max_offset=(1.0, -1.0, 1.0))), ("max_offset", _relocate(max_offset=(1.0, 1.0, INF))),
                   ("max_offset", _relocate(max_offset=(NAN, 1.0, 1.0)))]


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


def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def test_probe_survey_argument_checks():
    lib = _lib.load()
    rays = np.zeros((2 * 5, 6), np.float32)
    rays[:, 4] = 1.0
    hits = np.zeros(2 * 5, _lib.HIT_DTYPE)
    survey = np.full((2, 3, 4), 7.0, np.float32)
    good = dict(rays=rays.ctypes.data, hits=hits.ctypes.data, survey=survey.ctypes.data)

    def call(n=2, d=5, device=0, on_device=0, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_survey(device, n, d, a["rays"], a["hits"], a["survey"], on_device, None)

    for name in good:
        assert _said(lib, call(n=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(n=0, d=0), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(d=0), "directions") == A.FW_ERR_BAD_ARG and _said(lib, call(d=(1 << 20) + 1), "directions") == A.FW_ERR_BAD_ARG
    for name, off in (("survey", 4), ("survey", 8), ("hits", 4), ("hits", 8), ("rays", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(n=1 << 11, d=1 << 20, on_device=1, survey=C.c_void_p(good["survey"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=1 << 11, d=1 << 20), "directions must be below") == A.FW_ERR_UNSUPPORTED          # n D = 2^31
    assert _said(lib, call(n=1 << 11, d=1 << 20, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(survey == 7.0)
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_probe_relocate_step_argument_checks():
    lib = _lib.load()
    survey = np.full((2, 3, 4), 7.0, np.float32)
    placement = np.full((2, 4), 7.0, np.float32)
    good = dict(survey=survey.ctypes.data, placement=placement.ctypes.data)

    def call(rl=None, n=2, d=5, device=0, on_device=0, move=1, null_rl=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_relocate_step(device, None if null_rl else C.byref(rl if rl is not None else _relocate()), n, d, a["survey"],
                                          a["placement"], move, on_device, None)

    assert _said(lib, call(null_rl=True), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(_relocate(min_front=0.0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, rl in BAD_RELOCATIONS:
        assert _said(lib, call(rl, n=0), word) == A.FW_ERR_BAD_ARG, word                                              # the relocation before n
    assert _said(lib, call(_relocate(min_front=0.0, back_fraction=2.0, max_offset=(-1.0, 0.0, 0.0))), "min_front") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_relocate(back_fraction=2.0, max_offset=(-1.0, 0.0, 0.0))), "back_fraction") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=0, d=0), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(d=0), "directions") == A.FW_ERR_BAD_ARG and _said(lib, call(d=(1 << 20) + 1), "directions") == A.FW_ERR_BAD_ARG
    for name in good:
        for off in (4, 8):
            assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, device=-1, survey=C.c_void_p(good["survey"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    for ok in (_relocate(back_fraction=0.0), _relocate(back_fraction=1.0), _relocate(max_offset=(0.0, 0.0, 0.0))):      # the closed ends
        st = call(ok)
        assert st == (A.FW_ERR_NO_DEVICE if _lib.device_count() == 0 else A.FW_OK)
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(survey == 7.0) and np.all(placement == 7.0)
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_relocate_probes_argument_checks():
    """every refusal comes before the scene is looked at, so a scene handle that is never dereferenced will do"""
    lib = _lib.load()
    pos = np.zeros((3, 3), np.float32)
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call
    placement = api.neutral_placement(3)
    survey = np.full((3, 3, 4), 7.0, np.float32)

    def pset(n=3, d=65, positions=pos):
        s = A.fw_probe_set()
        s.n_probes, s.directions, s.jitter, s.seed, s.chunk_probes = n, d, 1, 0, 0
        s.positions = None if positions is None else positions.ctypes.data_as(C.POINTER(C.c_float))
        return s

    def call(s=None, rl=None, first=0, steps=1, null=None, pl=placement, sv=survey.ctypes.data):
        tp = A.fw_trace_params()
        tp.use_bvh = 1
        args = dict(scene=scene, s=C.byref(s if s is not None else pset()), rl=C.byref(rl if rl is not None else _relocate()), tp=C.byref(tp),
                    pl=pl.ctypes.data)
        if null:
            args[null] = None
        return lib.fw_relocate_probes(args["scene"], args["s"], args["rl"], args["tp"], first, steps, args["pl"], sv, None)

    for null in ("scene", "s", "rl", "tp", "pl"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    assert _said(lib, call(pset(positions=None)), "null positions") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(n=0)), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(d=0)), "directions") == A.FW_ERR_BAD_ARG
    bad = pos.copy()
    bad[1, 2] = NAN
    assert _said(lib, call(pset(positions=bad), _relocate(min_front=0.0)), "probe 1") == A.FW_ERR_BAD_ARG       # the set before the relocation
    bad_pl = placement.copy()
    bad_pl[2, 3] = 0.5
    for word, rl in BAD_RELOCATIONS:
        assert _said(lib, call(rl=rl, pl=bad_pl), word) == A.FW_ERR_BAD_ARG, word                                # the relocation before the placement
    assert _said(lib, call(pl=bad_pl, first=0xFFFFFFFF), "placement 2") == A.FW_ERR_BAD_ARG                     # the placement before the steps
    for entry in ((NAN, 0, 0, 1), (0, INF, 0, 1), (0, 0, -INF, 0), (0, 0, 0, NAN), (0, 0, 0, 2), (0, 0, 0, -1)):
        one = placement.copy()
        one[1] = entry
        assert _said(lib, call(pl=one), "placement 1") == A.FW_ERR_BAD_ARG, entry
    assert _said(lib, call(first=0xFFFFFFFF, steps=0), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFF0, steps=15), "overflows") == A.FW_ERR_BAD_ARG
    big = np.zeros(((1 << 11), 3), np.float32)
    big_pl = api.neutral_placement(1 << 11)
    assert _said(lib, call(pset(n=1 << 11, d=1 << 20, positions=big), pl=big_pl, first=0xFFFFFFFF), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(n=1 << 11, d=1 << 20, positions=big), pl=big_pl), "directions must be below") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(steps=0, sv=None) == A.FW_ERR_NO_DEVICE
        assert np.array_equal(placement, api.neutral_placement(3)) and np.all(survey == 7.0)


BIG = (1 << 11, 1 << 10, 1 << 10)        # nx ny nz = 2^31 (no array is read: the count comes first)
BAD_GRIDS = [("count", _grid(counts=(2, 0, 2))), ("finite", _grid(lo=(0.0, NAN, 0.0))), ("hi != lo", _grid(lo=(0.0, 2.0, 0.0))), ("flags", _grid(flags=2))]
BAD_DEPTHS = [("resolution", _depth(resolution=12)), ("sharpness_log2", _depth(sharpness_log2=9)), ("max_distance", _depth(max_distance=NAN))]
BAD_BIAS = [-0.5, NAN, INF]


def test_probe_irradiance_placed_argument_checks():
    lib = _lib.load()
    buf = dict(sh=np.full((12, 9, 3), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32), pl=np.full((12, 4), 7.0, np.float32),
               pos=np.full((5, 3), 7.0, np.float32), nrm=np.full((5, 3), 7.0, np.float32), out=np.full((5, 3), 7.0, np.float32))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(g=None, pd=None, bias=0.0, device=0, n=5, stride=3, on_device=0, null=None, **ptrs):
        a = dict(good, **ptrs)
        gp = None if null == "grid" else C.byref(g if g is not None else _grid())
        pp = None if null == "pd" else C.byref(pd if pd is not None else _depth())
        return lib.fw_probe_irradiance_placed(gp, a["sh"], pp, a["mom"], bias, a["pl"], device, n, a["pos"], a["nrm"], stride, a["out"], on_device, None)

    assert _said(lib, call(null="grid"), "null") == A.FW_ERR_BAD_ARG
    for name in ("sh", "pl", "pos", "nrm", "out"):
        assert _said(lib, call(n=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(null="pd"), "null") == A.FW_ERR_BAD_ARG and _said(lib, call(mom=None), "null") == A.FW_ERR_BAD_ARG   # one of the two
    for word, pd in BAD_DEPTHS:
        assert _said(lib, call(pd=pd, bias=-1.0), word) == A.FW_ERR_BAD_ARG, word
    for bias in BAD_BIAS:
        assert _said(lib, call(_grid(flags=2), bias=bias), "normal_bias") == A.FW_ERR_BAD_ARG, bias
    for null_vis in (False, True):                        # with depth maps, and with pd and moments both NULL (the bias is then not read)
        kw = dict(null="pd", mom=None, bias=NAN) if null_vis else {}
        for word, g in BAD_GRIDS:
            assert _said(lib, call(g, n=0, **kw), word) == A.FW_ERR_BAD_ARG, word
        assert _said(lib, call(n=0, stride=0, **kw), "n must") == A.FW_ERR_BAD_ARG
        assert _said(lib, call(stride=2, device=-1, **kw), "stride") == A.FW_ERR_BAD_ARG
        assert _said(lib, call(device=-1, **kw), "device") == A.FW_ERR_BAD_ARG
        for name in ("sh", "pl", "pos", "nrm", "out") + (() if null_vis else ("mom",)):
            assert _said(lib, call(on_device=1, **dict(kw, **{name: C.c_void_p(good[name] + 2)})), "aligned") == A.FW_ERR_BAD_ARG, name
        assert _said(lib, call(_grid(counts=BIG), **kw), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
        if _lib.device_count() == 0:
            assert call(**kw) == A.FW_ERR_NO_DEVICE and call(device=5, **kw) == A.FW_ERR_NO_DEVICE
        else:
            assert call(device=_lib.device_count(), **kw) == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_grid(counts=(1 << 7, 1 << 7, 1 << 7)), _depth(resolution=32)), "resolution^2") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert all(np.all(v == 7.0) for v in buf.values())


def test_probe_shade_placed_argument_checks():
    lib = _lib.load()
    buf = dict(sh=np.full((12, 9, 3), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32), pl=np.full((12, 4), 7.0, np.float32),
               aov=np.full((6, 12), 7.0, np.float32), lin=np.full((6, 3), 7.0, np.float32), gam=np.full((6, 3), 7.0, np.float32),
               rgb8=np.full((6, 3), 7, np.uint8))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def params(**kw):
        p = A.fw_probe_shade_params()
        p.width, p.height, p.gamma = 3, 2, 2.2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(g=None, pd=None, bias=0.0, p=None, null=(), **ptrs):
        a = dict(good, **ptrs)
        gp = None if "grid" in null else C.byref(g if g is not None else _grid())
        dp = None if "pd" in null else C.byref(pd if pd is not None else _depth())
        pp = None if "p" in null else C.byref(p if p is not None else params())
        return lib.fw_probe_shade_placed(gp, a["sh"], dp, a["mom"], bias, a["pl"], pp, a["aov"], a["lin"], a["gam"], a["rgb8"])

    for null in ("grid", "pd", "p"):
        assert _said(lib, call(null=(null,)), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("sh", "mom", "pl", "aov"):
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(pd=_depth(resolution=5), lin=None, gam=None, rgb8=None), "output") == A.FW_ERR_BAD_ARG   # the outputs first
    for word, pd in BAD_DEPTHS:
        assert _said(lib, call(pd=pd, bias=-1.0), word) == A.FW_ERR_BAD_ARG, word
    for bias in BAD_BIAS:
        assert _said(lib, call(_grid(flags=2), bias=bias), "normal_bias") == A.FW_ERR_BAD_ARG, bias
    for kw in ({}, dict(null=("pd",), mom=None, bias=NAN)):
        for word, g in BAD_GRIDS:
            assert _said(lib, call(g, p=params(width=0), **kw), word) == A.FW_ERR_BAD_ARG, word
        assert _said(lib, call(p=params(width=0, gamma=0.0), **kw), "width") == A.FW_ERR_BAD_ARG
        assert _said(lib, call(p=params(gamma=NAN, device=-1), **kw), "gamma") == A.FW_ERR_BAD_ARG
        assert _said(lib, call(p=params(device=-1), **kw), "device") == A.FW_ERR_BAD_ARG
        for name, off in (("aov", 4), ("aov", 8), ("sh", 2), ("lin", 2), ("gam", 2), ("pl", 2)) + ((("mom", 2),) if not kw else ()):
            assert _said(lib, call(p=params(on_device=1), **dict(kw, **{name: C.c_void_p(good[name] + off)})), "aligned") == A.FW_ERR_BAD_ARG, name
        assert _said(lib, call(_grid(counts=BIG), **kw), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
        assert _said(lib, call(p=params(width=0x10000, height=0x10000), **kw), "image too large") == A.FW_ERR_UNSUPPORTED
        if _lib.device_count() == 0:
            assert call(**kw) == A.FW_ERR_NO_DEVICE
        else:
            assert call(p=params(device=_lib.device_count()), **kw) == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert all(np.all(v == 7) for v in buf.values())


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("needs a machine without a GPU")
    grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))
    sh, pl = np.zeros((2, 9, 3), np.float32), api.neutral_placement(2)
    pts, nrm = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    calls = [lambda: _lib.probe_irradiance_placed(grid, sh, pl, pts, nrm),
             lambda: _lib.probe_irradiance_placed(grid, sh, pl, pts, nrm, ProbeDepth(4, 3, 5.0), np.ones((2, 4, 4, 2), np.float32)),
             lambda: _lib.probe_shade_placed(grid, sh, pl, np.zeros((1, 12), np.float32), 1, 1),
             lambda: _lib.probe_survey(np.zeros((2, 6), np.float32), np.zeros(2, _lib.HIT_DTYPE), 1),
             lambda: _lib.probe_relocate_step(ProbeRelocation(0.1, max_offset=1.0), np.zeros((2, 3, 4), np.float32), pl, 4)]
    for f in calls:
        with pytest.raises(_lib.FireworkError) as e:
            f()
        assert e.value.status == A.FW_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        _lib.probe_irradiance_placed(grid, sh, pl, pts, nrm, ProbeDepth(4, 3, 5.0), None)


# ---- the command line's refusals --------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "firework_amd", *args], cwd=ROOT, capture_output=True, text=True)


BAKE = ("--bake-probes", "2,2,2", "--probe-min", "0,0,0", "--probe-max", "1,1,1", "-o", "never_written.npz")


@pytest.mark.parametrize("args, word", [
    (("--probe-relocate", "0.1"), "--bake-probes"),
    ((*BAKE, "--probe-relocate", "0"), "--probe-relocate"),
    ((*BAKE, "--probe-relocate", "-1"), "--probe-relocate"),
    ((*BAKE, "--probe-relocate-steps", "2"), "--probe-relocate"),
    ((*BAKE, "--probe-relocate-max", "0.3"), "--probe-relocate"),
    ((*BAKE, "--probe-relocate", "0.1", "--probe-relocate-steps", "-1"), "--probe-relocate-steps"),
    ((*BAKE, "--probe-relocate", "0.1", "--probe-relocate-max", "-0.5"), "--probe-relocate-max"),
    ((*BAKE[:6], "--probe-relocate", "0.1"), "-o FILE.npz"),
    (("--bake-probes", "1,1,1", *BAKE[2:], "--probe-relocate", "0.1"), "spacing"),
    (("--probe-no-placement",), "--probe-lit"),
])
def test_cli_refusals(args, word):
    """refused where the siblings refuse: before the scene is read or the device looked for"""
    r = _cli("--scene-file", "no_such_scene_file.yaml", "-s", "1", *args)
    said = r.stderr.strip().splitlines()[-1]                                  # after the usage text: the parser's own message
    assert r.returncode == 2 and "error:" in said and word in said, (r.returncode, r.stderr)
    assert "no_such_scene_file" not in said and "device" not in said.lower() and not os.path.exists(os.path.join(ROOT, "never_written.npz"))
