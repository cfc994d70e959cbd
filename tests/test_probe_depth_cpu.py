"""CPU-side checks of probe visibility (fw_probe_depth_reduce, fw_bake_probe_depth, fw_probe_irradiance_vis, fw_probe_shade_vis;
DESIGN.md §9s): the exports and the struct's layout at ABI 8; the numpy statement's known answers (unit texel directions, the fetch at
a texel centre, the reduction to probe_lookup under constant moments, the 1 x 1 x 1 grid); the leak between a lit and a dark room,
analytically; and every argument error of the four calls in the header's order (they come before HIP is called)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import ProbeDepth, ProbeGrid, ProbeSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
MISS = np.uint32(0xFFFFFFFF)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    for name in A.PROBE_DEPTH_PROTOTYPES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name
    assert not hasattr(lib, "fw_probe_depth")


def test_struct_layout(tmp_path):
    """ctypes' fw_probe_depth equals the C compiler's, size and every field offset"""
    names = ["resolution", "sharpness_log2", "max_distance"]
    assert [f for f, _ in A.fw_probe_depth._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(fw_probe_depth)' +
           "".join(f",offsetof(fw_probe_depth,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_probe_depth)] + [getattr(A.fw_probe_depth, f).offset for f in names]


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 8, 16, 32])
def test_texel_directions_are_unit_and_fetch_returns_the_texel(R):
    T = api.probe_depth_dirs(R)
    assert T.shape == (R, R, 3)
    # three correctly rounded divisions by one correctly rounded length: |T| is 1 to a few float64 ulps
    assert np.all(np.abs(np.sqrt((T * T).sum(axis=-1)) - 1.0) <= 4 * 2.0 ** -53)
    assert len(np.unique(np.round(T.reshape(-1, 3), 12), axis=0)) == R * R                # all different
    assert np.all(T[: R // 2, :, 2].max(axis=0) >= 0) and T[0, 0, 2] < 0 and T[R // 2, R // 2, 2] > 0   # corners below, the centre above
    rng = np.random.default_rng(R)
    maps = rng.uniform(1.0, 9.0, size=(R * R, R, R, 2)).astype(np.float32)               # one map per fetched direction
    mu, mu2 = api.probe_depth_fetch(R, maps, T.reshape(-1, 3))
    b, a = np.divmod(np.arange(R * R), R)
    want = maps[np.arange(R * R), b, a].astype(np.float64)
    # the fetch lands on the texel's own centre to within the roundings of T, ox and su: su is off an integer by at most a few R u, and
    # the bilinear form then mixes in at most that much of a neighbour, a value of the same size: 64 R u relative is generous and derived
    tol = 64 * R * 2.0 ** -53 * 9.0
    assert np.all(np.abs(mu - want[:, 0]) <= tol) and np.all(np.abs(mu2 - want[:, 1]) <= tol)


def _points(n, rng, lo, hi):
    pts = (np.asarray(lo) + rng.uniform(-0.2, 1.2, size=(n, 3)) * (np.asarray(hi) - np.asarray(lo))).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]).astype(np.float32)
    return pts, nrm


@pytest.mark.parametrize("wrap", [True, False])
def test_constant_far_moments_reduce_to_the_lookup_with_the_crush(wrap):
    """With mu = r_max and mu2 = r_max^2 everywhere and every point nearer than r_max to its corner probes, dist <= mu holds, so v = 1 and
    g = crush(max(1e-6, fac)): probe_lookup_vis is probe_lookup's sum with the weights tri * g, normalised.  With wrap, fac = h h + 0.2
    lies in [0.2, 1.2], where neither the floor nor the crush acts (the crush needs g < 0.2), so the two functions agree bit for bit;
    without wrap g = 1 and the normalisation divides trilinear weights by their sum, 1 to a few ulps."""
    rng = np.random.default_rng(3)
    grid = ProbeGrid((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5), wrap)
    sh = rng.normal(size=(60, 9, 3)).astype(np.float32)
    pd = ProbeDepth(8, 6, 100.0)
    moments = np.empty((60, 8, 8, 2), np.float32)
    moments[..., 0], moments[..., 1] = 100.0, 100.0 * 100.0
    pts, nrm = _points(200, rng, grid.lo, grid.hi)
    E, T, X = api.probe_lookup_vis(grid, sh, pd, moments, pts, nrm, 0.0, terms=True)
    assert np.all(X["v"] == 1.0) and np.all(X["dist"] < 100.0)
    ref, Tref = api.probe_lookup(grid, sh, pts, nrm, terms=True)
    if wrap:
        assert np.all(X["fac"] >= 0.2) and np.array_equal(X["g"], X["fac"])
        assert np.array_equal(_u64(E), _u64(ref)) and np.array_equal(_u64(T), _u64(Tref))
    else:
        assert np.all(X["g"] == 1.0)
        assert np.all(np.abs(E - ref) <= 16 * 2.0 ** -53 * Tref)          # 8 additions, a division and the product, on weights that sum to 1
    # a bias keeps v = 1 here and moves nothing else: the wrap factor and the cell are taken at p, not at q
    assert np.array_equal(_u64(api.probe_lookup_vis(grid, sh, pd, moments, pts, nrm, 0.25)), _u64(E))


def test_a_single_probe_is_returned_whatever_its_visibility():
    """1 x 1 x 1: one corner, whose weight cancels in the normalisation — bit for bit probe_lookup's result"""
    rng = np.random.default_rng(4)
    sh = rng.normal(size=(1, 9, 3)).astype(np.float32)
    pts, nrm = _points(64, rng, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    moments = rng.uniform(0.01, 0.2, size=(1, 4, 4, 2)).astype(np.float32)            # nearly everything is behind something
    for wrap in (True, False):
        grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), wrap)
        E, _T, X = api.probe_lookup_vis(grid, sh, ProbeDepth(4, 3, 5.0), moments, pts, nrm, 0.0, terms=True)
        assert np.any(X["v"] < 0.5) and np.all(X["w"] == 1.0)
        assert np.array_equal(_u64(E), _u64(api.probe_lookup(grid, sh, pts, nrm)))


def test_moments_statement():
    pd = ProbeDepth(4, 0, 7.5)
    sums = np.zeros((1, 4, 4, 4), np.float32)
    sums[0, 0, 0] = (6.0, 18.0, 2.0, NAN)
    sums[0, 0, 1] = (1.0, 1.0, 3.0, 5.0)
    m = api.probe_depth_moments(pd, sums)
    assert m.dtype == np.float32 and m.shape == (1, 4, 4, 2)
    assert m[0, 0, 0].tolist() == [3.0, 9.0]
    assert m[0, 0, 1, 0] == np.float32(1.0 / 3.0) and m[0, 0, 1, 1] == np.float32(1.0 / 3.0)
    assert np.all(m[0, 1:] == np.array([7.5, 56.25], np.float32))                      # no weight: (r_max, r_max^2)


def test_reduce_statement_known_answers():
    """one ray straight at a texel centre: at k = 0 the texel gets w = 1 (to the roundings of |T|), A = dist, B = dist^2; a miss and a hit
    beyond r_max both count as r_max; non-unit directions scale t; the order of the rays does not matter to a single ray's texel"""
    R = 4
    T = api.probe_depth_dirs(R)
    pd = ProbeDepth(R, 0, 10.0)
    d = T[1, 2]
    rays = np.zeros((3, 6), np.float32)
    rays[:, 3:] = d
    rays[1, 3:] = 2.0 * d.astype(np.float32)                                            # twice as long: t counts double
    t = np.array([3.0, 2.5, 4.0], np.float32)
    out = api.probe_depth_reduce(pd, rays, t, np.array([0, 1, MISS], np.uint32), 3)
    assert out.shape == (1, R, R, 3)
    w = out[0, 1, 2, 2]
    assert abs(w - 4.0) <= 1e-6                                                          # 1 + 2 + 1 (float32 directions: 2^-24 each)
    assert abs(out[0, 1, 2, 0] - (3.0 + 2.0 * 5.0 + 10.0)) <= 1e-5 and abs(out[0, 1, 2, 1] - (9.0 + 2.0 * 25.0 + 100.0)) <= 1e-4
    far = api.probe_depth_reduce(pd, rays[:1], np.array([50.0], np.float32), np.array([7], np.uint32), 1)
    assert abs(far[0, 1, 2, 0] - 10.0) <= 1e-6
    # the opposite texel sees none of it: max(0, .) cuts the back hemisphere
    opposite = np.argmin((T * d).sum(axis=-1))
    assert out.reshape(-1, 3)[opposite].tolist() == [0.0, 0.0, 0.0]
    # sharper weights concentrate: at k = 6 a neighbour 30 degrees away weighs cos^64 < 1e-3 of the centre
    sharp = api.probe_depth_reduce(ProbeDepth(R, 6, 10.0), rays[:1], t[:1], np.array([0], np.uint32), 1)
    assert sharp[0, 1, 2, 2] > 0.99 and np.sort(sharp[0, :, :, 2].ravel())[-2] < 1e-3 * sharp[0, 1, 2, 2]


# ---- the leak, analytically ---------------------------------------------------------------------------------------------------------
def _two_rooms(R, k, D):
    """Probes at x = 0 (lit) and x = 4 (dark) and a wall at x = 1; r_max = 10; spherical-Fibonacci directions (the set's own, without
    jitter).  The lit probe sees the wall at 1 / d_x for d_x > 0, the dark probe at 3 / |d_x| for d_x < 0, everything else is a miss.
    Returns (grid with wrap, grid without, pd, moments)."""
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (2, 1, 1), D).jitter(False)
    rays = probes.rays(0)
    dx = rays[:, 3].astype(np.float64).reshape(2, D)
    obj = np.full((2, D), MISS, np.uint32)
    t = np.zeros((2, D), np.float32)
    with np.errstate(divide="ignore"):
        obj[0, dx[0] > 0], obj[1, dx[1] < 0] = 0, 0
        t[0] = np.where(dx[0] > 0, 1.0 / np.abs(dx[0]), 0.0)
        t[1] = np.where(dx[1] < 0, 3.0 / np.abs(dx[1]), 0.0)
    pd = ProbeDepth(R, k, 10.0)
    sums = np.zeros((2, R, R, 4), np.float32)
    sums[..., :3] = api.probe_depth_reduce(pd, rays, t.ravel(), obj.ravel(), D).astype(np.float32)
    return ProbeGrid.of(probes, True), ProbeGrid.of(probes, False), pd, api.probe_depth_moments(pd, sums)


def _lit_share(grid, pd, moments, normal):
    """the lit probe's share of the normalised weights at (2, 0, 0)"""
    sh = np.zeros((2, 9, 3), np.float32)
    _E, _T, X = api.probe_lookup_vis(grid, sh, pd, moments, np.array([[2.0, 0.0, 0.0]], np.float32), np.array([normal], np.float32), 0.0, terms=True)
    assert X["w"].shape == (1, 2) and abs(X["w"].sum() - 1.0) <= 4 * 2.0 ** -53
    return float(X["w"][0, 0])


def test_wrap_alone_leaks_half_and_a_seventh():
    """the two figures of the issue, from probe_lookup itself: at the midpoint the trilinear weights are equal; with the normal along the
    wall both wrap factors are 0.25 + 0.2; with the normal away from the lit probe they are 0.2 and 1.2"""
    grid = ProbeGrid((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (2, 1, 1), True)
    sh = np.zeros((2, 9, 3), np.float32)
    sh[0, 0] = 1.0                                                                       # only the lit probe holds light
    p = np.array([[2.0, 0.0, 0.0]], np.float32)
    own = api.probe_lookup(ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), True), sh[:1], p, np.array([[0.0, 1.0, 0.0]], np.float32))
    for normal, share in (((0.0, 1.0, 0.0), 0.5), ((1.0, 0.0, 0.0), 1.0 / 7.0)):
        E = api.probe_lookup(grid, sh, p, np.array([normal], np.float32))
        assert np.all(np.abs(E / own - share) <= 1e-12), (normal, E / own)


@pytest.mark.parametrize("R", [4, 8, 16])
@pytest.mark.parametrize("D", [64, 256, 1024])
def test_visibility_closes_the_leak(R, D):
    """The condition of the issue: with visibility at k >= 3 the lit probe's share at (2, 0, 0) is at most 1e-3 for both normals (the
    statement gives at most 6.7e-10); at k = 0 the cosine-weighted moments are too blurred to help, and the share stays where wrap alone
    leaves it, not even halved — the sharpness is what closes the leak."""
    for normal, wrap_share in (((0.0, 1.0, 0.0), 0.5), ((1.0, 0.0, 0.0), 1.0 / 7.0)):
        for k in (3, 6):
            grid, _plain, pd, moments = _two_rooms(R, k, D)
            share = _lit_share(grid, pd, moments, normal)
            print(f"R {R} D {D} k {k} normal {normal}: lit share {share:.3e}")
            assert 0.0 <= share <= 1e-3, (k, normal, share)
        grid, _plain, pd, moments = _two_rooms(R, 0, D)
        blurred = _lit_share(grid, pd, moments, normal)
        print(f"R {R} D {D} k 0 normal {normal}: lit share {blurred:.3e} (wrap alone {wrap_share:.3f})")
        assert blurred >= 0.5 * wrap_share, (normal, blurred)


def test_visibility_keeps_a_visible_probe():
    """the other side of the wall: at (0.5, 0, 0), in the lit room, the lit probe is nearer than its mean depth along +x and keeps
    v = 1, while the dark probe is cut — the weight goes where the light is"""
    grid, _plain, pd, moments = _two_rooms(8, 6, 256)
    sh = np.zeros((2, 9, 3), np.float32)
    _E, _T, X = api.probe_lookup_vis(grid, sh, pd, moments, np.array([[0.5, 0.0, 0.0]], np.float32), np.array([[0.0, 1.0, 0.0]], np.float32), 0.0,
                                     terms=True)
    assert X["v"][0, 0] == 1.0 and X["v"][0, 1] < 1e-3 and X["w"][0, 0] > 1.0 - 1e-6


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _depth(resolution=8, sharpness_log2=6, max_distance=10.0):
    d = A.fw_probe_depth()
    d.resolution, d.sharpness_log2, d.max_distance = resolution, sharpness_log2, max_distance
    return d


BAD_DEPTHS = [("resolution", _depth(resolution=0)), ("resolution", _depth(resolution=12)), ("resolution", _depth(resolution=64)),
              ("sharpness_log2", _depth(sharpness_log2=9)), ("max_distance", _depth(max_distance=0.0)), ("max_distance", _depth(max_distance=-1.0)),
              ("max_distance", _depth(max_distance=INF)), ("max_distance", _depth(max_distance=NAN))]


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


def test_probe_depth_reduce_argument_checks():
    lib = _lib.load()
    rays = np.zeros((2 * 5, 6), np.float32)
    rays[:, 4] = 1.0
    hits = np.zeros(2 * 5, _lib.HIT_DTYPE)
    sums = np.full((2, 8, 8, 4), 7.0, np.float32)
    good = dict(rays=rays.ctypes.data, hits=hits.ctypes.data, sums=sums.ctypes.data)

    def call(pd=None, n=2, d=5, device=0, on_device=0, null_pd=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_probe_depth_reduce(device, None if null_pd else C.byref(pd if pd is not None else _depth()), n, d, a["rays"], a["hits"], a["sums"],
                                         on_device, None)

    assert _said(lib, call(null_pd=True), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, pd in BAD_DEPTHS:
        assert _said(lib, call(pd), word) == A.FW_ERR_BAD_ARG, word
    # the order inside the description, then n_probes, directions, alignment, the two size limits, the device
    assert _said(lib, call(_depth(resolution=5, sharpness_log2=9, max_distance=NAN)), "resolution") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_depth(sharpness_log2=9, max_distance=NAN)), "sharpness_log2") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_depth(max_distance=NAN), n=0), "max_distance") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=0, d=0), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(d=0), "directions") == A.FW_ERR_BAD_ARG and _said(lib, call(d=(1 << 20) + 1), "directions") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("hits", 4), ("hits", 8), ("rays", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(n=1 << 11, d=1 << 20, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=1 << 11, d=1 << 20), "directions must be below") == A.FW_ERR_UNSUPPORTED          # n D = 2^31
    assert _said(lib, call(_depth(resolution=32), n=1 << 21, d=1), "resolution^2") == A.FW_ERR_UNSUPPORTED     # n R^2 = 2^31
    assert _said(lib, call(n=1 << 11, d=1 << 20, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0)
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_bake_probe_depth_argument_checks():
    """every refusal comes before the scene is looked at, so a scene handle that is never dereferenced will do"""
    lib = _lib.load()
    pos = np.zeros((3, 3), np.float32)
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call
    sums = np.zeros((3, 8, 8, 4), np.float32)
    mom = np.zeros((3, 8, 8, 2), np.float32)

    def pset(n=3, d=65, positions=pos):
        s = A.fw_probe_set()
        s.n_probes, s.directions, s.jitter, s.seed, s.chunk_probes = n, d, 1, 0, 0
        s.positions = None if positions is None else positions.ctypes.data_as(C.POINTER(C.c_float))
        return s

    def call(s=None, pd=None, first=0, rounds=1, on_device=0, null=None, sums_p=sums.ctypes.data, mom_p=mom.ctypes.data):
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, s=C.byref(s if s is not None else pset()), pd=C.byref(pd if pd is not None else _depth()), tp=C.byref(tp))
        if null:
            args[null] = None
        return lib.fw_bake_probe_depth(args["scene"], args["s"], args["pd"], args["tp"], first, rounds, sums_p, mom_p, None)

    for null in ("scene", "s", "pd", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    assert _said(lib, call(pset(positions=None)), "null positions") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(n=0)), "n_probes") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(d=0)), "directions") == A.FW_ERR_BAD_ARG
    bad = pos.copy()
    bad[1, 2] = NAN
    assert _said(lib, call(pset(positions=bad)), "probe 1") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pset(positions=bad), _depth(resolution=5)), "probe 1") == A.FW_ERR_BAD_ARG            # the set before the description
    for word, pd in BAD_DEPTHS:
        assert _said(lib, call(pd=pd, rounds=0), word) == A.FW_ERR_BAD_ARG, word                                   # the description before the rounds
    assert _said(lib, call(rounds=0), "rounds") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=2, sums_p=None), "first_round > 0") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(on_device=1, sums_p=C.c_void_p(sums.ctypes.data + 8)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(on_device=1, mom_p=C.c_void_p(mom.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    big = np.zeros(((1 << 11), 3), np.float32)
    assert _said(lib, call(pset(n=1 << 11, d=1 << 20, positions=big), rounds=0), "rounds") == A.FW_ERR_BAD_ARG   # bad arguments before the size
    assert _said(lib, call(pset(n=1 << 11, d=1 << 20, positions=big)), "directions must be below") == A.FW_ERR_UNSUPPORTED
    wide = np.zeros(((1 << 21), 3), np.float32)
    assert _said(lib, call(pset(n=1 << 21, d=1, positions=wide), _depth(resolution=32)), "resolution^2") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE


def _vis_buffers():
    return dict(sh=np.full((12, 9, 3), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32), pos=np.full((5, 3), 7.0, np.float32),
                nrm=np.full((5, 3), 7.0, np.float32), out=np.full((5, 3), 7.0, np.float32))


BIG = (1 << 11, 1 << 10, 1 << 10)        # nx ny nz = 2^31 (neither sh nor the moments are read: the count comes first)
BAD_GRIDS = [("count", _grid(counts=(2, 0, 2))), ("finite", _grid(lo=(0.0, NAN, 0.0))), ("hi != lo", _grid(lo=(0.0, 2.0, 0.0))), ("flags", _grid(flags=2))]
BAD_BIAS = [-0.5, NAN, INF, -INF]


def test_probe_irradiance_vis_argument_checks():
    lib = _lib.load()
    buf = _vis_buffers()
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(g=None, pd=None, bias=0.0, device=0, n=5, stride=3, on_device=0, null=None, **ptrs):
        a = dict(good, **ptrs)
        gp = None if null == "grid" else C.byref(g if g is not None else _grid())
        pp = None if null == "pd" else C.byref(pd if pd is not None else _depth())
        return lib.fw_probe_irradiance_vis(gp, a["sh"], pp, a["mom"], bias, device, n, a["pos"], a["nrm"], stride, a["out"], on_device, None)

    for null in ("grid", "pd"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in good:
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, pd in BAD_DEPTHS:
        assert _said(lib, call(pd=pd, bias=-1.0), word) == A.FW_ERR_BAD_ARG, word                                   # the description before the bias
    for bias in BAD_BIAS:
        assert _said(lib, call(_grid(flags=2), bias=bias), "normal_bias") == A.FW_ERR_BAD_ARG, bias                 # the bias before the grid
    for word, g in BAD_GRIDS:
        assert _said(lib, call(g, n=0), word) == A.FW_ERR_BAD_ARG, word                                             # the grid before n
    assert _said(lib, call(n=0, stride=0), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, device=-1), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(device=-1), "device") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + 2)}), "aligned") == A.FW_ERR_BAD_ARG, name
    big = _grid(counts=BIG)
    assert _said(lib, call(big, stride=2), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(big), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_grid(counts=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_grid(counts=(1 << 7, 1 << 7, 1 << 7)), _depth(resolution=32)), "resolution^2") == A.FW_ERR_UNSUPPORTED   # 2^21 x 2^10
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert call(device=_lib.device_count()) == A.FW_ERR_BAD_ARG


def test_probe_shade_vis_argument_checks():
    lib = _lib.load()
    buf = dict(sh=np.full((12, 9, 3), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32), aov=np.full((6, 12), 7.0, np.float32),
               lin=np.full((6, 3), 7.0, np.float32), gam=np.full((6, 3), 7.0, np.float32), rgb8=np.full((6, 3), 7, np.uint8))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def params(**kw):
        p = A.fw_probe_shade_params()
        p.width, p.height, p.gamma = 3, 2, 2.2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(g=None, pd=None, bias=0.0, p=None, null=None, **ptrs):
        a = dict(good, **ptrs)
        gp = None if null == "grid" else C.byref(g if g is not None else _grid())
        dp = None if null == "pd" else C.byref(pd if pd is not None else _depth())
        pp = None if null == "p" else C.byref(p if p is not None else params())
        return lib.fw_probe_shade_vis(gp, a["sh"], dp, a["mom"], bias, pp, a["aov"], a["lin"], a["gam"], a["rgb8"])

    for null in ("grid", "pd", "p"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("sh", "mom", "aov"):
        assert _said(lib, call(**{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(pd=_depth(resolution=5), lin=None, gam=None, rgb8=None), "output") == A.FW_ERR_BAD_ARG   # the outputs first
    for word, pd in BAD_DEPTHS:
        assert _said(lib, call(pd=pd, bias=-1.0), word) == A.FW_ERR_BAD_ARG, word
    for bias in BAD_BIAS:
        assert _said(lib, call(_grid(flags=2), bias=bias), "normal_bias") == A.FW_ERR_BAD_ARG, bias
    for word, g in BAD_GRIDS:
        assert _said(lib, call(g, p=params(width=0)), word) == A.FW_ERR_BAD_ARG, word
    assert _said(lib, call(p=params(width=0, gamma=0.0)), "width") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(gamma=NAN, device=-1)), "gamma") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(device=-1)), "device") == A.FW_ERR_BAD_ARG
    for name, off in (("aov", 4), ("aov", 8), ("sh", 2), ("lin", 2), ("gam", 2), ("mom", 2)):
        assert _said(lib, call(p=params(on_device=1), **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(_grid(counts=BIG)), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_grid(counts=(1 << 7, 1 << 7, 1 << 7)), _depth(resolution=32)), "resolution^2") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_grid(counts=(1 << 7, 1 << 7, 1 << 7)), _depth(resolution=32), p=params(width=0x10000, height=0x10000)), "resolution^2") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(p=params(width=0x10000, height=0x10000)), "image too large") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7) for v in buf.values())
    else:
        assert call(p=params(device=_lib.device_count())) == A.FW_ERR_BAD_ARG


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("needs a machine without a GPU")
    grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))
    pd = ProbeDepth(4, 3, 5.0)
    sh, mom = np.zeros((2, 9, 3), np.float32), np.ones((2, 4, 4, 2), np.float32)
    pts = np.zeros((1, 3), np.float32)
    nrm = np.ones((1, 3), np.float32)
    with pytest.raises(_lib.FireworkError) as e:
        _lib.probe_irradiance_vis(grid, sh, pd, mom, pts, nrm)
    assert e.value.status == A.FW_ERR_NO_DEVICE
    with pytest.raises(_lib.FireworkError) as e:
        _lib.probe_shade_vis(grid, sh, pd, mom, np.zeros((1, 12), np.float32), 1, 1)
    assert e.value.status == A.FW_ERR_NO_DEVICE
    with pytest.raises(_lib.FireworkError) as e:
        _lib.probe_depth_reduce(pd, np.zeros((2, 6), np.float32), np.zeros(2, _lib.HIT_DTYPE), 1)
    assert e.value.status == A.FW_ERR_NO_DEVICE
