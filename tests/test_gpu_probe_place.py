"""Probe relocation and classification on the device: fw_probe_survey and fw_probe_relocate_step against their numpy
statements (api.probe_survey, api.probe_relocate_step) within the bounds tests/probe_place_ref.py derives; fw_relocate_probes against its
composition by hand, progressive, and leaving renders alone; the placed lookups against api.probe_lookup_placed and, with a neutral
placement, bit for bit against their counterparts; a black box around a probe, end to end; render_probe_lit and the command line."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import (ColorEnv, LambertianMat, ProbeDepth, ProbeGrid, ProbeRelocation, ProbeSet, Rect3d, RenderObject, Scene, Sphere,
                              XZRect)

import probe_place_ref as REF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FAR = np.array([3e3, -2e3, 5e3])
# test_gpu_probe_lookup.py's grids: a single probe, one and two flat axes, the smallest full cell, an uneven grid, and two far from the origin
GRIDS = [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)), ((-1.0, 0.0, 0.0), (2.0, 1.0, 1.0), (2, 1, 1)), ((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (1, 3, 2)),
         ((0.0, 0.0, 0.0), (1.0, 2.0, 0.5), (2, 2, 2)), ((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5)),
         (tuple(FAR - 1.0), tuple(FAR + (1.0, 2.0, 0.5)), (2, 2, 2)), (tuple(FAR - (1.5, 0.25, 2.0)), tuple(FAR + (2.0, 1.75, 3.0)), (4, 3, 5))]
COUNTS_N = [1, 63, 65, 200]          # one point, a wave's tail, a wave plus one, several waves with a tail
DIRECTIONS = [1, 63, 64, 65, 200]    # one ray, a wave's tail, a wave, a wave plus one, several strides with a tail


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _hits_tensor(hits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.float32).reshape(-1, 12)).to(dev)


# ---- fw_probe_survey ------------------------------------------------------------------------------------------------------------------
def _hand_made(n, D, rng):
    """rays with directions of length 0.5 .. 2 and hits that in turn miss, sit at t = 0 and lie in between, normals of both signs; some
    rays zeroed; and, where D allows, exact ties in distance: every hit at t = 0 (the minimum of both classes) and two pairs of twins
    (equal t along equal directions) further out"""
    d = rng.normal(size=(n * D, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n * D, 1))
    rays = np.zeros((n * D, 6), np.float32)
    rays[:, :3] = rng.normal(size=(n * D, 3))
    rays[:, 3:] = d
    hits = np.zeros(n * D, _lib.HIT_DTYPE)
    kind = (np.arange(n * D) + rng.integers(3)) % 3
    hits["t"] = rng.uniform(0.01, 5.0, size=n * D)
    hits["object"] = rng.integers(0, 9, size=n * D)
    hits["normal"] = rng.normal(size=(n * D, 3))
    hits["point"], hits["prim"], hits["u"] = rng.normal(size=(n * D, 3)), 5, 0.5           # never read
    if D >= 63:
        hits["t"][kind == 1] = 0.0
        zero = rng.random(n * D) < 0.1
        rays[zero, 3:] = 0.0
        for p in range(n):                       # two pairs of twins per probe: the same direction, t and normal, one pair per class
            for c, (a, b) in enumerate(((7, 40), (12, 33))):
                ia, ib = p * D + a, p * D + b
                rays[ia, 3:] = rays[ib, 3:] = (0.25, -0.5, 1.0)
                hits["t"][ia] = hits["t"][ib] = 2.0 ** -10
                hits["object"][ia] = hits["object"][ib] = 1
                hits["normal"][ia] = hits["normal"][ib] = (0.0, 0.0, 1.0 if c == 0 else -1.0)
                kind[ia] = kind[ib] = 2
    miss = kind == 0
    hits["object"][miss] = A.FW_NO_HIT
    for f in ("t", "u", "v", "prim", "material"):
        hits[f][miss] = 0
    hits["point"][miss], hits["normal"][miss] = 0.0, 0.0                                  # a miss has every other field 0
    return rays, hits


@pytest.mark.parametrize("n", [1, 3])
def test_survey_matches_the_statement(n):
    torch, dev = _torch()
    rng = np.random.default_rng(n)
    side = torch.cuda.Stream(device=dev)
    for D in DIRECTIONS:
        rays, hits = _hand_made(n, D, rng)
        args = (rays, hits["t"], hits["normal"], hits["object"], D)
        assert REF.survey_gap(*args) > REF.argmin_gap                                     # asked of the inputs before the device is
        ref, J = api.probe_survey(*args, terms=True)
        what = f"n {n} D {D}"
        if D >= 63:
            # exact ties at the minimum of both classes (the hits at t = 0): without the winner the same distance wins again, further on
            fewer = rays.copy()
            fewer.reshape(n, D, 6)[np.arange(n)[:, None], J, 3:] = 0.0
            ref2, J2 = api.probe_survey(fewer, *args[1:], terms=True)
            assert np.all(J >= 0) and np.all(J2 > J) and np.array_equal(ref2[:, 0:2, 3], ref[:, 0:2, 3]) and np.all(ref[:, 2, 0:3] > 0), what
        host = np.full((n, 3, 4), NAN, np.float32)
        assert _lib.probe_survey(rays, hits, D, out=host) is host
        assert not np.any(np.isnan(host)), what                                           # fully overwritten
        assert np.array_equal(host[:, 2], ref[:, 2].astype(np.float32)), what             # the counts are exact
        for c in (0, 1):
            want_dir = np.where((J[:, c] >= 0)[:, None], rays.reshape(n, D, 6)[np.arange(n), np.maximum(J[:, c], 0), 3:], np.float32(0.0))
            assert np.array_equal(_u32(host[:, c, 0:3]), _u32(want_dir.astype(np.float32))), (what, c)        # the winner's stored bits
            none = J[:, c] < 0
            assert np.all(host[none, c, 3] == INF)
            err = np.abs(host[~none, c, 3].astype(np.float64) - ref[~none, c, 3])
            assert np.all(err <= REF.survey_dist_bound(ref[~none, c, 3])), (what, c, err)
        # device arrays on a side stream give the same bits, two runs are bit-equal, and the inputs are only read
        d_rays, d_hits = torch.from_numpy(rays).to(dev), _hits_tensor(hits, dev)
        outs = []
        for _ in range(2):
            d_out = torch.full((n, 3, 4), NAN, dtype=torch.float32, device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                assert _lib.probe_survey(d_rays, d_hits, D, out=d_out) is d_out
            side.synchronize()
            outs.append(d_out.cpu().numpy())
        assert np.array_equal(_u32(outs[0]), _u32(host)) and np.array_equal(_u32(outs[1]), _u32(host)), what
        assert np.array_equal(_u32(d_rays.cpu().numpy()), _u32(rays)) and np.array_equal(_u32(d_hits.cpu().numpy()), _u32(_hits_tensor(hits, "cpu").numpy()))
        # a probe's record is its own rays': each probe alone gives its slice
        for p in range(n):
            one = _lib.probe_survey(rays[p * D:(p + 1) * D], hits[p * D:(p + 1) * D], D)
            assert np.array_equal(_u32(one[0]), _u32(host[p])), (what, p)


# ---- fw_probe_relocate_step -----------------------------------------------------------------------------------------------------------
def _branches(n, rng):
    """surveys and placements that walk the four branches in turn: inside and allowed, too near a front face, neither, inside and
    rejected; offsets already present; D = 64"""
    sv = np.zeros((n, 3, 4), np.float32)
    pl = np.zeros((n, 4), np.float32)
    pl[:, 0:3] = rng.uniform(-0.2, 0.2, size=(n, 3))
    pl[:, 3] = rng.integers(0, 2, size=n)
    d = rng.normal(size=(n, 2, 3))
    sv[:, 0:2, 0:3] = d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 2, 1))
    kind = np.arange(n) % 4
    sv[:, 0, 3] = np.where(kind == 3, 5.0, rng.uniform(0.05, 0.6, size=n))                # branch 3 asks for more than max_offset allows
    sv[:, 1, 3] = np.where(kind == 1, rng.uniform(0.01, 0.2, size=n), rng.uniform(0.3, 2.0, size=n))
    sv[:, 2, 0] = np.where((kind == 0) | (kind == 3), rng.integers(17, 64, size=n), rng.integers(0, 17, size=n))   # > 16 = 0.25 x 64 is inside
    sv[:, 2, 1] = 64 - sv[:, 2, 0]
    return sv, pl, kind


@pytest.mark.parametrize("n", [1, 65])
def test_relocate_step_matches_the_statement(n):
    torch, dev = _torch()
    rl = ProbeRelocation(0.25, 0.25, (1.5, 1.5, 1.5))
    for trial in range(4 if n == 1 else 1):            # n = 1: each branch in turn
        rng = np.random.default_rng(100 * n + trial)
        sv, pl, kind = _branches(max(n, 4), rng)
        if n == 1:
            sv, pl, kind = sv[trial:trial + 1].copy(), pl[trial:trial + 1].copy(), kind[trial:trial + 1]
        ref = api.probe_relocate_step(rl, sv, pl, 64)
        moved = np.any(ref[:, 0:3] != pl[:, 0:3], axis=1)
        assert np.array_equal(moved, (kind == 0) | (kind == 1)), (n, trial)               # the cases keep clear of max_offset: see probe_place_ref
        assert np.array_equal(ref[:, 3] == 0.0, (kind == 0) | (kind == 3))
        got = _lib.probe_relocate_step(rl, sv, pl.copy(), 64)
        assert np.array_equal(_u32(got[:, 3]), _u32(ref[:, 3])), (n, trial)               # the state is decided on exact integers
        assert np.array_equal(_u32(got[~moved]), _u32(ref[~moved]))                       # kept offsets are kept bit for bit
        err = np.abs(got[:, 0:3].astype(np.float64) - ref[:, 0:3].astype(np.float64))
        assert np.all(err <= REF.step_bound(pl, sv, rl.min_front, rl.back_fraction, 64)), (n, trial, err.max())
        d_pl = torch.from_numpy(pl).to(dev)
        assert _lib.probe_relocate_step(rl, torch.from_numpy(sv).to(dev), d_pl, 64) is d_pl
        assert np.array_equal(_u32(d_pl.cpu().numpy()), _u32(got))
        # move = 0 writes the state alone
        only = _lib.probe_relocate_step(rl, sv, pl.copy(), 64, move=False)
        assert np.array_equal(_u32(only[:, 0:3]), _u32(pl[:, 0:3])) and np.array_equal(_u32(only[:, 3]), _u32(ref[:, 3]))
        assert np.array_equal(_u32(only), _u32(api.probe_relocate_step(rl, sv, pl, 64, move=False)))


# ---- fw_relocate_probes ---------------------------------------------------------------------------------------------------------------
def _closed_form_scene():
    """the scenes of tests/test_probe_place_cpu.py in one: a unit sphere at the origin and a wide floor at y = -3"""
    scene = Scene.new()
    grey = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, grey)))
    scene.add_object(RenderObject.new(XZRect.new(-1000.0, 1000.0, -1000.0, 1000.0, -3.0, grey)))
    scene.set_environment(ColorEnv((0.5, 0.5, 0.5)))
    # inside the sphere; 0.1 above the floor; 0.1 below it; far above everything; inside the sphere at its centre
    return scene, [[0.3, 0.2, -0.1], [5.0, -2.9, 0.0], [5.0, -3.1, 0.0], [40.0, 300.0, 20.0], [0.0, 0.0, 0.0]]


def _suzanne_scene():
    scene, _r = scenes.config("C3_suzanne", 24, 16, 2)             # the mesh at the origin and a floor at y = -1
    return scene, [[0.0, 0.0, 0.0], [0.0, 0.1, 1.6], [0.0, -0.95, 2.0], [0.0, -1.05, 2.0], [3.0, 3.0, 3.0]]


def _renderer(use_bvh, seed=11):
    cam = api.CameraSettings.default().cam_pos((0.0, 1.0, 8.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    return api.Renderer.default().width(24).height(16).samples(2).use_bvh(use_bvh).seed(seed).camera(cam)


def _chained(ds, r, probes, rl, steps, first_step=0, placement=None):
    """fw_probe_rays over a set at the moved positions, fw_trace_rays (seed + step, key_base 0), fw_probe_survey and
    fw_probe_relocate_step by hand, on the device over the whole set; then the classifying step"""
    torch, dev = _torch()
    s = r.settings
    D, n = probes.directions, probes.n_probes
    pl = api.neutral_placement(n) if placement is None else placement.copy()
    survey = None
    for i in range(steps + 1):
        st = first_step + i
        rays = _lib.probe_rays(probes.moved(pl), st, out=torch.empty((n * D, 6), dtype=torch.float32, device=dev))
        hits = ds.trace(rays, s["use_bvh"], seed=s["seed"] + st)
        survey = _lib.probe_survey(rays, hits, D)
        d_pl = torch.from_numpy(pl).to(dev)
        _lib.probe_relocate_step(rl, survey, d_pl, D, move=i < steps)
        pl = d_pl.cpu().numpy()
    return pl, survey.cpu().numpy()


@pytest.mark.parametrize("which,bvh", [("closed", False), ("closed", True), ("suzanne", True)])
def test_relocate_equals_its_composition_and_is_progressive(which, bvh):
    scene, positions = _closed_form_scene() if which == "closed" else _suzanne_scene()
    r = _renderer(bvh)
    probes = ProbeSet(positions, 65).seed(7)
    rl = ProbeRelocation(0.25, 0.25, (2.0, 2.0, 2.0), steps=3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        before = ds.render(r)
        ref_pl, ref_sv = _chained(ds, r, probes, rl, 3)
        for chunk in (1, 2, 0):
            pl, sv = r.relocate_probes(ds, probes, rl, chunk=chunk)
            assert np.array_equal(_u32(pl), _u32(ref_pl)) and np.array_equal(_u32(sv), _u32(ref_sv)), (which, bvh, chunk)
            st = r.probe_place_stats
            assert st["rays"] == 5 * 65 * (3 + 1) and st["ms_render"] > 0, st
        # progressive: (0, 2) then (2, 1) leaves what (0, 3) leaves
        two = ProbeRelocation(0.25, 0.25, (2.0, 2.0, 2.0), steps=2)
        pl2, sv2 = r.relocate_probes(ds, probes, two, chunk=2)
        c_pl2, c_sv2 = _chained(ds, r, probes, two, 2)
        assert np.array_equal(_u32(pl2), _u32(c_pl2)) and np.array_equal(_u32(sv2), _u32(c_sv2))
        one = ProbeRelocation(0.25, 0.25, (2.0, 2.0, 2.0), steps=1)
        pl3, sv3 = r.relocate_probes(ds, probes, one, first_step=2, placement=pl2, chunk=1)
        assert pl3 is pl2 and np.array_equal(_u32(pl3), _u32(ref_pl)) and np.array_equal(_u32(sv3), _u32(ref_sv))
        # steps = 0 classifies only: no offset moves
        zero = ProbeRelocation(0.25, 0.25, (2.0, 2.0, 2.0), steps=0)
        pl0, _sv0 = r.relocate_probes(ds, probes, zero)
        assert np.all(pl0[:, 0:3] == 0.0) and r.probe_place_stats["rays"] == 5 * 65
        # timing changes no bit, and the kernels' time is reported
        t = _renderer(bvh)
        t.settings["flags"] = t.settings["flags"] | A.FW_FLAG_TIME_KERNELS
        pl_t, _sv_t = t.relocate_probes(ds, probes, rl, chunk=2)
        assert np.array_equal(_u32(pl_t), _u32(ref_pl)) and t.probe_place_stats["ms_raygen"] > 0 and t.probe_place_stats["ms_accumulate"] > 0
        # fw_render is left as it was
        after = ds.render(r)
        assert np.array_equal(after.rgb8, before.rgb8) and np.array_equal(_u32(after.linear), _u32(before.linear))
    finally:
        ds.close()
    where = probes.positions.astype(np.float64) + ref_pl[:, 0:3].astype(np.float64)
    print(f"{which} bvh {bvh}: placement\n{ref_pl}\nfinal counts\n{ref_sv[:, 2]}")
    if which == "closed":
        assert pl0[:, 3].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]                             # classified where they stand
        for p in (0, 4):                                                                   # out of the sphere, min_front clear of it, active
            assert 1.24 <= np.linalg.norm(where[p]) <= 1.25 + 0.125 and ref_pl[p, 3] == 1.0 and ref_sv[p, 2, 0] == 0.0, where[p]
        assert -3.0 + 0.24 <= where[1, 1] <= -3.0 + 0.2501 and ref_pl[1, 3] == 1.0         # lifted to min_front above the floor
        assert -3.0 + 0.24 <= where[2, 1] <= -3.0 + 0.2501 and ref_pl[2, 3] == 1.0         # brought up through it, then lifted
        assert np.array_equal(_u32(ref_pl[3]), _u32(api.neutral_placement(1)[0]))          # nothing near: the neutral record, bit for bit
    else:
        assert ref_pl[1, 3] == 1.0 and ref_pl[4, 3] == 1.0 and np.all(ref_pl[4, 0:3] == 0.0)
        assert where[3, 1] > -1.0 and ref_pl[3, 3] == 1.0                                  # from under the floor to above it


# ---- fw_probe_irradiance_placed, fw_probe_shade_placed ----------------------------------------------------------------------------------
def _points(grid, n, rng):
    """test_gpu_probe_lookup.py's families: n float32 points in turn strictly inside the grid, exactly on a probe, on a face, on an edge
    and outside a face (all six in turn), with normals of length 1, 0.5 and 3"""
    lo, hi = np.array(grid.lo), np.array(grid.hi)
    probes = ProbeSet.grid(grid.lo, grid.hi, grid.counts).positions
    pts = (lo + rng.uniform(0.05, 0.95, size=(n, 3)) * (hi - lo)).astype(np.float32)
    for i in range(n):
        kind, k = i % 5, (i // 5) % 3
        if kind == 1:
            pts[i] = probes[rng.integers(len(probes))]
        elif kind == 2:
            pts[i, k] = np.float32((lo, hi)[(i // 15) % 2][k])
        elif kind == 3:
            pts[i, k] = np.float32(lo[k])
            pts[i, (k + 1) % 3] = np.float32(hi[(k + 1) % 3])
        elif kind == 4:
            side = (i // 15) % 2
            pts[i, k] = np.float32((lo[k] - 0.75 * (hi[k] - lo[k]) - 0.5) if side == 0 else (hi[k] + 1.25 * (hi[k] - lo[k]) + 0.5))
    nrm = rng.normal(size=(n, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]
    return pts, nrm.astype(np.float32)


def _random_moments(n_probes, res, rng):
    mu = rng.uniform(0.2, 3.0, size=(n_probes, res, res))
    return np.stack([mu, mu * mu + rng.uniform(0.05, 1.0, size=mu.shape)], axis=-1).astype(np.float32)


def _random_placement(grid, rng):
    """offsets within 0.45 of the spacing (of the extent on a flat axis), a quarter of the probes inactive — never all of them"""
    n = grid.n_probes
    span = np.array([abs(grid.hi[k] - grid.lo[k]) / max(grid.counts[k] - 1, 1) for k in range(3)])
    pl = api.neutral_placement(n)
    pl[:, 0:3] = rng.uniform(-0.45, 0.45, size=(n, 3)) * span
    pl[rng.random(n) < 0.25, 3] = 0.0
    if n > 1:
        pl[rng.integers(n), 3] = 1.0
    return pl


def _assert_within(got, ref, bound, what):
    assert got.dtype == np.float32 and got.shape == ref.shape and np.all(np.isfinite(got)), what
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (what, float((err / bound).max()), np.argwhere(err > bound)[:4])


@pytest.mark.parametrize("lo,hi,counts", GRIDS)
def test_placed_lookup_matches_the_statement_and_its_counterparts(lo, hi, counts):
    torch, dev = _torch()
    rng = np.random.default_rng(sum(counts) * 13 + int(lo[0] > 100))
    n_probes = counts[0] * counts[1] * counts[2]
    sh = rng.normal(size=(n_probes, 9, 3)).astype(np.float32)
    d_sh = torch.from_numpy(sh).to(dev)
    neutral = api.neutral_placement(n_probes)
    side = torch.cuda.Stream(device=dev)
    for res, wrap, bias in ((8, True, 0.0), (4, False, 0.125), (None, True, 0.0), (None, False, 0.0)):
        grid = ProbeGrid(lo, hi, counts, wrap)
        pd = None if res is None else ProbeDepth(res, 6, 10.0)
        moments = None if res is None else _random_moments(n_probes, res, rng)
        vis = () if res is None else (pd, moments, bias)
        pl = _random_placement(grid, rng)
        off = pl[:, 3] == 0.0
        bad_sh = sh.copy()
        bad_sh[off] = NAN
        bad_mom = None
        if res is not None:
            bad_mom = moments.copy()
            bad_mom[off] = NAN
        for n in COUNTS_N:
            pts, nrm = _points(grid, n, rng)
            what = f"{counts} R {res} wrap {wrap} bias {bias} n {n}"
            # a neutral placement: the counterpart's bits wherever the counterpart normalises
            got0 = _lib.probe_irradiance_placed(grid, sh, neutral, pts, nrm, *vis)
            if res is not None:
                assert np.array_equal(_u32(got0), _u32(_lib.probe_irradiance_vis(grid, sh, pd, moments, pts, nrm, bias))), what
            elif wrap:
                assert np.array_equal(_u32(got0), _u32(_lib.probe_irradiance(grid, sh, pts, nrm))), what
            # moved and classified probes, NaN in every inactive probe's sh and moments: the statement's bound, and finite
            ref, T, X = api.probe_lookup_placed(grid, sh, pl, pts, nrm, *vis, terms=True)
            bound = REF.placed_bound(ref, T, X, grid, res, pts, bias, pl)
            host = np.full((n, 3), NAN, np.float32)
            assert _lib.probe_irradiance_placed(grid, bad_sh, pl, pts, nrm, pd, bad_mom, bias, out=host) is host
            _assert_within(host, ref, bound, what + " host")
            # device arrays in place in 48-byte records (stride 12), into a NaN-filled tensor on a side stream
            rec = np.full((n, 12), NAN, np.float32)
            rec[:, 8:11], rec[:, 4:7] = pts, nrm
            d_rec = torch.from_numpy(rec).to(dev)
            out = torch.full((n, 3), NAN, dtype=torch.float32, device=dev)
            d_mom = None if res is None else torch.from_numpy(bad_mom).to(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                _lib.probe_irradiance_placed(grid, torch.from_numpy(bad_sh).to(dev), torch.from_numpy(pl).to(dev), d_rec[:, 8:11], d_rec[:, 4:7], pd,
                                             d_mom, bias, out=out)
            side.synchronize()
            assert np.array_equal(_u32(out.cpu().numpy()), _u32(host)), what + " device records"
        # every probe inactive: zeros, whatever the arrays hold
        none = neutral.copy()
        none[:, 3] = 0.0
        assert np.all(_u32(_lib.probe_irradiance_placed(grid, np.full_like(sh, NAN), none, pts, nrm, *vis)) == 0), what
    del d_sh


@pytest.mark.parametrize("w,h", [(17, 5), (64, 1)])
def test_shade_placed_is_the_float32_statement_on_the_lookups_output(w, h):
    torch, dev = _torch()
    rng = np.random.default_rng(w)
    n = w * h
    for wrap, res, bias in ((True, 8, 0.05), (False, None, 0.0)):
        grid = ProbeGrid((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (3, 2, 2), wrap)
        sh = rng.normal(size=(12, 9, 3)).astype(np.float32)
        pd = None if res is None else ProbeDepth(res, 6, 10.0)
        moments = None if res is None else _random_moments(12, res, rng)
        pl = _random_placement(grid, rng)
        pts, nrm = _points(grid, n, rng)
        rec = np.zeros((n, 12), np.float32)
        rec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
        rec[:, 3] = np.array([0.0, 0.25, 1.0], np.float32)[np.arange(n) % 3]
        rec[:, 4:7], rec[:, 8:11] = nrm, pts
        rec[::6, 4:7] = 0.0
        E = _lib.probe_irradiance_placed(grid, sh, pl, rec[:, 8:11], rec[:, 4:7], pd, moments, bias)
        want = api.probe_shade_ref(grid, sh, rec, E)
        gamma = 2.2 if wrap else 1.7
        rgb8, gam, lin = _lib.probe_shade_placed(grid, sh, pl, rec, w, h, pd, moments, bias, gamma)
        assert np.array_equal(_u32(lin), _u32(want))
        ref8, refg, _refl = _lib.denoise(want, rec, None, w, h, 0, gamma)                  # resolve_pixel(out, 1, gamma), as fw_denoise writes it
        assert np.array_equal(_u32(gam), _u32(refg)) and np.array_equal(rgb8, ref8)
        d_mom = None if res is None else torch.from_numpy(moments).to(dev)
        d8, dg, dl = _lib.probe_shade_placed(grid, torch.from_numpy(sh).to(dev), torch.from_numpy(pl).to(dev), torch.from_numpy(rec).to(dev), w, h, pd,
                                             d_mom, bias, gamma)
        assert np.array_equal(d8.cpu().numpy(), rgb8) and np.array_equal(_u32(dg.cpu().numpy()), _u32(gam)) and np.array_equal(_u32(dl.cpu().numpy()), _u32(lin))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _boxed_probe_scene():
    """a white environment, a grey floor at y = 0, and a black closed box of half-size 0.5 around (0, 1, 0)"""
    scene = Scene.new()
    grey = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    black = scene.add_material(LambertianMat.with_color((0.0, 0.0, 0.0)))
    scene.add_object(RenderObject.new(XZRect.new(-1000.0, 1000.0, -1000.0, 1000.0, 0.0, grey)))
    scene.add_object(RenderObject.new(Rect3d.with_size((1.0, 1.0, 1.0), black)).position(-0.5, 0.5, -0.5))
    scene.set_environment(ColorEnv((1.0, 1.0, 1.0)))
    return scene


def test_a_probe_inside_a_black_box_end_to_end():
    """A 3 x 1 x 1 grid at x = -2, 0, 2 and y = 1; the middle probe sits in the box.  With max_offset 0.3 it cannot leave (it needs 0.5 and
    more): rejected, inactive, and the floor point between probes 1 and 2 is lit by probe 2 alone — more than the plain lookup gives,
    which blends the black probe in.  With max_offset 0.9 it leaves and ends active."""
    probes = ProbeSet.grid((-2.0, 1.0, 0.0), (2.0, 1.0, 0.0), (3, 1, 1), 65).seed(3)
    r = _renderer(True, seed=5)
    r.samples(8)
    p, nrm = np.array([[1.0, 0.0, 0.0]], np.float32), np.array([[0.0, 1.0, 0.0]], np.float32)
    ds = _lib.DeviceScene(_boxed_probe_scene().to_desc())
    try:
        pl, sv = r.relocate_probes(ds, probes, ProbeRelocation(0.25, max_offset=0.3, steps=2))
        assert sv[1, 2].tolist() == [65.0, 0.0, 0.0, 0.0] and pl[1].tolist() == [0.0, 0.0, 0.0, 0.0]          # rejected where it stands: inactive
        assert pl[0].tolist() == pl[2].tolist() == [0.0, 0.0, 0.0, 1.0]
        sh, _sums = r.bake_probes(ds, probes.moved(pl), 1)
        wide, sv_w = r.relocate_probes(ds, probes, ProbeRelocation(0.25, max_offset=0.9, steps=2))
    finally:
        ds.close()
    assert np.all(sh[1] == 0.0)                                                            # the boxed probe baked black
    E = _lib.probe_irradiance_placed(probes, sh, pl, p, nrm)
    own, T = api.probe_lookup(ProbeGrid((2.0, 1.0, 0.0), (2.0, 1.0, 0.0), (1, 1, 1), False), sh[2:], p, nrm, terms=True)
    ref, Tp, X = api.probe_lookup_placed(probes, sh, pl, p, nrm, terms=True)
    assert X["active"].tolist() == [[False, True]] and X["w"].tolist() == [[0.0, 1.0]]
    assert np.all(np.abs(E.astype(np.float64) - own) <= REF.placed_bound(own, T, None, ProbeGrid.of(probes), None, p, 0.0, pl))
    plain = _lib.probe_irradiance(probes, sh, p, nrm)
    print(f"E placed {E[0]}, probe 2's own {own[0]}, plain {plain[0]}")
    assert np.all(own > 0.0) and np.all(E > plain), (E, plain)
    assert wide[1, 3] == 1.0 and np.abs(wide[1, 0:3]).max() > 0.5 and sv_w[1, 2, 0] == 0.0, (wide, sv_w)


def test_render_probe_lit_with_a_placement_is_its_composition_and_without_it_todays_path():
    torch, dev = _torch()
    scene, r = scenes.config("C2_cornell_box", 16, 16, 4)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    pd = ProbeDepth(8, 6, 800.0)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        pl, _sv = r.relocate_probes(ds, probes, ProbeRelocation(60.0, steps=2))
        assert np.any(pl[:, 0:3] != 0.0)                                                   # cornell's boxes are near some probe
        moved = probes.moved(pl)
        sh, _sums = r.bake_probes(ds, moved, 1)
        moments, _dsums = r.bake_probe_depth(ds, moved, pd, 1)
        aov = ds.aovs(r, 4, out=torch.empty((16 * 16, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        d_sh, d_pl, d_mom = torch.from_numpy(sh).to(dev), torch.from_numpy(pl).to(dev), torch.from_numpy(moments).to(dev)
        grid = ProbeGrid.of(probes, True)
        for vis in (False, True):
            kw = dict(depth=pd, moments=moments, normal_bias=2.0) if vis else {}
            res = r.render_probe_lit(ds, probes, sh, aov_samples=4, placement=pl, **kw)
            E = _lib.probe_irradiance_placed(grid, d_sh, d_pl, aov[:, 8:11], aov[:, 4:7], pd if vis else None, d_mom if vis else None, 2.0)
            want = api.probe_shade_ref(grid, sh, rec, E.cpu().numpy())
            assert np.array_equal(_u32(res.linear), _u32(want)), vis
            ref8, refg, _ = _lib.denoise(want, rec, None, 16, 16, 0, r.settings["gamma"])
            assert np.array_equal(res.rgb8, ref8) and np.array_equal(_u32(res.gamma), _u32(refg)), vis
            # placement=None: the calls of before, bit for bit
            plain = r.render_probe_lit(ds, probes, sh, aov_samples=4, **kw)
            d8, dg, dl = (_lib.probe_shade_vis(grid, d_sh, pd, d_mom, aov, 16, 16, 2.0, r.settings["gamma"]) if vis
                          else _lib.probe_shade(grid, d_sh, aov, 16, 16, r.settings["gamma"]))
            assert np.array_equal(plain.rgb8, d8.cpu().numpy()) and np.array_equal(_u32(plain.linear), _u32(dl.cpu().numpy()))
            assert not np.array_equal(_u32(plain.linear), _u32(res.linear))                # and the placement does change the picture
            # with ao the irradiance comes from fw_probe_irradiance_placed: another picture than without the placement
            ao = api.AmbientOcclusion(50.0, 16)
            lit_ao = r.render_probe_lit(ds, probes, sh, aov_samples=4, placement=pl, ao=ao, **kw)
            assert not np.array_equal(_u32(lit_ao.linear), _u32(r.render_probe_lit(ds, probes, sh, aov_samples=4, ao=ao, **kw).linear))
    finally:
        ds.close()


def test_cli_relocates_bakes_and_lights_a_view(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    from firework_amd.yaml_io import load_scene
    yml = os.path.join(ROOT, "scenes", "three_lights.yml")
    base = ["--scene-file", yml, "-s", "2"]
    bake = ["--bake-probes", "2,2,3", "--probe-min=-12,0.05,-12", "--probe-max", "12,9,12", "--probe-dirs", "32", "--probe-depth", "8"]
    lit = ["--width", "24", "--height", "16", "--aov-samples", "2"]
    placed, without = str(tmp_path / "r.npz"), str(tmp_path / "p.npz")
    assert main(base + bake + ["--probe-relocate", "0.5", "--probe-relocate-steps", "2", "--probe-relocate-max", "0.3", "-o", placed]) == 0
    assert main(base + bake + ["-o", without]) == 0
    with np.load(placed) as z, np.load(without) as z0:
        assert sorted(set(z.files) - set(z0.files)) == ["placement", "relocate_min_front", "relocate_steps"]
        assert np.array_equal(z["positions"], z0["positions"])                            # the nominal positions
        pl = z["placement"]
        assert pl.shape == (12, 4) and pl.dtype == np.float32 and float(z["relocate_min_front"]) == 0.5 and int(z["relocate_steps"]) == 2
        assert np.all(np.abs(pl[:, 0:3]) <= np.float32(0.3) * np.array([24.0, 8.95, 12.0], np.float32) + 1e-6) and set(pl[:, 3].tolist()) <= {0.0, 1.0}
        grid, sh, moments = ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"], True), z["sh"], z["depth"]
        pd = ProbeDepth(8, 6, float(z["depth_max"]))
        # what the command line did, by hand
        cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
        r = api.Renderer.default().width(24).height(16).samples(2).use_bvh(True).camera(cam).seed(0)
        scene = load_scene(yml)
        probes = ProbeSet.grid(z["grid_lo"], z["grid_hi"], tuple(int(c) for c in z["grid_counts"]), 32).seed(0)
        rl = ProbeRelocation(0.5, max_offset=tuple(0.3 * s for s in api.probe_spacing(probes)), steps=2)
        want_pl, _sv = r.relocate_probes(scene, probes, rl)
        assert np.array_equal(_u32(pl), _u32(want_pl))
        want_sh, _s = r.bake_probes(scene, probes.moved(pl), 1)
        assert np.array_equal(_u32(sh), _u32(want_sh))
    png = {name: str(tmp_path / (name + ".png")) for name in ("placed", "ignored")}
    assert main(base + lit + ["--probe-lit", placed, "-o", png["placed"]]) == 0
    assert main(base + lit + ["--probe-lit", placed, "--probe-no-placement", "-o", png["ignored"]]) == 0
    img = {name: np.asarray(Image.open(path).convert("RGB")).reshape(-1, 3) for name, path in png.items()}
    assert np.array_equal(img["placed"], r.render_probe_lit(scene, grid, sh, aov_samples=2, depth=pd, moments=moments, placement=pl).rgb8)
    assert np.array_equal(img["ignored"], r.render_probe_lit(scene, grid, sh, aov_samples=2, depth=pd, moments=moments).rgb8)
