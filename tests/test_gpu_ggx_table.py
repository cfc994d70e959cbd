"""GPU checks of the GGX albedo table.  fw_ggx_terms against the numpy statement within the bound tests/ggx_table_ref.py
derives — for every quadrature size around the 256-lane stride and every batch size, with the bound's K and the margin of every
wi.z > 0 decision asserted on the CPU before the device is asked — and bit for bit between host arrays and device tensors, between
two runs, and between a pair alone and the pair in its batch.  fw_ggx_table against fw_ggx_terms at the centres, fw_ggx_table_lookup
against numpy, both bit for bit.  fw_probe_shade_split against fw_probe_shade_placed on diffuse pixels and against the float32
statement on the device lookups' own outputs on glossy ones, and its white furnace.  The test the feature exists for: the mean
radiance of the path tracer on a GgxMat floor under a constant environment against the split shade of the same floor, within a
derived tolerance that the glossy shade without the term misses by a factor.  And the layers: render_probe_lit, the CLI, fw_render
left as it was."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import (ColorEnv, GgxMat, GgxTable, ProbeDepth, ProbeGrid, ProbeRadiance, ProbeSet, RenderObject, Scene, Sphere, XZRect)

import ggx_table_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
LOOKUP_N = [1, 63, 64, 65, 200]
TABLES = [(2, 2), (3, 5), (16, 16)]

_cache = {}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_u32(a), _u32(b))


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _table(n_mu, n_rho):
    """the device's table at 16 x 16 samples, baked once and shared"""
    key = (n_mu, n_rho)
    if key not in _cache:
        _cache[key] = _lib.ggx_table((16, 16), n_mu, n_rho)
    return _cache[key]


# ---- fw_ggx_terms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2", R.QUADS)
def test_terms_match_the_float64_statement(m1, m2):
    torch, dev = _torch()
    worst = 0.0
    for n in R.COUNTS:
        mu, rho, replaced = R.pairs(n, 100 + n, m1, m2)
        assert replaced <= R.MAX_REPLACED * n, (n, replaced)                              # at most one pair in ten (the seeds need none)
        AB, bound, info = R.terms_bound(mu, rho, m1, m2)
        assert np.all(info["fit"]) and np.all(info["min_wz"] >= R.WZ_MARGIN)             # every decision is safe before the device is asked
        assert np.all(info["K"] * 2.0 ** -53 < R.K_LIMIT), float(info["K"].max())         # a float32 evaluation cannot pass
        got = _lib.ggx_terms((m1, m2), mu, rho)
        assert got.dtype == np.float32 and got.shape == (n, 2) and np.all(np.isfinite(got))
        err = np.abs(got.astype(np.float64) - AB)
        assert np.all(err <= bound), (n, float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[:4])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(got[~info["ok"]] == 0.0)
        if n >= 12:
            assert np.sum(~info["ok"]) >= 7
        # device tensors on a side stream into NaN-filled outputs; a second run; each pair alone
        out = torch.full((n, 2), NAN, dtype=torch.float32, device=dev)
        d_mu, d_rho = torch.from_numpy(mu).to(dev), torch.from_numpy(rho).to(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _lib.ggx_terms((m1, m2), d_mu, d_rho, out=out, stream=side.cuda_stream)
        assert _same(out.cpu().numpy(), got), n
        assert _same(_lib.ggx_terms((m1, m2), mu, rho), got), n
        for q in range(min(n, 7)):
            assert _same(_lib.ggx_terms((m1, m2), mu[q:q + 1], rho[q:q + 1])[0], got[q]), (n, q)
    print(f"fw_ggx_terms {m1} x {m2}: largest error / bound {worst:.3f}")


# ---- fw_ggx_table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mu,n_rho", TABLES)
def test_table_is_terms_at_the_centres(n_mu, n_rho):
    torch, dev = _torch()
    t = _table(n_mu, n_rho)
    assert t.shape == (n_rho, n_mu, 2) and t.dtype == np.float32
    mu, rho = api.ggx_table_centres(n_mu, n_rho)
    assert _same(t, _lib.ggx_terms((16, 16), mu.reshape(-1), rho.reshape(-1)).reshape(n_rho, n_mu, 2))
    out = torch.full((n_rho, n_mu, 2), NAN, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        _lib.ggx_table(GgxTable(n_mu, n_rho, 16, 16), out=out, stream=side.cuda_stream)
    assert _same(out.cpu().numpy(), t)
    AB, bound, info = R.terms_bound(mu.reshape(-1), rho.reshape(-1), 16, 16)
    if np.all(info["fit"]):                                                             # the centres happen to be fit: the bound holds too
        assert np.all(np.abs(t.reshape(-1, 2).astype(np.float64) - AB) <= bound)
    assert np.all(t >= 0.0) and np.all(t[..., 0] + t[..., 1] <= 1.0 + 1e-6)


# ---- fw_ggx_table_lookup --------------------------------------------------------------------------------------------------------------
def _lookup_points(n, rng):
    mu, rho = rng.uniform(-0.2, 1.2, n).astype(np.float32), rng.uniform(-0.2, 1.2, n).astype(np.float32)
    special = [(0.0, 0.0), (1.0, 1.0), (-5.0, 0.5), (0.5, 7.0), (NAN, 0.5), (0.5, NAN), (INF, 0.5), (0.5, -INF), (1e30, -1e30), (0.5, 0.5)]
    for i in range(min(n - 1, len(special))):
        mu[i + 1], rho[i + 1] = special[i]
    return mu, rho


@pytest.mark.parametrize("n", LOOKUP_N)
def test_lookup_equals_numpy_bit_for_bit(n):
    torch, dev = _torch()
    rng = np.random.default_rng(n)
    wild = (rng.normal(size=(7, 5, 2)) * 10.0 ** rng.integers(-20, 20, size=(7, 5, 2))).astype(np.float32)
    for table in [_table(*s) for s in TABLES] + [wild]:
        mu, rho = _lookup_points(n, rng)
        want = api.ggx_table_lookup(table, mu, rho)
        got = _lib.ggx_table_lookup(table, mu, rho)
        assert _same(got, want), (table.shape, np.argwhere(_u32(got) != _u32(want))[:4])
        out = torch.full((n, 2), NAN, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        with torch.cuda.stream(side):
            _lib.ggx_table_lookup(d(table), d(mu), d(rho), out=out, stream=side.cuda_stream)
        assert _same(out.cpu().numpy(), got)
        bad = ~(np.isfinite(mu) & np.isfinite(rho))
        assert np.all(got[bad] == 0.0)
        # clamping: a point outside [0, 1] reads what the nearest point of the square reads
        inside = _lib.ggx_table_lookup(table, np.clip(np.where(bad, 0.5, mu), 0.0, 1.0).astype(np.float32),
                                       np.clip(np.where(bad, 0.5, rho), 0.0, 1.0).astype(np.float32))
        assert _same(inside[~bad], got[~bad])


# ---- fw_probe_shade_split -------------------------------------------------------------------------------------------------------------
def _points(grid, n, rng):
    """tests/test_gpu_probe_radiance.py's families of points: inside the grid, on a probe, on a face, on an edge, outside a face"""
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
    dirs = rng.normal(size=(n, 3)) * np.array([1.0, 0.25, 5.0])[(np.arange(n) // 3) % 3, None]
    return pts, nrm.astype(np.float32), dirs.astype(np.float32)


@pytest.mark.parametrize("w,h", [(17, 5), (64, 1)])
def test_split_shade_is_the_float32_statement_on_the_lookups_outputs(w, h):
    torch, dev = _torch()
    rng = np.random.default_rng(w)
    n = w * h
    table = _table(16, 16)
    for wrap, depth_res, bias, placed in ((True, 8, 0.05, True), (False, None, 0.0, False)):
        grid = ProbeGrid((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (3, 2, 2), wrap)
        sh = rng.normal(size=(12, 9, 3)).astype(np.float32)
        pr = ProbeRadiance(16)
        maps = rng.uniform(-1.0, 4.0, size=(12, pr.texels, 4)).astype(np.float32)
        pd = None if depth_res is None else ProbeDepth(depth_res, 6, 10.0)
        moments = None
        if depth_res is not None:
            m = rng.uniform(0.2, 3.0, size=(12, depth_res, depth_res))
            moments = np.stack([m, m * m + rng.uniform(0.05, 1.0, size=m.shape)], axis=-1).astype(np.float32)
        neutral = np.tile(np.array([0.0, 0.0, 0.0, 1.0], np.float32), (12, 1))
        placement = None
        if placed:
            placement = neutral.copy()
            placement[:, 0:3] = rng.uniform(-0.1, 0.1, size=(12, 3)) * 0.5
            placement[1::3, 3] = 0.0
        pts, nrm, view = _points(grid, n, rng)
        rec = np.zeros((n, 12), np.float32)
        rec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
        rec[:, 3] = np.array([0.0, 0.25, 1.0], np.float32)[np.arange(n) % 3]
        rec[:, 4:7], rec[:, 8:11] = nrm, pts
        rec[::6, 4:7] = 0.0
        spec = np.empty((n, 4), np.float32)
        spec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
        spec[:, 3] = np.array([0.3, 0.0, 0.05, -1.0, 1.0, NAN, 0.6], np.float32)[np.arange(n) % 7]
        spec[8, 3] = INF                                                                  # glossy, and a roughness no table answers
        view[5], view[12, 1] = 0.0, NAN
        glossy = spec[:, 3] > 0
        gamma = 2.2 if wrap else 1.7
        _d8, _dg, diffuse = _lib.probe_shade_placed(grid, sh, neutral if placement is None else placement, rec, w, h, pd, moments, bias, gamma)
        r, _S, ok = api.probe_glossy_dirs(rec, view)
        Ls = _lib.probe_radiance_lookup(grid, pr, maps, rec[:, 8:11], rec[:, 4:7], r, np.where(glossy, spec[:, 3], np.float32(0.5)).astype(np.float32),
                                        pd, moments, bias, placement)
        mu_f = api.probe_split_mu(rec, view)
        terms = _lib.ggx_table_lookup(table, mu_f, np.where(glossy, spec[:, 3], np.float32(0.5)).astype(np.float32))
        assert np.any(mu_f[glossy] > 0) and np.any(mu_f[glossy] == 0)
        for flags in (0, A.FW_SPLIT_ENERGY):
            want = api.probe_split_ref(rec, spec, view, diffuse, Ls, terms=terms, flags=flags)
            rgb8, gam, lin = _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, w, h, flags, pd, moments, bias, placement, gamma)
            diff = int((_u32(lin) != _u32(want)).any(axis=1).sum())
            assert diff == 0, (flags, diff, np.argwhere(_u32(lin) != _u32(want))[:4])
            assert _same(lin[~glossy], diffuse[~glossy]) and (~glossy).sum() >= 3 * n // 7 - 1
            ref8, refg, _refl = _lib.denoise(want, rec, None, w, h, 0, gamma)
            assert _same(gam, refg) and np.array_equal(rgb8, ref8)
            rays = np.zeros((n, 6), np.float32)
            rays[:, 3:6] = view
            d_rays = torch.from_numpy(rays).to(dev)
            t = lambda a: None if a is None else torch.from_numpy(a).to(dev)      # noqa: E731
            d8, dg, dl = _lib.probe_shade_split(grid, t(sh), pr, t(maps), t(rec), t(spec), d_rays[:, 3:6], t(table), w, h, flags, pd, t(moments), bias,
                                                t(placement), gamma)
            assert np.array_equal(d8.cpu().numpy(), rgb8) and _same(dg.cpu().numpy(), gam) and _same(dl.cpu().numpy(), lin)
        assert not _same(_lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, w, h, 0, pd, moments, bias, placement, gamma)[2],
                         _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, w, h, 1, pd, moments, bias, placement, gamma)[2])


@pytest.mark.parametrize("with_depth", [False, True])
def test_the_glossy_and_the_split_shade_share_one_pixel(with_depth):
    """k_probe_shade_glossy and k_probe_split_shade run one pixel body (shade_glossy_pixel) with two specular terms: on a 16 x 16 image over
    a 2 x 2 x 2 grid with every kind of pixel, each is its own float32 statement bit for bit, and the two agree bit for bit wherever the
    term is not used — the diffuse pixels — and on `linear` wherever it is multiplied by a coverage of zero."""
    rng = np.random.default_rng(7 + with_depth)
    w = h = 16
    n = w * h
    table = _table(16, 16)
    grid = ProbeGrid((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (2, 2, 2), True)
    sh = rng.normal(size=(8, 9, 3)).astype(np.float32)
    pr = ProbeRadiance(8)
    maps = rng.uniform(0.0, 4.0, size=(8, pr.texels, 4)).astype(np.float32)
    pd, moments, bias = None, None, 0.0
    if with_depth:
        pd, bias = ProbeDepth(4, 6, 10.0), 0.05
        m = rng.uniform(0.2, 3.0, size=(8, 4, 4))
        moments = np.stack([m, m * m + rng.uniform(0.05, 1.0, size=m.shape)], axis=-1).astype(np.float32)
    placement = np.tile(np.array([0.0, 0.0, 0.0, 1.0], np.float32), (8, 1))
    pts, nrm, view = _points(grid, n, rng)
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
    rec[:, 3] = np.array([0.0, 0.25, 1.0], np.float32)[np.arange(n) % 3]                 # coverage 0, between, 1
    rec[:, 4:7], rec[:, 8:11] = nrm, pts
    rec[::11, 4:7] = 0.0                                                                  # an unusable normal
    spec = np.empty((n, 4), np.float32)
    spec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
    spec[:, 3] = np.array([0.3, 0.0, 0.05, 1.0, 0.6], np.float32)[np.arange(n) % 5]      # roughness 0: the diffuse branch
    view[5], view[12, 1], view[6], view[13, 2] = 0.0, NAN, 0.0, NAN                       # zero and NaN views at several coverages
    glossy = spec[:, 3] > 0
    for kind in ((rec[:, 3] == 0), (rec[:, 3] == 1), ~np.any(rec[:, 4:7] != 0, axis=1), np.all(view == 0, axis=1), np.any(np.isnan(view), axis=1)):
        assert np.any(kind & glossy), "every kind of pixel on the glossy branch"
    assert np.any(~glossy) and np.any((rec[:, 3] == 0) & ~glossy)
    diffuse = _lib.probe_shade_placed(grid, sh, placement, rec, w, h, pd, moments, bias)[2]
    r, _S, _ok = api.probe_glossy_dirs(rec, view)
    rho = np.where(glossy, spec[:, 3], np.float32(0.5)).astype(np.float32)
    Ls = _lib.probe_radiance_lookup(grid, pr, maps, rec[:, 8:11], rec[:, 4:7], r, rho, pd, moments, bias, placement)
    terms = _lib.ggx_table_lookup(table, api.probe_split_mu(rec, view), rho)
    g8, gg, gl = _lib.probe_shade_glossy(grid, sh, pr, maps, rec, spec, view, w, h, pd, moments, bias, placement)
    assert _same(gl, api.probe_glossy_ref(rec, spec, view, diffuse, Ls))
    for flags in (0, A.FW_SPLIT_ENERGY):
        s8, sg, sl = _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, w, h, flags, pd, moments, bias, placement)
        assert _same(sl, api.probe_split_ref(rec, spec, view, diffuse, Ls, terms=terms, flags=flags)), flags
        assert _same(sl[~glossy], gl[~glossy]) and _same(sg[~glossy], gg[~glossy]) and np.array_equal(s8[~glossy], g8[~glossy])
        assert _same(sl[~glossy], diffuse[~glossy])
        unseen = rec[:, 3] == 0
        assert _same(sl[unseen], gl[unseen]) and np.any(unseen & glossy)
        assert not _same(sl[glossy], gl[glossy])                                          # and elsewhere the two terms differ


def _floor_records(mus, per, c, f0, rho):
    """hand-made records of a floor y = 0 seen along directions of cosine mu, `per` pixels each: (rec, spec, view)"""
    n = len(mus) * per
    rec, spec, view = np.zeros((n, 12), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32)
    rec[:, 0:3], rec[:, 3], rec[:, 5] = 0.5, 1.0, 1.0
    rec[:, 8], rec[:, 10] = np.linspace(0.2, 0.8, n), 0.5
    spec[:, 0:3], spec[:, 3] = f0, rho
    for k, mu in enumerate(mus):
        view[k * per:(k + 1) * per] = (np.sqrt(1.0 - mu * mu), -mu, 0.0)
    return rec, spec, view


def _constant_maps(c):
    grid = ProbeGrid((0.0, -1.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), False)
    pr = ProbeRadiance(8)
    maps = np.empty((8, pr.texels, 4), np.float32)
    maps[..., 0:3], maps[..., 3] = c, 1.0
    return grid, pr, maps, np.zeros((8, 9, 3), np.float32)


def test_white_furnace_on_the_device():
    """constant maps of value c, F0 = 1 and the energy flag give c within 4 float32 ulps at every texel centre of the 16 x 16 table"""
    c = np.float32([0.75, 1.5, 3.0])
    table = _table(16, 16)
    mu, rho = (v.reshape(-1) for v in api.ggx_table_centres(16, 16))
    grid, pr, maps, sh = _constant_maps(c)
    rec, spec, view = _floor_records([0.5], mu.size, c, (1.0, 1.0, 1.0), 0.5)
    view[:, 0], view[:, 1], spec[:, 3] = np.sqrt(1.0 - mu.astype(np.float64) ** 2), -mu, rho
    Ls = _lib.probe_radiance_lookup(grid, pr, maps, rec[:, 8:11], rec[:, 4:7], api.probe_glossy_dirs(rec, view)[0], rho)
    assert np.all(np.abs(Ls - c) <= np.spacing(c))
    lin = _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, mu.size, 1, A.FW_SPLIT_ENERGY)[2]
    assert np.all(np.abs(lin - c) <= 4.0 * np.spacing(c)), float(np.max(np.abs(lin - c) / np.spacing(c)))
    off = _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, mu.size, 1, 0)[2]
    terms = _lib.ggx_table_lookup(table, api.probe_split_mu(rec, view), rho)
    assert _same(off, api.probe_split_ref(rec, spec, view, np.zeros_like(off), Ls, terms=terms)) and np.all(off < lin + 1e-6)


# ---- against the path tracer ------------------------------------------------------------------------------------------------------------
def test_split_shade_agrees_with_the_path_tracer_and_the_glossy_shade_does_not():
    """A large GgxMat floor under ColorEnv(c): a path leaves after one vertex, so a sample is c F k in [0, c] (0 where the path ends) and
    the mean over n = 64 rays x 4096 samples is the albedo times c.  Tolerance: Hoeffding's c sqrt(ln(2 / delta) / (2 n)) at delta =
    1e-9 (0.0064 c) plus 2e-3 c for the table's quadrature; derived, not tuned.  The glossy shade without the term lies outside it at
    rho = 1, mu = 0.9."""
    c, f0 = 2.0, (1.0, 0.5, 0.04)
    mus, per, spp = (0.2, 0.5, 0.9), 64, 4096
    n = per * spp
    tol = c * np.sqrt(np.log(2.0 / 1e-9) / (2.0 * n)) + 2e-3 * c
    assert abs(tol / c - 0.0084) < 1e-4
    table = _lib.ggx_table(GgxTable(64, 64, 128, 128))
    grid, pr, maps, sh = _constant_maps(np.float32([c, c, c]))
    rng = np.random.default_rng(9)
    for rho in (0.3, 1.0):
        scene = Scene.new()
        floor = scene.add_material(GgxMat.new(f0, rho))
        scene.add_object(RenderObject.new(XZRect.new(-1000, 1000, -1000, 1000, 0, floor)))
        scene.set_environment(ColorEnv((c, c, c)))
        rays = np.zeros((len(mus) * per, 6), np.float32)
        for k, mu in enumerate(mus):
            d = np.array([np.sqrt(1.0 - mu * mu), -mu, 0.0])
            hit = np.stack([rng.uniform(-5, 5, per), np.zeros(per), rng.uniform(-5, 5, per)], 1)
            rays[k * per:(k + 1) * per, 0:3], rays[k * per:(k + 1) * per, 3:6] = hit - d * (2.0 / mu), d
        ds = _lib.DeviceScene(scene.to_desc())
        try:
            got = ds.render_rays(rays, spp, seed=5).linear.astype(np.float64).reshape(len(mus), per, 3)
        finally:
            ds.close()
        assert np.all(got > 0.0)                                                         # every ray met the floor and some light came back
        traced = got.mean(axis=1)
        rec, spec, view = _floor_records(mus, 1, c, f0, rho)
        view[:] = rays[::per, 3:6]
        split = _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, view, table, len(mus), 1, 0)[2].astype(np.float64)
        glossy = _lib.probe_shade_glossy(grid, sh, pr, maps, rec, spec, view, len(mus), 1)[2].astype(np.float64)
        for k, mu in enumerate(mus):
            print(f"rho {rho} mu {mu}: path tracer {traced[k]}, split shade {split[k]}, glossy shade {glossy[k]}, |diff| / tol "
                  f"{np.abs(split[k] - traced[k]) / tol}")
        assert np.all(np.abs(split - traced) <= tol), (rho, np.abs(split - traced) / tol)
        if rho == 1.0:
            assert np.all(np.abs(glossy[2, 0:2] - traced[2, 0:2]) > tol) and glossy[2, 0] > 3.0 * traced[2, 0]


# ---- layers -----------------------------------------------------------------------------------------------------------------------------
def test_render_probe_lit_with_a_table_is_its_composition():
    torch, dev = _torch()
    scene, r = scenes.config("C2_cornell_box", 32, 24, 4)
    f0, rho = (0.9, 0.6, 0.3), 0.6
    ggx = scene.add_material(GgxMat.new(f0, rho))
    scene.add_object(RenderObject.new(Sphere.new(80.0, ggx)).position(278.0, 300.0, 278.0))
    scene.add_light(api.PointLight((278.0, 500.0, 278.0), (2e4, 2e4, 2e4)))
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    pr = ProbeRadiance(8, 2)
    gt = GgxTable(16, 8, 16, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        maps, _sums, sh, _sh_sums = r.bake_probe_radiance(ds, probes, pr, 1, with_sh=True)
        aov = ds.aovs(r, 4, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        rays = ds.camera_rays(r, 0)
        hits = ds.trace(rays, r.settings["use_bvh"], seed=r.settings["seed"])
        sphere = (hits["object"] != A.FW_NO_HIT) & (hits["material"] == ggx)
        assert 10 < sphere.sum() < 32 * 24 // 2
        spec = np.zeros((32 * 24, 4), np.float32)
        spec[sphere] = np.float32(f0 + (rho,))
        grid = ProbeGrid.of(probes, True)
        table = _lib.ggx_table(gt)
        plain = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps)
        for energy in (False, True):
            g = GgxTable(16, 8, 16, 16, energy=energy)
            res = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps, ggx_table=g)
            rgb8, gam, lin = _lib.probe_shade_split(grid, sh, pr, maps, rec, spec, rays[:, 3:6], table, 32, 24, g.flags, gamma=r.settings["gamma"])
            assert _same(res.linear, lin) and _same(res.gamma, gam) and np.array_equal(res.rgb8, rgb8), energy
            given = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps, ggx_table=g, table=table)
            assert _same(given.linear, res.linear)
            differs = (_u32(res.linear) != _u32(plain.linear)).any(axis=1)
            assert np.array_equal(differs, sphere), (energy, int(differs.sum()), int(sphere.sum()))
        none = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps, ggx_table=None)
        assert _same(none.linear, plain.linear) and np.array_equal(none.rgb8, plain.rgb8)
        # direct= still adds the same term
        direct = api.DirectLight()
        base = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps, ggx_table=gt)
        lit = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps, ggx_table=gt, direct=direct)
        lit0 = r.render_probe_lit(ds, probes, sh, aov_samples=4, radiance=pr, maps=maps, direct=direct)
        term = r._direct_term(ds, direct, aov, None, torch.from_numpy(rays).to(dev))[0].cpu().numpy()
        assert _same(lit.linear, (base.linear.reshape(-1, 3) + term).astype(np.float32).reshape(lit.linear.shape))
        assert _same(lit0.linear, (plain.linear.reshape(-1, 3) + term).astype(np.float32).reshape(lit0.linear.shape)) and term.max() > 0
        with pytest.raises(ValueError):
            r.render_probe_lit(ds, probes, sh, ggx_table=gt)
    finally:
        ds.close()


def test_cli_round_trip(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    from firework_amd.yaml_io import load_scene
    yml = os.path.join(ROOT, "scenes", "ggx_lights.yml")
    base = ["--scene-file", yml, "-s", "2"]
    bake = ["--bake-probes", "2,1,3", "--probe-min=-24,2,-12", "--probe-max", "24,12,12", "--probe-dirs", "64", "--probe-rounds", "2"]
    lit = ["--width", "24", "--height", "16", "--aov-samples", "2"]
    with_maps, without = str(tmp_path / "r.npz"), str(tmp_path / "p.npz")
    assert main(base + bake + ["--probe-radiance", "16", "--probe-radiance-roughness", "0.15,0.4,0.9", "-o", with_maps]) == 0
    assert main(base + bake + ["-o", without]) == 0
    with np.load(with_maps) as z:
        grid, sh, maps = ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"], True), z["sh"], z["radiance"]
    pr = ProbeRadiance(16, 2, (0.15, 0.4, 0.9))
    png = {name: str(tmp_path / (name + ".png")) for name in ("glossy", "split", "sized", "energy")}
    assert main(base + lit + ["--probe-lit", with_maps, "-o", png["glossy"]]) == 0
    assert main(base + lit + ["--probe-lit", with_maps, "--probe-split-sum", "-o", png["split"]]) == 0
    assert main(base + lit + ["--probe-lit", with_maps, "--probe-split-sum", "16,8", "-o", png["sized"]]) == 0
    assert main(base + lit + ["--probe-lit", with_maps, "--probe-split-sum", "16,8", "--probe-energy", "-o", png["energy"]]) == 0
    img = {name: np.asarray(Image.open(path).convert("RGB")).reshape(-1, 3) for name, path in png.items()}
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(24).height(16).samples(2).use_bvh(True).camera(cam).seed(0)
    scene = load_scene(yml)
    assert np.array_equal(img["split"], r.render_probe_lit(scene, grid, sh, aov_samples=2, radiance=pr, maps=maps, ggx_table=GgxTable()).rgb8)
    assert np.array_equal(img["sized"], r.render_probe_lit(scene, grid, sh, aov_samples=2, radiance=pr, maps=maps, ggx_table=GgxTable(16, 8)).rgb8)
    assert np.array_equal(img["energy"], r.render_probe_lit(scene, grid, sh, aov_samples=2, radiance=pr, maps=maps,
                                                           ggx_table=GgxTable(16, 8, energy=True)).rgb8)
    assert not np.array_equal(img["glossy"], img["split"]) and not np.array_equal(img["sized"], img["energy"])
    assert main(base + lit + ["--probe-lit", without, "--probe-split-sum", "-o", str(tmp_path / "x.png")]) == 2     # no radiance maps in the file


def test_fw_render_is_left_as_it_was():
    scene, r = scenes.config("C2_cornell_box", 32, 32, 4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        before = ds.render(r)
        t = _lib.ggx_table((9, 7), 3, 5)
        _lib.ggx_terms((9, 7), np.float32([0.5]), np.float32([0.5]))
        _lib.ggx_table_lookup(t, np.float32([0.5]), np.float32([0.5]))
        after = ds.render(r)
    finally:
        ds.close()
    assert np.array_equal(before.rgb8, after.rgb8) and np.array_equal(_u32(before.linear), _u32(after.linear))
