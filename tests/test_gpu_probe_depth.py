"""Probe visibility on the GPU (fw_probe_depth_reduce, fw_bake_probe_depth, fw_probe_irradiance_vis, fw_probe_shade_vis,
Renderer.bake_probe_depth, Renderer.render_probe_lit with depth).

k_probe_depth against the numpy float64 statement (api.probe_depth_reduce) within the bound of tests/probe_depth_ref.py — derived from the
order of operations, nothing in it measured — over every chunk boundary of the directions, every texel count per lane, host and device
arrays, a side stream, NaN-filled and pre-filled sums; the bake against the three public calls chained by hand, bit for bit, for every
chunking, progressively, with fw_render left as it was; a probe in a sphere's centre; fw_probe_irradiance_vis against api.probe_lookup_vis
within the derived bound over test_gpu_probe_lookup.py's grids and point families; fw_probe_shade_vis bit for bit on the lookup's own
output; the leak between two rooms closed end to end; render_probe_lit with and without depth; the CLI's round trip."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import (ColorEnv, ConstantTexture, EmissiveMat, LambertianMat, ProbeDepth, ProbeGrid, ProbeSet, RenderObject, Scene, Sphere,
                              TriangleMesh, XZRect, YZRect)

import probe_depth_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
FAR = np.array([3e3, -2e3, 5e3])
# test_gpu_probe_lookup.py's grids: a single probe, one and two flat axes, the smallest full cell, an uneven grid, and two far from the origin
GRIDS = [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)), ((-1.0, 0.0, 0.0), (2.0, 1.0, 1.0), (2, 1, 1)), ((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (1, 3, 2)),
         ((0.0, 0.0, 0.0), (1.0, 2.0, 0.5), (2, 2, 2)), ((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5)),
         (tuple(FAR - 1.0), tuple(FAR + (1.0, 2.0, 0.5)), (2, 2, 2)), (tuple(FAR - (1.5, 0.25, 2.0)), tuple(FAR + (2.0, 1.75, 3.0)), (4, 3, 5))]
COUNTS_N = [1, 63, 64, 65, 200]      # one point, a wave's tail, a wave, a wave plus one, several waves with a tail
DIRECTIONS = [1, 63, 64, 65, 256, 257, 600]     # one ray, around a wave, one staged chunk exactly, one more, two chunks and a tail


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _hits_tensor(hits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.float32).reshape(-1, 12)).to(dev)


# ---- fw_probe_depth_reduce ----------------------------------------------------------------------------------------------------------
def _hand_made(n, D, r_max, rng):
    """rays with directions of length 0.5 .. 2 and hits that miss, lie beyond r_max, sit at t = 0 and in between, in turn"""
    d = rng.normal(size=(n * D, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n * D, 1))
    rays = np.zeros((n * D, 6), np.float32)
    rays[:, :3] = rng.normal(size=(n * D, 3))
    rays[:, 3:] = d
    hits = np.zeros(n * D, _lib.HIT_DTYPE)
    kind = (np.arange(n * D) + rng.integers(4)) % 4
    hits["t"] = rng.uniform(0.001, 0.9 * r_max, size=n * D)
    hits["t"][kind == 1] = 3.0 * r_max
    hits["t"][kind == 2] = 0.0
    hits["object"] = rng.integers(0, 9, size=n * D)
    hits["object"][kind == 0] = A.FW_NO_HIT
    hits["t"][kind == 0] = 0.0                                                           # a miss has every other field 0
    hits["point"], hits["normal"], hits["prim"] = rng.normal(size=(n * D, 3)), rng.normal(size=(n * D, 3)), 5   # never read
    return rays, hits


@pytest.mark.parametrize("res", [4, 8, 32])
def test_reduce_matches_the_float64_statement(res):
    torch, dev = _torch()
    rng = np.random.default_rng(res)
    side = torch.cuda.Stream(device=dev)
    worst = 0.0
    for k in (0, 6):
        pd = ProbeDepth(res, k, 7.5)
        for n in (1, 3):
            for D in DIRECTIONS:
                rays, hits = _hand_made(n, D, 7.5, rng)
                acc, G = api.probe_depth_reduce(pd, rays, hits["t"], hits["object"], D, terms=True)
                assert np.all(acc[..., 2] >= 0) and np.any(acc[..., 2] > 0)
                what = f"R {res} k {k} n {n} D {D}"
                # host arrays into pre-filled sums: .w comes back as it went in
                prior = rng.uniform(-2.0, 2.0, size=(n, res, res, 4)).astype(np.float32)
                host = prior.copy()
                assert _lib.probe_depth_reduce(pd, rays, hits, D, sums=host) is host
                assert np.array_equal(_u32(host[..., 3]), _u32(prior[..., 3])), what
                want = prior[..., :3].astype(np.float64) + acc
                err, bound = np.abs(host[..., :3].astype(np.float64) - want), R.reduce_bound(acc, G, prior[..., :3], D, k)
                worst = max(worst, float((err / bound).max()))
                assert np.all(np.isfinite(host)) and np.all(err <= bound), (what, float((err / bound).max()))
                # device arrays on a side stream give the same bits, and two runs are bit-equal
                d_rays, d_hits = torch.from_numpy(rays).to(dev), _hits_tensor(hits, dev)
                outs = []
                for _ in range(2):
                    d_sums = torch.from_numpy(prior).to(dev)
                    side.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(side):
                        assert _lib.probe_depth_reduce(pd, d_rays, d_hits, D, sums=d_sums) is d_sums
                    side.synchronize()
                    outs.append(d_sums.cpu().numpy())
                assert np.array_equal(_u32(outs[0]), _u32(host)) and np.array_equal(_u32(outs[1]), _u32(host)), what
                assert np.array_equal(_u32(d_rays.cpu().numpy()), _u32(rays))                                     # the inputs are only read
                # NaN-filled sums stay NaN in x, y, z (an addition, not a store) and .w is not written; sums=None starts from zeros
                d_nan = torch.full((n, res, res, 4), NAN, dtype=torch.float32, device=dev)
                d_nan[..., 3] = 3.0
                got = _lib.probe_depth_reduce(pd, d_rays, d_hits, D, sums=d_nan).cpu().numpy()
                assert np.all(np.isnan(got[..., :3])) and np.all(got[..., 3] == 3.0), what
                zero = _lib.probe_depth_reduce(pd, rays, hits, D)
                assert np.all(zero[..., 3] == 0.0)
                err0 = np.abs(zero[..., :3].astype(np.float64) - acc)
                assert np.all(err0 <= R.reduce_bound(acc, G, np.zeros_like(acc), D, k)), what
    print(f"R {res}: largest error / bound {worst:.3f}")


def test_reduce_does_not_depend_on_the_other_probes():
    """a probe's sums are its own rays': reducing three probes at once equals reducing each alone"""
    rng = np.random.default_rng(1)
    pd = ProbeDepth(8, 6, 7.5)
    rays, hits = _hand_made(3, 257, 7.5, rng)
    full = _lib.probe_depth_reduce(pd, rays, hits, 257)
    for p in range(3):
        one = _lib.probe_depth_reduce(pd, rays[p * 257:(p + 1) * 257], hits[p * 257:(p + 1) * 257], 257)
        assert np.array_equal(_u32(one[0]), _u32(full[p])), p


# ---- fw_bake_probe_depth ------------------------------------------------------------------------------------------------------------
def _small_scene():
    """a mesh (a tilted quad of two triangles), a sphere and a ConstantMedium under a dim sky"""
    scene = Scene.new()
    grey = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, grey)).position(2.5, 0.0, 0.0))
    quad = TriangleMesh.new([[-1.5, -1.0, -3.0], [1.5, -1.0, -3.0], [1.5, 2.0, -2.0], [-1.5, 2.0, -2.0]], [0, 1, 2, 0, 2, 3], None, None, grey)
    scene.add_object(RenderObject.new(quad).position(0.0, 0.0, 0.0))
    scene.add_volume(RenderObject.new(Sphere.new(1.5, grey)).position(-2.5, 0.5, 0.0), 0.8, ConstantTexture.new((1.0, 1.0, 1.0)))
    scene.set_environment(ColorEnv((0.2, 0.2, 0.2)))
    return scene


def _renderer(use_bvh, seed=11):
    cam = api.CameraSettings.default().cam_pos((0.0, 1.0, 8.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    return api.Renderer.default().width(24).height(16).samples(2).use_bvh(use_bvh).seed(seed).camera(cam)


def _chained(ds, r, probes, pd, rounds, first_round=0, sums=None):
    """fw_probe_rays, fw_trace_rays (seed + round, key_base 0) and fw_probe_depth_reduce by hand, on the device over the whole set"""
    torch, dev = _torch()
    s = r.settings
    D, n = probes.directions, probes.n_probes
    if sums is None:
        sums = torch.zeros((n, pd.resolution, pd.resolution, 4), dtype=torch.float32, device=dev)
    hit_any = miss_any = False
    for rd in range(first_round, first_round + rounds):
        rays = _lib.probe_rays(probes, rd, out=torch.empty((n * D, 6), dtype=torch.float32, device=dev))
        hits = ds.trace(rays, s["use_bvh"], seed=s["seed"] + rd)
        obj = _lib.hit_fields(hits)["object"].cpu().numpy()
        hit_any, miss_any = hit_any or bool(np.any(obj != -1)), miss_any or bool(np.any(obj == -1))
        _lib.probe_depth_reduce(pd, rays, hits, D, sums=sums)
    assert hit_any and miss_any
    return sums.cpu().numpy()


@pytest.mark.parametrize("bvh", [False, True])
def test_bake_equals_its_composition_and_is_progressive(bvh):
    torch, dev = _torch()
    r = _renderer(bvh)
    probes = ProbeSet([[0.0, 0.5, 0.0], [1.0, 1.5, 1.0], [-2.5, 0.5, 0.0]], 65).seed(3)      # the last one inside the medium
    pd = ProbeDepth(8, 6, 6.0)
    ds = _lib.DeviceScene(_small_scene().to_desc())
    try:
        before = ds.render(r)
        ref = _chained(ds, r, probes, pd, 3)
        assert np.all(ref[..., 3] == 0.0) and np.all(ref[..., 2] > 0.0)
        for chunk in (1, 2, 0):
            moments, sums = r.bake_probe_depth(ds, probes, pd, 3, chunk=chunk)
            assert np.array_equal(_u32(sums), _u32(ref)), (bvh, chunk)
            assert np.array_equal(_u32(moments), _u32(api.probe_depth_moments(pd, ref))), (bvh, chunk)
            st = r.probe_depth_stats
            assert st["rays"] == 3 * 3 * 65 and st["n_batches"] >= 3 * (1 if chunk == 0 else -(-3 // chunk)) and st["ms_render"] > 0
        # progressive: 2 + 1 rounds through sums equal 3 rounds in one call, on the host ...
        m2, sums = r.bake_probe_depth(ds, probes, pd, 2, chunk=2)
        assert np.array_equal(_u32(sums), _u32(_chained(ds, r, probes, pd, 2))) and np.array_equal(_u32(m2), _u32(api.probe_depth_moments(pd, sums)))
        m3, sums3 = r.bake_probe_depth(ds, probes, pd, 1, first_round=2, sums=sums, chunk=1)
        assert sums3 is sums and np.array_equal(_u32(sums3), _u32(ref)) and np.array_equal(_u32(m3), _u32(api.probe_depth_moments(pd, ref)))
        # ... and with device tensors on a side stream
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _m, d_sums = r.bake_probe_depth(ds, probes, pd, 2, on_device=True, chunk=0)
            d_m, d_sums2 = r.bake_probe_depth(ds, probes, pd, 1, first_round=2, sums=d_sums, chunk=2)
        side.synchronize()
        assert d_m.is_cuda and d_sums2 is d_sums
        assert np.array_equal(_u32(d_sums.cpu().numpy()), _u32(ref)) and np.array_equal(_u32(d_m.cpu().numpy()), _u32(api.probe_depth_moments(pd, ref)))
        # the medium draws with the round's seed: another seed gives other sums for the probe inside it
        other, _ = _renderer(bvh, seed=12).bake_probe_depth(ds, probes, pd, 3)
        assert not np.array_equal(_u32(other[2]), _u32(api.probe_depth_moments(pd, ref)[2]))
        # timing changes no bit, and the two kernels' time is reported
        t = _renderer(bvh)
        t.settings["flags"] = t.settings["flags"] | A.FW_FLAG_TIME_KERNELS
        _mt, sums_t = t.bake_probe_depth(ds, probes, pd, 3, chunk=2)
        assert np.array_equal(_u32(sums_t), _u32(ref))
        st = t.probe_depth_stats
        assert st["ms_raygen"] > 0 and st["ms_accumulate"] > 0 and st["ms_render"] >= st["ms_raygen"] + st["ms_accumulate"]
        # fw_render is left as it was
        after = ds.render(r)
        assert np.array_equal(after.rgb8, before.rgb8) and np.array_equal(_u32(after.linear), _u32(before.linear))
        assert after.stats["rays"] == before.stats["rays"]
    finally:
        ds.close()


def test_a_probe_in_the_centre_of_a_sphere():
    """One probe at the centre of a sphere of radius rho < r_max: every traced distance is rho to the tracer's own roundings, and a
    weighted mean cannot leave the range of its inputs — every mu lies within [min_j dist_j, max_j dist_j] of the traced hits and every
    mu2 within the same range squared, widened by the reduction's relative bound (R.reduce_bound over the accumulators, for numerator and
    denominator) and the division's one float32 rounding."""
    rho, D = 2.0, 256
    scene = Scene.new()
    grey = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(rho, grey)).position(1.0, -2.0, 0.5))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    probes = ProbeSet([[1.0, -2.0, 0.5]], D).seed(5)
    pd = ProbeDepth(8, 6, 5.0)
    r = _renderer(True)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = _lib.probe_rays(probes, 0)
        hits = ds.trace(rays, True, seed=r.settings["seed"])
        moments, sums = r.bake_probe_depth(ds, probes, pd, 1)
    finally:
        ds.close()
    assert np.all(hits["object"] == 0)
    d = rays[:, 3:].astype(np.float64)
    dist = hits["t"].astype(np.float64) * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert np.all(np.abs(dist - rho) <= 1e-3 * rho)                                       # the tracer's float32 sphere, not part of the claim
    acc, G = api.probe_depth_reduce(pd, rays, hits["t"], hits["object"], D, terms=True)
    rel = (R.reduce_bound(acc, G, np.zeros_like(acc), D, 6) / acc)[0]                     # (8, 8, 3): A, B, W are all positive
    assert np.all(acc > 0) and np.all(rel < 1e-6)
    up = (1.0 + rel[..., 2]) / (1.0 - rel[..., 2]) * (1.0 + 2.0 ** -23)
    for m, col, lo, hi in ((moments[0, ..., 0], 0, dist.min(), dist.max()), (moments[0, ..., 1], 1, dist.min() ** 2, dist.max() ** 2)):
        widen = (1.0 + rel[..., col]) * up
        assert np.all(m.astype(np.float64) >= lo / widen) and np.all(m.astype(np.float64) <= hi * widen), col
    assert np.array_equal(_u32(moments), _u32(api.probe_depth_moments(pd, sums)))


# ---- fw_probe_irradiance_vis, fw_probe_shade_vis ------------------------------------------------------------------------------------
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
    """mu in 0.2 .. 3 — on both sides of the points' distances to their probes — and mu2 = mu^2 + a variance of 0.05 .. 1"""
    mu = rng.uniform(0.2, 3.0, size=(n_probes, res, res))
    m = np.stack([mu, mu * mu + rng.uniform(0.05, 1.0, size=mu.shape)], axis=-1).astype(np.float32)
    assert np.all(m[..., 1].astype(np.float64) >= m[..., 0].astype(np.float64) ** 2)
    return m


def _assert_within(got, ref, bound, what):
    assert got.dtype == np.float32 and got.shape == ref.shape and np.all(np.isfinite(got)), what
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (what, float((err / bound).max()), np.argwhere(err > bound)[:4])


@pytest.mark.parametrize("lo,hi,counts", GRIDS)
def test_lookup_vis_matches_the_float64_statement(lo, hi, counts):
    torch, dev = _torch()
    rng = np.random.default_rng(sum(counts) * 11 + int(lo[0] > 100))
    n_probes = counts[0] * counts[1] * counts[2]
    sh = rng.normal(size=(n_probes, 9, 3)).astype(np.float32)
    d_sh = torch.from_numpy(sh).to(dev)
    side = torch.cuda.Stream(device=dev)
    for res, wrap, bias in ((8, True, 0.0), (4, False, 0.125), (32, True, 0.3), (16, False, 0.0)):
        grid = ProbeGrid(lo, hi, counts, wrap)
        pd = ProbeDepth(res, 6, 10.0)
        moments = _random_moments(n_probes, res, rng)
        d_mom = torch.from_numpy(moments).to(dev)
        for n in COUNTS_N:
            pts, nrm = _points(grid, n, rng)
            ref, T, X = api.probe_lookup_vis(grid, sh, pd, moments, pts, nrm, bias, terms=True)
            bound = R.vis_bound(ref, T, X, grid, res, pts, bias)
            what = f"{counts} R {res} wrap {wrap} bias {bias} n {n}"
            if n == 200 and n_probes > 1:
                assert np.any(X["v"] == 1.0) and np.any(X["v"] < 0.5), what               # both branches are walked
            # host arrays, stride 3, into a NaN-filled buffer
            host = np.full((n, 3), NAN, np.float32)
            assert _lib.probe_irradiance_vis(grid, sh, pd, moments, pts, nrm, bias, out=host) is host
            _assert_within(host, ref, bound, what + " host")
            # device arrays in place in 48-byte records (stride 12), into a NaN-filled tensor on a side stream
            rec = np.full((n, 12), NAN, np.float32)
            rec[:, 8:11], rec[:, 4:7] = pts, nrm
            d_rec = torch.from_numpy(rec).to(dev)
            out = torch.full((n, 3), NAN, dtype=torch.float32, device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                _lib.probe_irradiance_vis(grid, d_sh, pd, d_mom, d_rec[:, 8:11], d_rec[:, 4:7], bias, out=out)
            side.synchronize()
            assert np.array_equal(_u32(out.cpu().numpy()), _u32(host)), what + " device records"
            # device arrays, stride 3, the current stream
            got = _lib.probe_irradiance_vis(grid, d_sh, pd, d_mom, torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev), bias)
            assert np.array_equal(_u32(got.cpu().numpy()), _u32(host)), what + " device packed"


def test_lookup_vis_is_deterministic_pointwise_and_answers_bad_points_with_zeros():
    rng = np.random.default_rng(5)
    grid = ProbeGrid((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5), True)
    sh = rng.normal(size=(60, 9, 3)).astype(np.float32)
    pd = ProbeDepth(8, 6, 10.0)
    moments = _random_moments(60, 8, rng)
    pts, nrm = _points(grid, 200, rng)
    first = _lib.probe_irradiance_vis(grid, sh, pd, moments, pts, nrm, 0.1)
    assert np.array_equal(_u32(_lib.probe_irradiance_vis(grid, sh, pd, moments, pts, nrm, 0.1)), _u32(first))
    perm = rng.permutation(200)
    assert np.array_equal(_u32(_lib.probe_irradiance_vis(grid, sh, pd, moments, pts[perm], nrm[perm], 0.1)), _u32(first[perm]))
    assert not np.array_equal(_u32(first), _u32(_lib.probe_irradiance(grid, sh, pts, nrm)))          # the moments matter
    bad_p, bad_n = pts.copy(), nrm.copy()
    bad_p[3, 1], bad_p[64, 0], bad_n[65] = NAN, np.inf, 0.0
    bad_n[130, 2] = NAN
    got = _lib.probe_irradiance_vis(grid, sh, pd, moments, bad_p, bad_n, 0.1)
    bad = np.zeros(200, bool)
    bad[[3, 64, 65, 130]] = True
    assert np.all(_u32(got[bad]) == 0) and np.array_equal(_u32(got[~bad]), _u32(first[~bad]))
    # moments of any content — NaN, infinities, negative — are read inside the arrays and give an answer for every point
    wild = moments.copy()
    wild.reshape(-1)[::7] = NAN
    wild.reshape(-1)[3::11] = np.inf
    wild.reshape(-1)[5::13] = -4.0
    assert _lib.probe_irradiance_vis(grid, sh, pd, wild, pts, nrm, 0.1).shape == (200, 3)


@pytest.mark.parametrize("w,h", [(17, 5), (64, 1)])
def test_shade_vis_is_the_float32_statement_on_the_lookups_output(w, h):
    torch, dev = _torch()
    rng = np.random.default_rng(w)
    n = w * h
    for wrap, bias in ((True, 0.05), (False, 0.0)):
        grid = ProbeGrid((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (3, 2, 2), wrap)
        sh = rng.normal(size=(12, 9, 3)).astype(np.float32)
        pd = ProbeDepth(8, 6, 10.0)
        moments = _random_moments(12, 8, rng)
        pts, nrm = _points(grid, n, rng)
        rec = np.zeros((n, 12), np.float32)
        rec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
        rec[:, 3] = np.array([0.0, 0.25, 1.0], np.float32)[np.arange(n) % 3]
        rec[:, 4:7], rec[:, 8:11] = nrm, pts
        rec[::6, 4:7] = 0.0                                                               # a zero normal on every other coverage-0 record
        E = _lib.probe_irradiance_vis(grid, sh, pd, moments, rec[:, 8:11], rec[:, 4:7], bias)
        assert np.any(E[rec[:, 3] > 0] < 0.0) and np.any(E[rec[:, 3] > 0] > 0.0)          # some lookups are clamped, some are not
        want = api.probe_shade_ref(grid, sh, rec, E)
        gamma = 2.2 if wrap else 1.7
        rgb8, gam, lin = _lib.probe_shade_vis(grid, sh, pd, moments, rec, w, h, bias, gamma)
        assert np.array_equal(_u32(lin), _u32(want))
        ref8, refg, _refl = _lib.denoise(want, rec, None, w, h, 0, gamma)                  # resolve_pixel(out, 1, gamma), as fw_denoise writes it
        assert np.array_equal(_u32(gam), _u32(refg)) and np.array_equal(rgb8, ref8)
        d8, dg, dl = _lib.probe_shade_vis(grid, torch.from_numpy(sh).to(dev), pd, torch.from_numpy(moments).to(dev), torch.from_numpy(rec).to(dev),
                                          w, h, bias, gamma)
        assert np.array_equal(d8.cpu().numpy(), rgb8) and np.array_equal(_u32(dg.cpu().numpy()), _u32(gam)) and np.array_equal(_u32(dl.cpu().numpy()), _u32(lin))
        only8 = _lib.probe_shade_vis(grid, sh, pd, moments, rec, w, h, bias, gamma, outputs=("rgb8",))
        assert only8[1] is None and only8[2] is None and np.array_equal(only8[0], rgb8)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _two_rooms():
    """a black environment; an emissive sphere at x = -2; a Lambertian wall at x = 1 and a Lambertian floor at y = -1, both +-1000 wide"""
    scene = Scene.new()
    white = scene.add_material(LambertianMat.with_color((0.7, 0.7, 0.7)))
    lamp = scene.add_material(EmissiveMat.with_color((20.0, 16.0, 12.0)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, lamp)).position(-2.0, 0.0, 0.0))
    scene.add_object(RenderObject.new(YZRect.new(-1000.0, 1000.0, -1000.0, 1000.0, 1.0, white)))
    scene.add_object(RenderObject.new(XZRect.new(-1000.0, 1000.0, -1000.0, 1000.0, -1.0, white)))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    return scene


def test_visibility_closes_the_leak_through_a_wall():
    """Probes at x = 0 (with the lamp) and x = 4 (behind the wall), R = 8, k = 6, D = 256.  At the floor point (2, -1, 0) in the dark room
    fw_probe_irradiance blends half of the lit probe in: E_wrap > 0 is the leak.  The condition: fw_probe_irradiance_vis gives at most
    1e-2 of E_wrap per channel (the weight share alone is below 1e-9 by tests/test_probe_depth_cpu.py; the rest is the dark probe's own
    irradiance, which the wall keeps at zero here)."""
    probes = ProbeSet.grid((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (2, 1, 1), 256).seed(2)
    pd = ProbeDepth(8, 6, 10.0)
    r = _renderer(True, seed=4)
    r.samples(16)
    ds = _lib.DeviceScene(_two_rooms().to_desc())
    try:
        sh, _sums = r.bake_probes(ds, probes, 1)
        moments, _dsums = r.bake_probe_depth(ds, probes, pd, 1)
    finally:
        ds.close()
    p, nrm = np.array([[2.0, -1.0, 0.0]], np.float32), np.array([[0.0, 1.0, 0.0]], np.float32)
    E_wrap = _lib.probe_irradiance(probes, sh, p, nrm)[0]
    E_vis = _lib.probe_irradiance_vis(probes, sh, pd, moments, p, nrm)[0]
    own = _lib.probe_irradiance(ProbeGrid((4.0, 0.0, 0.0), (4.0, 0.0, 0.0), (1, 1, 1)), sh[1:], p, nrm)[0]
    print(f"E_wrap {E_wrap}, E_vis {E_vis}, the dark probe's own {own}")
    assert np.all(E_wrap > 0.0)
    assert np.all(np.abs(E_vis) <= 1e-2 * E_wrap), (E_vis, E_wrap)
    # on the lit side of the wall the visibility takes nothing away: at (0.5, -1, 0) the lit probe keeps the weight
    q = np.array([[0.5, -1.0, 0.0]], np.float32)
    lit_own = _lib.probe_irradiance(ProbeGrid((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1, 1, 1)), sh[:1], q, nrm)[0]
    lit_vis = _lib.probe_irradiance_vis(probes, sh, pd, moments, q, nrm)[0]
    assert np.all(np.abs(lit_vis - lit_own) <= 0.01 * np.abs(lit_own) + 1e-2 * E_wrap), (lit_vis, lit_own)


def test_render_probe_lit_with_depth_is_its_composition_and_without_it_todays_path():
    torch, dev = _torch()
    scene, r = scenes.config("C2_cornell_box", 32, 24, 4)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    pd = ProbeDepth(8, 6, 800.0)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sh, _sums = r.bake_probes(ds, probes, 1)
        moments, _dsums = r.bake_probe_depth(ds, probes, pd, 1)
        aov = ds.aovs(r, 4, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        d_sh = torch.from_numpy(sh).to(dev)
        for wrap in (True, False):
            grid = ProbeGrid.of(probes, wrap)
            for bias in (0.0, 2.0):
                res = r.render_probe_lit(ds, probes, sh, aov_samples=4, wrap=wrap, depth=pd, moments=moments, normal_bias=bias)
                E = _lib.probe_irradiance_vis(grid, d_sh, pd, torch.from_numpy(moments).to(dev), aov[:, 8:11], aov[:, 4:7], bias)
                want = api.probe_shade_ref(grid, sh, rec, E.cpu().numpy())
                assert np.array_equal(_u32(res.linear), _u32(want)), (wrap, bias)
                ref8, refg, _ = _lib.denoise(want, rec, None, 32, 24, 0, r.settings["gamma"])
                assert np.array_equal(res.rgb8, ref8) and np.array_equal(_u32(res.gamma), _u32(refg)), (wrap, bias)
            # without depth: the calls of before, bit for bit
            plain = r.render_probe_lit(ds, probes, sh, aov_samples=4, wrap=wrap)
            E0 = _lib.probe_irradiance(grid, d_sh, aov[:, 8:11], aov[:, 4:7])
            want0 = api.probe_shade_ref(grid, sh, rec, E0.cpu().numpy())
            assert np.array_equal(_u32(plain.linear), _u32(want0)), wrap
            d8, dg, dl = _lib.probe_shade(grid, d_sh, aov, 32, 24, r.settings["gamma"])
            assert np.array_equal(plain.rgb8, d8.cpu().numpy()) and np.array_equal(_u32(plain.gamma), _u32(dg.cpu().numpy()))
            assert not np.array_equal(_u32(plain.linear), _u32(res.linear))                # and the depth does change the picture
        with pytest.raises(ValueError):
            r.render_probe_lit(ds, probes, sh, depth=pd)
    finally:
        ds.close()


def test_cli_bakes_depth_and_lights_a_view_with_and_without_it(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    from firework_amd.yaml_io import load_scene
    yml = os.path.join(ROOT, "scenes", "three_lights.yml")
    base = ["--scene-file", yml, "-s", "2"]
    bake = ["--bake-probes", "2,1,3", "--probe-min=-12,1,-12", "--probe-max", "12,9,12", "--probe-dirs", "32", "--probe-rounds", "2"]
    lit = ["--width", "24", "--height", "16", "--aov-samples", "2"]
    with_depth, without = str(tmp_path / "d.npz"), str(tmp_path / "p.npz")
    assert main(base + bake + ["--probe-depth", "8", "-o", with_depth]) == 0
    assert main(base + bake + ["-o", without]) == 0
    with np.load(with_depth) as z, np.load(without) as z0:
        assert "depth" not in z0.files and sorted(set(z.files) - set(z0.files)) == ["depth", "depth_max", "depth_res", "depth_sharpness"]
        for k in z0.files:
            assert np.array_equal(z[k], z0[k]), k                                         # the depth bake leaves the SH bake as it was
        assert z["depth"].shape == (6, 8, 8, 2) and z["depth"].dtype == np.float32 and int(z["depth_res"]) == 8 and int(z["depth_sharpness"]) == 6
        diagonal = np.float32(np.sqrt(24.0 ** 2 + 8.0 ** 2 + 24.0 ** 2))
        assert z["depth_max"].dtype == np.float32 and float(z["depth_max"]) == float(diagonal)
        grid, sh, moments = ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"], True), z["sh"], z["depth"]
        pd = ProbeDepth(8, 6, float(z["depth_max"]))
    png = {name: str(tmp_path / (name + ".png")) for name in ("vis", "novis", "plain")}
    assert main(base + lit + ["--probe-lit", with_depth, "--probe-normal-bias", "0.5", "-o", png["vis"]]) == 0
    assert main(base + lit + ["--probe-lit", with_depth, "--probe-no-visibility", "-o", png["novis"]]) == 0
    assert main(base + lit + ["--probe-lit", without, "-o", png["plain"]]) == 0
    img = {name: np.asarray(Image.open(path).convert("RGB")).reshape(-1, 3) for name, path in png.items()}
    assert np.array_equal(img["novis"], img["plain"])                                      # byte for byte the image of a file without depth
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(24).height(16).samples(2).use_bvh(True).camera(cam).seed(0)
    scene = load_scene(yml)
    assert np.array_equal(img["vis"], r.render_probe_lit(scene, grid, sh, aov_samples=2, depth=pd, moments=moments, normal_bias=0.5).rgb8)
    assert np.array_equal(img["plain"], r.render_probe_lit(scene, grid, sh, aov_samples=2).rgb8)
    assert not np.array_equal(img["vis"], img["plain"])
