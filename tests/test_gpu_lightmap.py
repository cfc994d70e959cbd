"""Lightmaps baked on the GPU (fw_lightmap_texels, fw_lightmap_rays, fw_lightmap_reduce, fw_lightmap_dilate, fw_bake_lightmap;
DESIGN.md §9o).

k_lm_cover's owner map against the numpy statement (api.Lightmap.texels) exactly; k_lm_texels' records and k_lm_rays' rays against the
float64 statements to one float32 ulp at each vector's scale (§9k's bound: both sides round the same float64 expression, whose libm
results differ by a few float64 ulps); k_lm_reduce against api.lightmap_reduce within a bound derived from its construction
(tests/lightmap_ref.py: reduce_bound); k_lm_dilate against api.lightmap_dilate bit for bit; fw_bake_lightmap against its composition
from the public calls bit for bit, for every chunk size, through sums, on a side stream; a furnace, a sky and an occluder against closed
forms; a baked map put back on the mesh as an image texture and seen from above; lights honoured; fw_render left untouched."""
import copy
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import ColorEnv, EmissiveMat, ImageTexture, LambertianMat, Lightmap, RenderObject, Rotor3, Scene, SkyEnv, Sphere, TriangleMesh

import lightmap_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = api.LIGHTMAP_NO_OWNER
DIRECTIONS = [1, 3, 16, 63, 64, 65, 200]        # one entry, below a wave, powers of two, a wave's tail, a wave, a wave plus one, strides and a tail
ROUNDS = [0, 5, (1 << 31) + 3]
SEEDS = [0, 7, 0x1234567800000009]              # the last one exercises the 64-bit seed fold


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _with(r, **settings):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    rr.settings.update(settings)
    return rr


def assert_vectors_close(got, ref, what):
    """per component |gpu - ref| <= 2^-23 x the largest magnitude among that 3-vector's reference components; every entry finite"""
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.all(np.isfinite(got)), what
    g, r = got.astype(np.float64).reshape(-1, 3), ref.astype(np.float64).reshape(-1, 3)
    bound = 2.0 ** -23 * np.abs(r).max(axis=1, keepdims=True)
    err = np.abs(g - r)
    assert np.all(err <= bound), (what, float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[:4])


def assert_records_close(rec, own, lm, what):
    ref_rec, ref_own = lm.texels()
    assert rec.shape == ref_rec.shape and own.shape == ref_own.shape, what
    assert np.array_equal(own.view(np.uint32), ref_own), (what, np.argwhere(own.view(np.uint32) != ref_own)[:4])   # the owner map: exactly
    assert np.array_equal(_u32(rec[:, 3]), ref_own) and np.all(_u32(rec[:, 7]) == 0), what
    assert_vectors_close(np.ascontiguousarray(rec[:, 0:3]), ref_rec[:, 0:3], what + " positions")
    assert_vectors_close(np.ascontiguousarray(rec[:, 4:7]), ref_rec[:, 4:7], what + " normals")


@pytest.mark.parametrize("w,h", [(8, 8), (17, 5), (64, 1)])
def test_owner_map_and_records_match_the_numpy_statement(w, h):
    seen = 0
    for layout in ("quad", "overlap", "shared_edge", "diagonal", "zero_area", "outside"):
        for place in R.placements():
            for normals in (True, False):
                if place not in ("identity", "far") and layout not in ("quad", "outside") and not normals:
                    continue                                            # (every layout, every placement; both normal sources on a few)
                lm = R.lightmap(layout, w, h, normals=normals, placement=place)
                what = f"{w}x{h} {layout} {place} normals {normals}"
                rec, own, n_cov = _lib.lightmap_texels(lm)               # host output: NaN-filled records on the way in
                assert_records_close(rec, own, lm, what + " host")
                assert n_cov == lm.covered().size, what
                d_rec, d_own, d_cov = _lib.lightmap_texels(lm, on_device=True)
                assert_records_close(d_rec.cpu().numpy(), d_own.cpu().numpy(), lm, what + " device")
                assert d_cov == n_cov and np.array_equal(_u32(d_rec.cpu().numpy()), _u32(rec)), what
                seen += n_cov
    assert seen > 0
    # a mesh whose normals cancel covers nothing, and the count says so
    m = R.lightmap("quad", w, h).mesh
    rec, own, n_cov = _lib.lightmap_texels(Lightmap(TriangleMesh(m.verts, m.indicies, np.zeros_like(m.verts), m.uvs, 0), w, h))
    assert n_cov == 0 and np.all(own == NO) and np.all(rec[:, [0, 1, 2, 4, 5, 6, 7]] == 0.0)


@pytest.mark.parametrize("D", DIRECTIONS)
def test_rays_match_the_numpy_statement(D):
    import torch
    dev = torch.device("cuda", 0)
    base = R.lightmap("quad", 8, 8, placement="far", directions=D)
    n = base.covered().size
    assert n == 25
    for rnd in ROUNDS:
        for seed in SEEDS:
            for jitter in (True, False):
                lm = R.lightmap("quad", 8, 8, placement="far", directions=D).seed(seed).jitter(jitter)
                ref = lm.rays(rnd)
                what = f"D {D} round {rnd} seed {seed:#x} jitter {jitter}"
                got = _lib.lightmap_rays(lm, rnd)
                assert got.shape == (n * D, 6)
                assert_vectors_close(got.reshape(-1, 3), ref.reshape(-1, 3), what + " host")
                if seed == 7:                                           # device output, and first > 0: the shift is the texel's own
                    out = torch.full((4 * D, 6), float("nan"), dtype=torch.float32, device=dev)
                    part = _lib.lightmap_rays(lm, rnd, first=3, n=4, out=out).cpu().numpy()
                    assert_vectors_close(part.reshape(-1, 3), ref[3 * D:7 * D].reshape(-1, 3), what + " device from 3")
                    assert np.array_equal(_u32(part), _u32(got[3 * D:7 * D])), what
                    assert np.array_equal(_u32(_lib.lightmap_rays(lm, rnd, first=n - 2, n=2)), _u32(got[(n - 2) * D:])), what
    # bias 0: the origins are the records' positions bit for bit
    lm = R.lightmap("quad", 8, 8, placement="far", directions=D).seed(7).bias(0.0)
    rec, own, _ = _lib.lightmap_texels(lm)
    ids = np.nonzero(own != NO)[0]
    rays = _lib.lightmap_rays(lm, 5)
    assert np.array_equal(_u32(rays[:, :3]), _u32(np.repeat(rec[ids, 0:3], D, axis=0)))
    assert_vectors_close(rays.reshape(-1, 3), lm.rays(5).reshape(-1, 3), "bias 0")
    a = R.lightmap("quad", 8, 8, placement="far", directions=D).seed(7)
    assert not np.array_equal(_lib.lightmap_rays(a, 0), _lib.lightmap_rays(a, 1))
    assert not np.array_equal(_lib.lightmap_rays(a, 0), _lib.lightmap_rays(R.lightmap("quad", 8, 8, placement="far", directions=D).seed(8), 0))
    with pytest.raises(_lib.FireworkError) as e:                         # beyond the covered list
        _lib.lightmap_rays(a, 0, first=n - 1, n=2)
    assert e.value.status == A.FW_ERR_BAD_ARG


def synthetic_accum(n, D, samples, seed):
    """sums of `samples` samples of a radiance with constant, linear-in-j and per-entry noise parts of both signs"""
    rng = np.random.default_rng(seed)
    j = np.arange(D)[None, :, None] / max(1, D - 1)
    L = np.array([0.7, 1.5, 0.2]) + j * np.array([0.5, -0.8, 0.4]) + rng.uniform(-2.0, 2.0, (n, D, 3))
    acc = np.empty((n * D, 4), np.float32)
    acc[:, :3] = (L * samples).astype(np.float32).reshape(-1, 3)
    acc[:, 3] = rng.integers(1, 9, n * D) * samples                      # (segments: not read)
    return acc


@pytest.mark.parametrize("D", DIRECTIONS)
def test_reduce_matches_the_float64_statement(D):
    import torch
    g = 1
    while g < min(D, 64):
        g *= 2
    n = 2 * (64 // g) + 1 if g < 64 else 3                               # not a multiple of the 64 / G texels a wave serves
    n_tex = n + 4
    for S in (1, 7):
        acc = synthetic_accum(n, D, S, 100 * D + S)
        ref = api.lightmap_reduce(acc, S, D)
        T = R.abs_terms(acc, S, D)
        d_acc = torch.from_numpy(acc).cuda()
        # the identity mapping into zero sums: host arrays and device tensors
        got_h = _lib.lightmap_reduce(acc, S, D, np.zeros((n_tex, 4), np.float32))
        got_d = _lib.lightmap_reduce(d_acc, S, D, torch.zeros((n_tex, 4), dtype=torch.float32, device="cuda")).cpu().numpy()
        for got in (got_h, got_d):
            err = np.abs(got[:n, :3].astype(np.float64) - ref)
            bound = R.reduce_bound(ref, T, np.zeros((n, 3)), D)
            assert np.all(err <= bound), (D, S, float((err / bound).max()))
            assert np.all(got[n:] == 0.0) and np.all(got[:, 3] == 0.0)
        assert np.array_equal(_u32(got_h), _u32(got_d))
        again = _lib.lightmap_reduce(d_acc, S, D, torch.zeros((n_tex, 4), dtype=torch.float32, device="cuda")).cpu().numpy()
        assert np.array_equal(_u32(again), _u32(got_d))                                                          # two runs: bit-equal
        # incoming sums are added to, .w is untouched, texels that are not named are untouched; a permuted list permutes the output
        rng = np.random.default_rng(S)
        before = rng.uniform(-3.0, 3.0, (n_tex, 4)).astype(np.float32)
        ids = rng.permutation(n_tex)[:n].astype(np.uint32)
        d_sums = torch.from_numpy(before.copy()).cuda()
        d_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        assert _lib.lightmap_reduce(d_acc, S, D, d_sums, texel_ids=d_ids) is d_sums
        got = d_sums.cpu().numpy()
        err = np.abs(got[ids, :3].astype(np.float64) - (before[ids, :3].astype(np.float64) + ref))
        bound = R.reduce_bound(ref, T, before[ids, :3], D)
        assert np.all(err <= bound), (D, S, float((err / bound).max()))
        assert np.array_equal(_u32(got[ids, :3]), _u32(before[ids, :3] + got_d[:n, :3]))                       # one float32 addition
        assert np.array_equal(_u32(got[:, 3]), _u32(before[:, 3]))
        rest = np.setdiff1d(np.arange(n_tex), ids)
        assert np.array_equal(_u32(got[rest]), _u32(before[rest]))
        h_sums = before.copy()
        _lib.lightmap_reduce(acc, S, D, h_sums, texel_ids=ids)
        assert np.array_equal(_u32(h_sums), _u32(got))


@pytest.mark.parametrize("w,h", [(17, 5), (8, 8)])
def test_dilate_is_the_numpy_statement(w, h):
    import torch
    rng = np.random.default_rng(w * 100 + h)
    masks = [rng.uniform(0.0, 1.0, (h, w)) < 0.2, np.zeros((h, w), bool), np.ones((h, w), bool)]
    one = np.zeros((h, w), bool)
    one[h // 2, 0] = one[0, w - 1] = True                                # sources on the borders: nothing wraps round
    masks.append(one)
    for mask in masks:
        img = np.zeros((h, w, 4), np.float32)
        img[mask, :3] = rng.uniform(-1.0, 4.0, (int(mask.sum()), 3)).astype(np.float32)
        img[mask, 3] = 1.0
        img[~mask, :3] = rng.uniform(5.0, 6.0, (int((~mask).sum()), 3)).astype(np.float32)       # (stale rgb under a = 0 is never a source)
        for passes in (0, 1, 3):
            ref = api.lightmap_dilate(img, passes)
            got_h = _lib.lightmap_dilate(img.copy(), passes)
            got_d = _lib.lightmap_dilate(torch.from_numpy(img.copy()).cuda(), passes).cpu().numpy()
            assert np.array_equal(_u32(got_h), _u32(ref)), (w, h, passes)
            assert np.array_equal(_u32(got_d), _u32(ref)), (w, h, passes)


def bake_quad(D=65):
    """the lightmap of the composition tests: a tilted quad over part of an 8 x 8 map, 42 covered texels"""
    lm = R.flat_quad(8, 8, -1.5, -1.0, 1.5, 1.0, u0=0.05, v0=0.15, u1=0.9, v1=0.9, directions=D)
    lm.placement(RenderObject.new(lm.mesh).rotate(Rotor3.from_rotation_xy(0.3) * Rotor3.from_rotation_yz(-0.2)).position(0.2, 2.5, 0.4))
    return lm.seed(3)


def chained(ds, r, lm, rounds, first_round=0, sums=None):
    """the public calls by hand, on the device, over the whole covered list: (irradiance before dilation, sums, rays traced)"""
    import torch
    s = r.settings
    D = lm.directions
    rec, own, n_cov = _lib.lightmap_texels(lm, on_device=True)
    ids = torch.nonzero(own != -1).reshape(-1).to(torch.int32)
    assert ids.numel() == n_cov
    if sums is None:
        sums = torch.zeros((lm.height, lm.width, 4), dtype=torch.float32, device="cuda")
    traced = 0
    for rnd in range(first_round, first_round + rounds):
        rays = _lib.lightmap_rays(lm, rnd, out=torch.empty((n_cov * D, 6), dtype=torch.float32, device="cuda"))
        res = ds.render_rays(rays, s["samples"], 0, None, seed=s["seed"] + rnd, use_bvh=s["use_bvh"], paths_per_batch=s["paths_per_batch"],
                             flags=s["flags"])
        traced += res.stats["rays"]
        _lib.lightmap_reduce(res.accum, s["samples"], D, sums, texel_ids=ids)
    h_sums = sums.cpu().numpy()
    irr = np.zeros_like(h_sums)
    cov = (own.cpu().numpy().view(np.uint32) != NO).reshape(lm.height, lm.width)
    irr[cov, :3] = (h_sums[cov, :3].astype(np.float64) / float(first_round + rounds)).astype(np.float32)
    irr[cov, 3] = 1.0
    return irr, h_sums, traced


def assert_bake_equals(ds, r, lm, rounds, ref, what):
    irr_ref, sums_ref, traced = ref
    n_cov = lm.covered().size
    for chunk in (1, 7, 0):
        irr, sums = r.bake_lightmap(ds, lm, rounds, dilate=0, chunk=chunk)
        assert np.array_equal(_u32(sums), _u32(sums_ref)), (what, chunk)
        assert np.array_equal(_u32(irr), _u32(irr_ref)), (what, chunk)
        assert r.lightmap_stats["rays"] == traced, (what, chunk)                         # the sum of the chunks'
        assert r.lightmap_stats["n_batches"] >= rounds * (1 if chunk == 0 else -(-n_cov // chunk)) and r.lightmap_stats["ms_render"] > 0


@pytest.mark.parametrize("name,bvh", [("conics", False), ("C3_suzanne", True)])
def test_bake_equals_its_composition(name, bvh):
    import torch
    scene, r = scenes.config(name, 8, 8, 4)
    r = _with(r, use_bvh=bvh, seed=11)
    lm = bake_quad()
    assert lm.covered().size == 42
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ref = chained(ds, r, lm, 3)
        assert ref[2] >= 3 * 42 * 65 * 4 and np.abs(ref[1]).max() > 0 and np.all(ref[1][..., 3] == 0.0)
        assert_bake_equals(ds, r, lm, 3, ref, name)
        # the dilation of the call is fw_lightmap_dilate's, which is the numpy statement
        irr2, _ = r.bake_lightmap(ds, lm, 3, dilate=2, chunk=7)
        assert np.array_equal(_u32(irr2), _u32(api.lightmap_dilate(ref[0], 2)))
        assert np.any(irr2[..., 3] == 0.5) and np.array_equal(irr2[..., 3] == 1.0, ref[0][..., 3] == 1.0)
        # progressive: 1 + 2 rounds through sums equal 3 rounds in one call (host arrays, and the composition's own two calls)
        irr1, sums = r.bake_lightmap(ds, lm, 1, dilate=0, chunk=7)
        c1 = chained(ds, r, lm, 1)
        assert np.array_equal(_u32(sums), _u32(c1[1])) and np.array_equal(_u32(irr1), _u32(c1[0]))
        irr3, sums3 = r.bake_lightmap(ds, lm, 2, dilate=0, first_round=1, sums=sums, chunk=1)
        assert sums3 is sums
        assert np.array_equal(_u32(sums3), _u32(ref[1])) and np.array_equal(_u32(irr3), _u32(ref[0]))
        # device tensors on a side stream
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            d_irr1, d_sums = r.bake_lightmap(ds, lm, 1, dilate=0, on_device=True, chunk=7)
            d_irr, d_sums2 = r.bake_lightmap(ds, lm, 2, dilate=2, first_round=1, sums=d_sums, chunk=0)
        side.synchronize()
        assert d_irr.is_cuda and d_sums2 is d_sums
        assert np.array_equal(_u32(_host(d_sums)), _u32(ref[1])) and np.array_equal(_u32(_host(d_irr)), _u32(irr2))
        assert np.array_equal(_u32(_host(d_irr1)), _u32(c1[0]))
        # timing changes no bit, and the two kernels' time is reported
        t = _with(r, flags=r.settings["flags"] | A.FW_FLAG_TIME_KERNELS)
        _, sums_t = t.bake_lightmap(ds, lm, 3, chunk=7)
        assert np.array_equal(_u32(sums_t), _u32(ref[1]))
        assert t.lightmap_stats["ms_raygen"] > 0 and t.lightmap_stats["ms_accumulate"] > 0
    finally:
        ds.close()


def _tiny_sphere_scene(env):
    """an environment and one 1 mm sphere 1000 units away, so that the scene is not empty"""
    scene = Scene.new()
    m = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(0.001, m)).position(0.3, -1000.0, 0.2))
    scene.set_environment(env)
    return scene


def test_furnace():
    """under a constant environment L every path returns L, so every covered texel's sum is pi L within fw_lightmap_reduce's own float
    bound (reduce_bound of the constant accum: nothing else is rounded), for both walks"""
    L = np.array([2.0, 0.75, 3.5])
    lm = bake_quad(200)
    cov = lm.texels()[1].reshape(8, 8) != NO
    r = api.Renderer.default().samples(1).use_bvh(True).seed(2)
    ds = _lib.DeviceScene(_tiny_sphere_scene(ColorEnv(tuple(L))).to_desc())
    try:
        for bvh in (False, True):
            irr, sums = _with(r, use_bvh=bvh).bake_lightmap(ds, lm, 1, dilate=0)
            L32 = L.astype(np.float32).astype(np.float64)
            acc = np.zeros((200, 4))
            acc[:, :3] = L32
            ref = api.lightmap_reduce(acc, 1, 200)[0]
            bound = R.reduce_bound(ref, R.abs_terms(acc, 1, 200)[0], np.zeros(3), 200)
            err = np.abs(sums[cov][:, :3].astype(np.float64) - np.pi * L32)
            assert np.all(err <= bound + 2.0 ** -50 * np.pi * L32), (bvh, float((err / bound).max()))
            assert np.array_equal(_u32(irr[cov][:, :3]), _u32(sums[cov][:, :3])) and np.all(irr[cov][:, 3] == 1.0) and np.all(irr[~cov] == 0.0)
            assert np.all(sums[~cov] == 0.0)
    finally:
        ds.close()


def test_sky():
    """a sky over a tilted quad whose rays all miss the one small sphere far below: every covered texel's irradiance is the closed form
    pi (h + z) / 2 + (pi / 3)(z - h) n_y within C / D (tests/lightmap_ref.py; the mean of two rounds is within it as each round is), plus the
    float32 steps between the analytic sky and the output: t = 0.5 (y + 1) and (1 - t) h + t z are five float32 roundings of values at most
    max(h, z) <= 1 in the shader, then one rounding of the projection, one addition per round and one division: at most 16 x 2^-24 pi."""
    hor, zen = np.array([1.0, 1.0, 1.0]), np.array([0.5, 0.7, 1.0])
    D, rounds = 256, 2
    lm = bake_quad(D)
    rec, own = lm.texels()
    cov = own != NO
    r = api.Renderer.default().samples(1).use_bvh(True).seed(1)
    ds = _lib.DeviceScene(_tiny_sphere_scene(SkyEnv(tuple(zen), tuple(hor))).to_desc())
    try:
        for k in range(rounds):
            assert np.all(ds.trace(_lib.lightmap_rays(lm, k), True)["object"] == A.FW_NO_HIT)
        irr, sums = r.bake_lightmap(ds, lm, rounds, dilate=0)
    finally:
        ds.close()
    n = rec[cov, 4:7].astype(np.float64)
    want = R.sky_irradiance(hor, zen, n)
    got = irr.reshape(-1, 4)[cov, :3].astype(np.float64)
    for c in range(3):
        alpha, beta = 0.5 * (hor[c] + zen[c]), np.array([0.0, 0.5 * (zen[c] - hor[c]), 0.0])
        bound = np.array([R.closed_form_bound(alpha, beta, v, D) for v in n]) + 16.0 * 2.0 ** -24 * np.pi
        err = np.abs(got[:, c] - want[:, c])
        assert np.all(err <= bound), (c, float((err / bound).max()))
    assert np.abs(got[:, 0] - want[:, 0]).max() > 0.0                     # (a lattice, not the integral: the bound is not vacuous)


@pytest.mark.parametrize("D", [64, 200])
def test_occluder_is_an_exact_count(D):
    """a black sphere of radius R centred at height h on the normal through one texel's centre, under a constant environment L, bias 0: a
    ray meets the sphere iff sin(theta) < R / h, that is u_j < R^2 / h^2, and the u_j are one per cell of width 1 / D — so the texel's
    irradiance is pi L (1 - R^2 / h^2) within 2 pi L / D (one lattice point for the cell, one for a direction rounded across the edge)
    plus fw_lightmap_reduce's float bound"""
    L = np.array([2.0, 0.75, 3.5])
    lm = R.flat_quad(8, 8, 0.0, 0.0, 8.0, 8.0, directions=D).seed(5).bias(0.0)
    rec, own = lm.texels()
    tx, ty = 3, 4
    pos = rec[ty * 8 + tx, 0:3].astype(np.float64)
    assert np.array_equal(pos, [3.5, 0.0, 4.5]) and np.array_equal(rec[ty * 8 + tx, 4:7], [0.0, 1.0, 0.0])
    h, rad = 5.0, 3.0                                                    # R / h = 0.6
    scene = Scene.new()
    black = scene.add_material(LambertianMat.with_color((0.0, 0.0, 0.0)))
    scene.add_object(RenderObject.new(Sphere.new(rad, black)).position(pos[0], pos[1] + h, pos[2]))
    scene.set_environment(ColorEnv(tuple(L)))
    r = api.Renderer.default().samples(2).use_bvh(True).seed(4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        irr, sums = r.bake_lightmap(ds, lm, 3, dilate=0)
    finally:
        ds.close()
    L32 = L.astype(np.float32).astype(np.float64)
    want = np.pi * L32 * (1.0 - rad * rad / (h * h))
    acc = np.zeros((D, 4))
    acc[:, :3] = L32
    # per round: ref and T at most pi L, incoming sums at most 2 pi L; the mean of the rounds' errors is within one round's bound; + the division
    float_bound = R.reduce_bound(np.pi * L32, R.abs_terms(acc, 1, D)[0], 2.0 * np.pi * L32, D) + 2.0 ** -24 * np.pi * L32
    err = np.abs(irr[ty, tx, :3].astype(np.float64) - want)
    assert np.all(err <= 2.0 * np.pi * L32 / D + float_bound), (D, err * D / (np.pi * L32))
    assert np.all(irr[ty, tx, :3] < np.float32(0.9) * np.pi * L32)        # the occluder is seen
    assert np.all(irr[0, 7, :3] > irr[ty, tx, :3])                        # a corner texel sees less of it


def test_round_trip_through_an_image_texture():
    """a 16 x 16 lightmap of a quad on cornell's floor, baked under light sampling, turned into an 8-bit ImageTexture on an emissive copy
    of the quad and seen from above with parallel (orthographic) rays, four per texel: every ray returns its own texel's colour — the uv convention
    checked through the tracer itself"""
    scene, r = scenes.config("C2_cornell_box", 8, 8, 4)
    lm = R.flat_quad(16, 16, 40.0, 60.0, 520.0, 500.0, y=0.0, directions=64).seed(2).bias(0.01)
    r = _with(r, seed=3).light_sampling()
    irr, _ = r.bake_lightmap(scene, lm, 2, dilate=0)
    assert np.all(irr[..., 3] == 1.0) and irr[..., :3].min() > 0.0
    img8 = np.clip(np.floor(irr[..., :3] / irr[..., :3].max() * 255.0 + 0.5), 0, 255).astype(np.uint8)
    assert len(np.unique(img8.reshape(-1, 3), axis=0)) > 64               # the map varies: a transposed or mirrored lookup would show
    assert not np.array_equal(img8, img8[::-1]) and not np.array_equal(img8, img8[:, ::-1]) and not np.array_equal(img8, img8.transpose(1, 0, 2))
    shown = Scene.new()
    mat = shown.add_material(EmissiveMat.new(ImageTexture.new(img8)))
    m = lm.mesh
    shown.add_object(RenderObject.new(TriangleMesh(m.verts, m.indicies, m.normals, m.uvs, mat)))
    shown.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    rec = lm.texels()[0]
    dx, dz = (520.0 - 40.0) / 16 / 4, (500.0 - 60.0) / 16 / 4             # a quarter of a texel
    # parallel rays from above, tilted towards +x: the tracer's triangle test, like the reference's, shears along the direction's SIGNED
    # largest component, which a ray straight down (0, -1, 0) does not have
    view = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    rays, want = [], []
    for ox, oz in ((-dx, -dz), (dx, -dz), (-dx, dz), (dx, dz)):
        o = rec[:, 0:3].astype(np.float64) + np.array([ox - 10.0, 10.0, oz])
        rays.append(np.concatenate([o, np.broadcast_to(view, o.shape)], axis=1))
        want.append(img8.reshape(-1, 3).astype(np.float32) / np.float32(255.0))
    rays, want = np.concatenate(rays).astype(np.float32), np.concatenate(want)
    ds = _lib.DeviceScene(shown.to_desc())
    try:
        res = ds.render_rays(rays, 1, 0, None, seed=1, use_bvh=True, gamma=1.0)
    finally:
        ds.close()
    assert np.array_equal(_u32(res.linear), _u32(want)), np.argwhere(res.linear != want)[:4]


def test_three_lights_bake_with_direct_light():
    from firework_amd import yaml_io
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "three_lights.yml"))
    assert len(scene.lights) > 0
    r = api.Renderer.default().samples(4).use_bvh(True).seed(9)
    lm = R.flat_quad(8, 8, -4.0, -6.0, -0.5, 6.0, y=0.05, directions=65).seed(5)         # a patch on the floor between the lit sphere and the box
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        lit, sums = r.bake_lightmap(ds, lm, 2)
        assert np.all(np.isfinite(lit)) and np.all(lit[..., 3] == 1.0)
        ref = chained(ds, r, lm, 2)
        assert np.array_equal(_u32(sums), _u32(ref[1]))
        ds.set_lights([])
        dark, _ = r.bake_lightmap(ds, lm, 2)
        # the lights reach the map through the lit surfaces its rays meet (a light without area cannot be hit by a ray)
        assert lit[..., :3].sum() > dark[..., :3].sum() and (lit[..., :3] - dark[..., :3]).max() > 0.0
    finally:
        ds.close()


@pytest.mark.parametrize("graph", [None, "1"])
def test_render_untouched(graph):
    """fw_render before and after a bake is bit-identical; under GRAPH its repeated frame is still replayed (bit 31)"""
    scene, r = scenes.config("C2_cornell_box", 48, 32, 4)
    lm = R.flat_quad(8, 8, 40.0, 60.0, 520.0, 500.0, y=1.0, directions=65)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        with _lib.options(GRAPH=graph):
            before = [ds.render(r) for _ in range(3)]
            for chunk in (5, 0):
                r.bake_lightmap(ds, lm, 2, chunk=chunk)
                assert r.lightmap_stats["reserved"] & 0x80000000 == 0
            after = [ds.render(r) for _ in range(2)]
        for a in before[1:] + after:
            assert np.array_equal(a.rgb8, before[0].rgb8)
            assert np.array_equal(_u32(a.linear), _u32(before[0].linear))
            assert a.stats["rays"] == before[0].stats["rays"]
        if graph:
            assert before[2].stats["reserved"] & 0x80000000 and after[1].stats["reserved"] & 0x80000000
    finally:
        ds.close()


def test_a_bad_mesh_is_refused_before_any_launch():
    scene, r = scenes.config("conics", 8, 8, 2)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        good = bake_quad(63)
        first = r.bake_lightmap(ds, good, 1)[1]
        m = good.mesh
        verts = m.verts.copy()
        verts[2, 1] = np.nan
        bad = Lightmap(TriangleMesh(verts, m.indicies, m.normals, m.uvs, 0), 8, 8, 63)
        sums = np.full((8, 8, 4), 7.0, np.float32)
        with pytest.raises(_lib.FireworkError) as e:
            r.bake_lightmap(ds, bad, 1, sums=sums)
        assert e.value.status == A.FW_ERR_BAD_ARG and "vert 2 " in str(e.value)
        assert np.all(sums == 7.0)
        assert np.array_equal(_u32(r.bake_lightmap(ds, good, 1)[1]), _u32(first))         # the next call is unaffected
    finally:
        ds.close()
