"""The direct light of point, spot and directional lights at surface points on the GPU (fw_direct_rays, fw_direct_reduce, fw_bake_direct,
Renderer.render_direct, Renderer.render_probe_lit and Renderer.bake_lightmap with direct).

k_direct_rays against the numpy float64 statement (api.direct_rays) to one float32 ulp at each vector's scale (§9k's bound) with the zero
entries exactly where the statement has them — the inputs are asserted, on the CPU and before anything runs, to keep every culling
decision 64 ulp from its threshold — over every point and light count, id list, view, spec and stride; k_direct_reduce against
api.direct_reduce within the bound of tests/direct_ref.py — derived from the order of operations, nothing in it measured — over both lobes,
glossy points, hand-made hits at and around t = 1, host and device arrays, pre-filled sums; the bake against the three public calls chained
by hand, bit for bit, for every chunking, progressively, through a medium, with fw_render left as it was; the renderer's own light
samples on the floors of tests/test_gpu_delta_lights.py and tests/test_gpu_ggx.py at those files' own bounds; shadows against their
closed forms; render_direct, render_probe_lit(direct=...) and bake_lightmap(direct=...) against their compositions; the CLI's round
trip."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import (ColorEnv, ConstantTexture, DirectionalLight, DirectLight, LambertianMat, PointLight, ProbeDepth, ProbeGrid,
                              ProbeRadiance, ProbeSet, RenderObject, Scene, SpotLight, Sphere, TriangleMesh)

import ao_ref as AO
import direct_ref as R
import lightmap_ref as LM
import test_gpu_delta_lights as TDL
import test_gpu_ggx as TGX

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
LIGHT_COUNTS = [1, 2, 3, 5, 63, 64, 65, 130, 300]       # every G from 1 to 64, a wave's tail, a wave plus one, strides and a tail; 300 crosses an LDS tile
POINT_COUNTS = [1, 63, 64, 65, 200]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _hits_tensor(hits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.float32).reshape(-1, 12)).to(dev)


def _dev(a, dev, dtype=None):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if dtype is None else a.astype(dtype)).to(dev)


def assert_rays_close(got, ref, what):
    """§9k: per component |gpu - ref| <= 2^-23 x the largest component of that vector in the statement; zero entries exactly where the
    statement has them; every entry finite"""
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.all(np.isfinite(got)), what
    zero_got, zero_ref = np.all(got == 0.0, axis=1), np.all(ref == 0.0, axis=1)
    assert np.array_equal(zero_got, zero_ref), (what, np.argwhere(zero_got != zero_ref)[:4])
    err, bound = np.abs(got.astype(np.float64) - ref.astype(np.float64)), R.ray_bound(ref)
    assert np.all(err <= bound), (what, float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[:4])


def _embedded(pos, nrm, stride):
    """the points inside records of `stride` floats, NaN elsewhere: stride 8 as fw_lightmap_texels lays them out, 12 as fw_render_aovs"""
    if stride == 3:
        return pos.copy(), nrm.copy()
    rec = np.full((pos.shape[0], stride), NAN, np.float32)
    p0, n0 = (0, 4) if stride == 8 else (8, 4)
    rec[:, p0:p0 + 3], rec[:, n0:n0 + 3] = pos, nrm
    return rec[:, p0:p0 + 3], rec[:, n0:n0 + 3]


def _embedded_view(view, as_rays):
    """the view directions alone (stride 3) or inside a ray buffer (rays + 3, stride 6), NaN origins"""
    if not as_rays:
        return view.copy()
    rays = np.full((view.shape[0], 6), NAN, np.float32)
    rays[:, 3:6] = view
    return rays[:, 3:6]


def _device_points(p, q, dev):
    """device tensors of two column ranges of one host array (or of two contiguous arrays), read in place"""
    import torch
    if p.base is None:
        return torch.from_numpy(p).to(dev), torch.from_numpy(q).to(dev)
    d_rec = torch.from_numpy(np.ascontiguousarray(p.base)).to(dev)
    off = lambda a: (a.__array_interface__["data"][0] - p.base.__array_interface__["data"][0]) // 4      # noqa: E731
    return d_rec[:, off(p):off(p) + 3], d_rec[:, off(q):off(q) + 3]


def _device_view(v, dev):
    import torch
    if v is None:
        return None
    if v.base is None:
        return torch.from_numpy(v).to(dev)
    return torch.from_numpy(np.ascontiguousarray(v.base)).to(dev)[:, 3:6]


# ---- fw_direct_rays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ln", LIGHT_COUNTS)
def test_rays_match_the_numpy_statement(Ln):
    torch, dev = _torch()
    rng = np.random.default_rng(Ln)
    lights = R.lights(Ln, rng)
    side = torch.cuda.Stream(device=dev)
    configs = [(POINT_COUNTS[(k + Ln) % 5], stride, ids, view, spec, fv, bias)
               for k, (stride, ids, view, spec, fv, bias) in enumerate([(3, "none", None, False, True, 1e-3), (8, "ascending", "rays", True, True, 0.0),
                                                                        (12, "permuted", "plain", False, False, 0.5), (12, "none", "rays", True, False, 0.0),
                                                                        (8, "permuted", "plain", True, True, 0.25)])]
    assert sorted(c[0] for c in configs) == POINT_COUNTS
    for n, stride, kind, view_kind, with_spec, fv, bias in configs:
        pos, nrm = R.points(n, rng)
        ok = api.ao_usable(pos, nrm)
        ids = {"none": None, "ascending": np.arange(0, n, 2, dtype=np.uint32), "permuted": rng.permutation(n).astype(np.uint32)[:max(1, (2 * n) // 3)]}[kind]
        view = None if view_kind is None else R.views(pos, rng)
        spec = R.specs(n, rng) if with_spec else None
        d = DirectLight(bias, "cosine", fv)
        what = f"Ln {Ln} n {n} stride {stride} ids {kind} view {view_kind} spec {with_spec} face_view {fv} bias {bias}"
        ref, terms = api.direct_rays(d, lights, pos, nrm, ids, view, spec, terms=True)
        assert R.well_clear(terms, lights), what                                          # before anything runs on the device
        m = n if ids is None else ids.size
        p, q = _embedded(pos, nrm, stride)
        v = None if view is None else _embedded_view(view, view_kind == "rays")
        host = _lib.direct_rays(d, lights, p, q, ids, v, spec)
        assert host.shape == (m * Ln, 6)
        assert_rays_close(host, ref, what + " host")
        at = np.arange(n) if ids is None else ids.astype(np.int64)
        assert np.all(host.reshape(m, Ln, 6)[~ok[at]] == 0.0), what
        lit = np.any(host != 0.0, axis=1)
        if n > 1:
            assert 0 < lit.sum() < lit.size, what
        if bias == 0.0:
            assert np.array_equal(_u32(host[lit][:, 0:3]), _u32(np.repeat(pos[at], Ln, axis=0)[lit])), what
        if spec is not None:
            assert np.all(host.reshape(m, Ln, 6)[spec[at, 3] < 0] == 0.0), what
        # device arrays on a side stream into a NaN-filled output: the host call's bits
        d_pos, d_nrm = _device_points(p, q, dev)
        d_ids, d_view, d_spec = _dev(ids, dev, np.int32), _device_view(v, dev), _dev(spec, dev)
        out = torch.full((m * Ln, 6), NAN, dtype=torch.float32, device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            assert _lib.direct_rays(d, lights, d_pos, d_nrm, d_ids, d_view, d_spec, out=out) is out
        side.synchronize()
        assert np.array_equal(_u32(out.cpu().numpy()), _u32(host)), what


def test_rays_on_texel_and_pixel_records_read_in_place():
    torch, dev = _torch()
    # fw_lightmap_texels' records (stride 8) and covered list
    lm = LM.lightmap("overlap", 9, 7, True, "rotated", 4)
    rec, own, n_cov = _lib.lightmap_texels(lm, on_device=True)
    ids = torch.nonzero(own != -1).flatten().to(torch.int32).contiguous()
    assert n_cov == ids.numel() > 10
    lights = R.lights(5, np.random.default_rng(8))
    d = DirectLight(1e-3)
    h = rec.cpu().numpy()
    ref, terms = api.direct_rays(d, lights, h[:, 0:3], h[:, 4:7], ids.cpu().numpy().astype(np.uint32), terms=True)
    assert R.well_clear(terms, lights)
    got = _lib.direct_rays(d, lights, rec[:, 0:3], rec[:, 4:7], ids)
    assert got.is_cuda
    assert_rays_close(got.cpu().numpy(), ref, "texels")
    assert 0 < np.any(ref != 0, axis=1).sum()
    # fw_render_aovs' records (stride 12) with the camera rays as the view (stride 6) on cornell: some pixels miss the scene
    scene, r = scenes.config("C2_cornell_box", 16, 16, 1)
    cam = api.CameraSettings.default().cam_pos((278.0, 278.0, -800.0)).look_at((278.0, 278.0, 0.0)).field_of_view(60.0)
    r = r.camera(cam).seed(4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        aov = ds.aovs(r, 1, out=torch.empty((256, 12), dtype=torch.float32, device=dev))
        rays = torch.from_numpy(ds.camera_rays(r, 0)).to(dev)
    finally:
        ds.close()
    a, v = aov.cpu().numpy(), rays.cpu().numpy()[:, 3:6]
    ref, terms = api.direct_rays(d, TDL.CORNELL_LIGHTS, a[:, 8:11], a[:, 4:7], None, v, terms=True)
    assert R.well_clear(terms, TDL.CORNELL_LIGHTS)
    got = _lib.direct_rays(d, TDL.CORNELL_LIGHTS, aov[:, 8:11], aov[:, 4:7], None, rays[:, 3:6]).cpu().numpy()
    assert_rays_close(got, ref, "pixels")
    missed = a[:, 3] == 0.0
    assert 0 < missed.sum() < 256 and np.all(got.reshape(256, -1, 6)[missed] == 0.0) and np.any(got.reshape(256, -1, 6)[~missed] != 0.0)


# ---- fw_direct_reduce -----------------------------------------------------------------------------------------------------------------
def _reduce_case(Ln, n, lobe, with_spec, rng):
    """points, lights, the statement's rays made well conditioned by hand, hand-made hits"""
    lights = R.lights(Ln, rng)
    pos, nrm = R.points(n, rng)
    view = R.views(pos, rng) if with_spec else None
    spec = R.specs(n, rng) if with_spec else None
    d = DirectLight(1e-3, lobe, True)
    rays = api.direct_rays(d, lights, pos, nrm, None, view, spec)
    rays, spec = R.tame(d, lights, pos, nrm, rays, None, view, spec)
    kind, _rec = api.light_records(lights)
    hits = R.hand_hits(n * Ln, np.tile(kind, n), rng)
    return d, lights, pos, nrm, view, spec, rays, hits


@pytest.mark.parametrize("Ln", LIGHT_COUNTS)
@pytest.mark.parametrize("lobe, with_spec", [("cosine", False), ("renderer", True), ("cosine", True)])
def test_reduce_matches_the_float64_statement(Ln, lobe, with_spec):
    torch, dev = _torch()
    rng = np.random.default_rng(1000 * Ln + 2 * int(with_spec) + (lobe == "renderer"))
    n = 23
    d, lights, pos, nrm, view, spec, rays, hits = _reduce_case(Ln, n, lobe, with_spec, rng)
    assert R.well_conditioned(d, lights, pos, nrm, rays, None, view, spec)                # before anything runs on the device
    ids = rng.permutation(n).astype(np.uint32)[:17]
    rest = np.setdiff1d(np.arange(n), ids)
    at = ids.astype(np.int64)
    sel = (at[:, None] * Ln + np.arange(Ln)[None, :]).reshape(-1)                         # the entries of the listed points, in the list's order
    acc, T, vis = api.direct_reduce(d, lights, pos, nrm, rays[sel], hits["t"][sel], hits["object"][sel], ids, view, spec, terms=True)
    assert np.any(vis) and not np.all(vis)
    if with_spec:
        glossy = spec[at, 3] > 0
        assert np.any(acc[glossy, 4:7] > 0) and np.all(acc[glossy, 0:3] == 0) and np.all(acc[~glossy, 4:7] == 0)
        assert np.all(acc[spec[at, 3] < 0] == 0.0)
    prior = rng.uniform(-2.0, 2.0, size=(n, 8)).astype(np.float32)
    prior[:, 3] = rng.integers(0, 5, size=n)
    prior[rest] = NAN
    sentinel = _u32(prior[:, 7]).copy()
    sums = prior.copy()
    assert _lib.direct_reduce(d, lights, pos, nrm, rays[sel], hits[sel], sums, ids, view, spec) is sums
    bound = R.reduce_bound(acc, T, prior[at, 0:7], Ln)
    err = np.abs(sums[at, 0:7].astype(np.float64) - (prior[at, 0:7].astype(np.float64) + acc))
    print(f"Ln {Ln} lobe {lobe} spec {with_spec}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert np.all(err <= bound), np.argwhere(err > bound)[:4]
    assert np.array_equal(sums[at, 3], prior[at, 3] + acc[:, 3].astype(np.float32))        # N is exact
    assert np.all(np.isnan(sums[rest])) and np.array_equal(_u32(sums[:, 7]), sentinel)     # outside ids, and .w of the second record: untouched
    # two runs are bit-equal; device arrays on a side stream give the host call's bits
    again = prior.copy()
    _lib.direct_reduce(d, lights, pos, nrm, rays[sel], hits[sel], again, ids, view, spec)
    assert np.array_equal(_u32(again), _u32(sums))
    side = torch.cuda.Stream(device=dev)
    d_sums = torch.from_numpy(prior.copy()).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _lib.direct_reduce(d, lights, _dev(pos, dev), _dev(nrm, dev), _dev(rays[sel], dev), _hits_tensor(hits[sel], dev), d_sums, _dev(ids, dev, np.int32),
                           _dev(view, dev), _dev(spec, dev))
    side.synchronize()
    assert np.array_equal(_u32(d_sums.cpu().numpy()), _u32(sums))
    # each point alone equals the point inside the batch
    for k in (0, 5, 16):
        one = prior.copy()
        e = slice(k * Ln, (k + 1) * Ln)
        _lib.direct_reduce(d, lights, pos, nrm, rays[sel][e], hits[sel][e], one, ids[k:k + 1], view, spec)
        assert np.array_equal(_u32(one[at[k]]), _u32(sums[at[k]])), k
        others = np.setdiff1d(np.arange(n), [at[k]])
        assert np.array_equal(_u32(one[others]), _u32(prior[others]))


# ---- fw_bake_direct -------------------------------------------------------------------------------------------------------------------
BAKE_LIGHTS = [PointLight((3.0, 4.0, 1.0), (40.0, 30.0, 20.0)),                                   # above, clear of all three
               SpotLight((-6.0, 1.0, 0.3), (1.0, -0.1, -0.05), (90.0, 80.0, 70.0), 15.0, 35.0),     # behind the medium, shining through it
               DirectionalLight((0.1, -0.2, 1.0), (2.0, 1.5, 1.0))]                                # from behind the quad


def _small_scene(lights=BAKE_LIGHTS):
    """§9s's small scene — a mesh (a tilted quad of two triangles), a sphere and a ConstantMedium under a dim sky — and three lights"""
    scene = Scene.new()
    grey = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, grey)).position(2.5, 0.0, 0.0))
    quad = TriangleMesh.new([[-1.5, -1.0, -3.0], [1.5, -1.0, -3.0], [1.5, 2.0, -2.0], [-1.5, 2.0, -2.0]], [0, 1, 2, 0, 2, 3], None, None, grey)
    scene.add_object(RenderObject.new(quad).position(0.0, 0.0, 0.0))
    scene.add_volume(RenderObject.new(Sphere.new(1.5, grey)).position(-2.5, 0.5, 0.0), 0.8, ConstantTexture.new((1.0, 1.0, 1.0)))
    scene.set_environment(ColorEnv((0.2, 0.2, 0.2)))
    for l in lights:
        scene.add_light(l)
    return scene


def _renderer(use_bvh, seed=11):
    cam = api.CameraSettings.default().cam_pos((0.0, 1.0, 8.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    return api.Renderer.default().width(24).height(16).samples(2).use_bvh(use_bvh).seed(seed).camera(cam)


def _bake_points(n, rng):
    """points between the three occluders with normals in every direction, three of them unusable"""
    pos = rng.uniform(-0.8, 0.8, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    pos[4, 1], nrm[9, 0], nrm[14] = np.nan, np.inf, 0.0
    return pos, nrm


def _chained(ds, d, lights, pos, nrm, ids, view, spec, use_bvh, seed, rounds, first_round=0, sums=None, per_round=None):
    """fw_direct_rays, fw_trace_rays (seed + round, key_base 0) and fw_direct_reduce by hand, on the device over all the points"""
    torch, dev = _torch()
    args = (_dev(pos, dev), _dev(nrm, dev))
    kw = dict(ids=_dev(ids, dev, np.int32), view=_dev(view, dev), spec=_dev(spec, dev))
    if sums is None:
        sums = torch.zeros((pos.shape[0], 8), dtype=torch.float32, device=dev)
    hit_any = miss_any = False
    traced = 0
    for rd in range(first_round, first_round + rounds):
        rays = _lib.direct_rays(d, lights, *args, **kw)
        hits = ds.trace(rays, use_bvh, seed=seed + rd)
        obj = _lib.hit_fields(hits)["object"].cpu().numpy()
        live = np.any(rays.cpu().numpy() != 0.0, axis=1)
        traced += int(live.sum())
        hit_any, miss_any = hit_any or bool(np.any(obj[live] != -1)), miss_any or bool(np.any(obj[live] == -1))
        before = sums.clone()
        _lib.direct_reduce(d, lights, args[0], args[1], rays, hits, sums, **kw)
        if per_round is not None:
            per_round.append((sums - before).cpu().numpy())
    assert hit_any and miss_any
    return sums.cpu().numpy(), traced


@pytest.mark.parametrize("bvh", [False, True])
def test_bake_equals_its_composition_and_is_progressive(bvh):
    torch, dev = _torch()
    n = 37
    rng = np.random.default_rng(2)
    pos, nrm = _bake_points(n, rng)
    view, spec = R.views(pos, rng), R.specs(n, rng)
    ok = api.ao_usable(pos, nrm)
    d = DirectLight(1e-3, "renderer", True)
    bake = dict(seed=11, use_bvh=bvh)
    r = _renderer(bvh)
    ds = _lib.DeviceScene(_small_scene().to_desc())
    try:
        before = ds.render(r)
        rounds = []
        ref, traced = _chained(ds, d, BAKE_LIGHTS, pos, nrm, None, view, spec, bvh, 11, 3, per_round=rounds)
        assert np.all(ref[~ok] == 0.0) and np.any(ref[ok, 0:3] > 0.0) and np.any(ref[ok, 4:7] > 0.0) and np.all(ref[:, 7] == 0.0)
        takes = ok & ~(spec[:, 3] < 0)
        assert np.all(ref[~takes] == 0.0) and np.any(ref[takes, 3] > 0.0) and np.all(ref[:, 3] <= 9.0)      # at most three lights in three rounds
        # the medium makes visibility a draw: the rounds differ — and the composition below still holds
        assert not np.array_equal(_u32(rounds[0]), _u32(rounds[1])) or not np.array_equal(_u32(rounds[1]), _u32(rounds[2]))
        for chunk in (1, 7, 0):
            out, sums, st = ds.bake_direct(d, pos, nrm, None, view, spec, 3, chunk=chunk, **bake)
            assert np.array_equal(_u32(sums), _u32(ref)), (bvh, chunk)
            assert np.array_equal(_u32(out), _u32(api.direct_resolve(ref, 3))), (bvh, chunk)
            assert st["rays"] == traced, (st["rays"], traced, chunk)                       # the non-zero rays
            assert st["n_batches"] >= 3 * (1 if chunk == 0 else -(-n // chunk)) and st["ms_render"] > 0
        assert np.all(out[~ok] == 0.0)
        # progressive: 2 + 1 rounds through sums equal 3 rounds in one call, on the host ...
        out2, sums, _ = ds.bake_direct(d, pos, nrm, None, view, spec, 2, chunk=7, **bake)
        assert np.array_equal(_u32(out2), _u32(api.direct_resolve(sums, 2)))
        out3, sums3, _ = ds.bake_direct(d, pos, nrm, None, view, spec, 1, first_round=2, sums=sums, chunk=1, **bake)
        assert sums3 is sums and np.array_equal(_u32(sums3), _u32(ref)) and np.array_equal(_u32(out3), _u32(api.direct_resolve(ref, 3)))
        # ... and with device tensors on a side stream
        dp = [_dev(a, dev) for a in (pos, nrm, view, spec)]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _o, d_sums, _ = ds.bake_direct(d, dp[0], dp[1], None, dp[2], dp[3], 2, chunk=0, **bake)
            d_out, d_sums2, _ = ds.bake_direct(d, dp[0], dp[1], None, dp[2], dp[3], 1, first_round=2, sums=d_sums, chunk=7, **bake)
        side.synchronize()
        assert d_out.is_cuda and d_sums2 is d_sums
        assert np.array_equal(_u32(d_sums.cpu().numpy()), _u32(ref)) and np.array_equal(_u32(d_out.cpu().numpy()), _u32(api.direct_resolve(ref, 3)))
        # an id list, without view and spec: sums and out are indexed by id, entries outside the list are not touched
        ids = np.random.default_rng(5).permutation(n).astype(np.uint32)[:20]
        plain = DirectLight(0.0, "cosine")
        ref_ids, _ = _chained(ds, plain, BAKE_LIGHTS, pos, nrm, ids, None, None, bvh, 11, 2)
        rest = np.setdiff1d(np.arange(n), ids)
        assert np.all(ref_ids[rest] == 0.0) and np.all(ref_ids[:, 4:] == 0.0)
        for on_device in (False, True):
            s0, o0 = np.zeros((n, 8), np.float32), np.full((n, 8), 7.0, np.float32)
            s0[rest] = NAN
            args = (pos, nrm, ids, s0, o0)
            if on_device:
                args = (dp[0], dp[1], _dev(ids, dev, np.int32), _dev(s0, dev), _dev(o0, dev))
            o, s, _ = ds.bake_direct(plain, args[0], args[1], args[2], None, None, 2, sums=args[3], out=args[4], chunk=7, **bake)
            o, s = (o.cpu().numpy(), s.cpu().numpy()) if on_device else (o, s)
            assert np.array_equal(_u32(s[ids]), _u32(ref_ids[ids])) and np.all(np.isnan(s[rest])), on_device
            assert np.array_equal(_u32(o[ids]), _u32(api.direct_resolve(ref_ids[ids], 2))) and np.all(o[rest] == 7.0), on_device
        # NULL sums at first_round 0 (the C call itself: the Python layer always passes an array): the sums live in the call's scratch
        lib, tp = _lib.load(), A.fw_trace_params()
        tp.use_bvh, tp.seed = int(bvh), 11
        a, raw = d.to_abi(), np.full((n, 8), 7.0, np.float32)
        a.chunk_points = 7
        assert lib.fw_bake_direct(ds.handle, a, tp, n, pos.ctypes.data, nrm.ctypes.data, 3, None, view.ctypes.data, 3, spec.ctypes.data, 0, 3, None,
                                  raw.ctypes.data, None) == A.FW_OK
        assert np.array_equal(_u32(raw), _u32(api.direct_resolve(ref, 3)))
        # timing changes no bit, and the two kernels' time is reported
        _o, sums_t, st = ds.bake_direct(d, pos, nrm, None, view, spec, 3, chunk=7, flags=A.FW_FLAG_TIME_KERNELS, **bake)
        assert np.array_equal(_u32(sums_t), _u32(ref))
        assert st["ms_raygen"] > 0 and st["ms_accumulate"] > 0 and st["ms_render"] >= st["ms_raygen"] + st["ms_accumulate"]
        # fw_render is left as it was
        after = ds.render(r)
        assert np.array_equal(after.rgb8, before.rgb8) and np.array_equal(_u32(after.linear), _u32(before.linear))
        assert after.stats["rays"] == before.stats["rays"]
        # a scene without lights traces nothing, leaves sums as they were and writes out from them
        ds.set_lights([])
        kept = rng.uniform(0.0, 3.0, size=(n, 8)).astype(np.float32)
        for on_device in (False, True):
            s_in = kept.copy() if not on_device else _dev(kept, dev)
            args = (pos, nrm, view, spec) if not on_device else dp
            o, s, st = ds.bake_direct(d, args[0], args[1], None, args[2], args[3], 2, first_round=1, sums=s_in, **bake)
            o, s = (o.cpu().numpy(), s.cpu().numpy()) if on_device else (o, s)
            assert np.array_equal(_u32(s), _u32(kept)) and np.array_equal(_u32(o), _u32(api.direct_resolve(kept, 3))) and st["rays"] == 0
    finally:
        ds.close()


# ---- the renderer's own light samples -------------------------------------------------------------------------------------------------
def _floor_E(light, pts, blocker=None, lobe="renderer"):
    """(out, sums) of fw_bake_direct at the floor points (x, 0, z) of tests/test_gpu_delta_lights.py's floor scene under `light`, normal up,
    bias 0: the renderer's shadow rays start at the hit point itself"""
    scene = TDL._floor_scene(blocker)
    scene.add_light(light)
    pos = np.array([[p[0], 0.0, p[1]] for p in pts], np.float32)
    nrm = np.tile(np.float32(TDL.UP), (len(pts), 1))
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        out, sums, _ = ds.bake_direct(DirectLight(0.0, lobe), pos, nrm, seed=7)
    finally:
        ds.close()
    return out, sums


def _spot_points():
    """test_probe_spot_light's own choice of points, restated: inside the inner cone, in the falloff at t >= 0.3, outside the outer cone"""
    l = TDL.SPOT.to_abi()
    ci, co = float(l.cos_inner), float(l.cos_outer)
    pts = []
    for p in TDL._grid(np.linspace(-6.0, 6.3, 13), np.linspace(-6.2, 6.0, 13)) + [(0.6, 0.3), (0.5, 0.2), (0.7, 0.45), (0.45, 0.4), (0.8, 0.3)]:
        c = TDL.R.spot_cosine(TDL.SPOT, (p[0], 0.0, p[1]))
        if c >= ci + 1e-3 or c <= co - 1e-3 or (c <= ci - 1e-3 and (c - co) / (ci - co) >= 0.3):
            pts.append(p)
    return pts


@pytest.mark.parametrize("name, light, pts", [("point", TDL.POINT, TDL.PROBE_POINTS), ("spot", TDL.SPOT, None), ("directional", TDL.SUN, TDL.PROBE_POINTS)])
def test_lambertian_floor_equals_the_renderers_light_sample(name, light, pts):
    """albedo E(lobe = renderer) / pi is what the path tracer's light sample adds at the floor: the probes of tests/test_gpu_delta_lights.py,
    whose comment derives the relative 1e-5 for exactly these points; zeros agree exactly outside the spot's cone"""
    pts = _spot_points() if pts is None else pts
    got = TDL._probe(light, pts).astype(np.float64)
    out, _ = _floor_E(light, pts)
    mine = np.float64(TDL.ALB) * out[:, 0:3].astype(np.float64) / np.pi
    lit = got.max(axis=1) > 0
    assert lit.sum() >= 30 and np.array_equal(lit, mine.max(axis=1) > 0)
    assert np.all(mine[~lit] == 0.0) and np.all(got[~lit] == 0.0) and np.all(out[~lit, 3] == 0.0) and np.all(out[lit, 3] == 1.0)
    err = np.abs(mine - got)[lit] / got[lit]
    print(f"{name}: {len(pts)} points, {int(lit.sum())} lit, largest relative difference {err.max():.3g}")
    assert np.all(err <= 1e-5)
    if name == "spot":
        assert (~lit).sum() >= 20


def test_lambertian_floor_umbra_is_exactly_dark():
    light = PointLight((0.0, 4.0, 0.0), (9.0, 6.0, 3.0))
    umbra = [(0.0, 0.0), (0.5, 0.3), (-0.7, 0.0), (0.0, 0.9), (-0.6, -0.6)]
    outside = [(1.5, 0.0), (0.0, -1.6), (2.0, 2.0), (-3.0, 1.0), (1.2, 1.2)]
    blocker = ((0.0, 2.0, 0.0), 0.5)
    got = TDL._probe(light, umbra + outside, blocker).astype(np.float64)
    out, _ = _floor_E(light, umbra + outside, blocker)
    lit, _ = _floor_E(light, umbra + outside)
    assert np.all(got[:5] == 0.0) and np.all(out[:5] == 0.0)
    assert np.array_equal(_u32(out[5:]), _u32(lit[5:])) and np.all(out[5:, 3] == 1.0)
    mine = np.float64(TDL.ALB) * out[5:, 0:3].astype(np.float64) / np.pi
    assert np.all(np.abs(mine - got[5:]) <= 1e-5 * got[5:])


@pytest.mark.parametrize("name, light", [("point", TGX.POINT), ("spot", TGX.SPOT), ("directional", TGX.SUN)])
def test_ggx_floor_equals_the_renderers_light_sample(name, light):
    """S at a GgxMat floor is what the path tracer's light sample adds there: tests/test_gpu_ggx.py's test_probes set-up, at that test's own
    bound (f cos's budget per entry, nothing added)"""
    torch, dev = _torch()
    rays, hit = TGX._probe_set()
    scene = TGX._floor_scene()
    scene.add_light(light)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        got = ds.render_rays(rays, TGX.SAMPLES, seed=7).linear.astype(np.float64)
        hits = _lib.hit_fields(ds.trace(torch.from_numpy(rays).to(dev), True, seed=7))
        pos, nrm = hits["point"].contiguous(), hits["normal"].contiguous()
        assert np.all(hits["object"].cpu().numpy() == 0)
        spec = torch.from_numpy(np.tile(np.float32(TGX.F0_FLOOR + (TGX.ROUGH,)), (len(rays), 1))).to(dev)
        out, _, _ = ds.bake_direct(DirectLight(0.0), pos, nrm, None, torch.from_numpy(rays).to(dev)[:, 3:6], spec, seed=7)
    finally:
        ds.close()
    out = out.cpu().numpy()
    want, bud = TGX._want(light, rays, hit)
    lit = want.max(1) > 0
    assert lit.sum() >= 30 and np.all(out[:, 0:3] == 0.0)
    mine = out[:, 4:7].astype(np.float64)
    assert np.all(mine[~lit] == 0.0) and np.all(got[~lit] == 0.0)
    err = np.abs(mine - got)[lit] / want[lit]
    print(f"{name}: {len(want)} probes, {int(lit.sum())} lit, largest relative difference {err.max():.3g}, largest difference / bound {(err / bud[lit, None]).max():.3g}")
    assert np.all(err <= bud[lit, None])


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def _ring(radius, k=8, phase=0.3):
    a = phase + 2.0 * np.pi * np.arange(k) / k
    return [(float(np.float32(radius * np.cos(t))), float(np.float32(radius * np.sin(t)))) for t in a]


def test_a_spheres_shadow_is_the_projected_disc():
    """a sphere of radius R at height a under a point light at height h shadows exactly the floor points inside the cone of tangents:
    N = 0 at 0.9 x the disc's radius, N = 1 at 1.1 x; the device against the statement by the derived bound, the statement — with the
    sphere's hits in float64 — against I cos / d^2 to float64 rounding"""
    Rs, a, h = 0.5, 2.0, 4.0
    I = np.array([9.0, 6.0, 3.0])
    rad = R.shadow_radius(Rs, a, h)
    assert abs(rad - 4.0 * np.tan(np.arcsin(0.25))) < 1e-12
    inside, outside = _ring(0.9 * rad) + [(0.0, 0.0)], _ring(1.1 * rad) + [(3.0, -2.0)]
    pts = inside + outside
    light = PointLight((0.0, h, 0.0), I)
    d = DirectLight(0.0)
    out, sums = _floor_E(light, pts, ((0.0, a, 0.0), Rs), lobe="cosine")
    assert np.all(out[:len(inside)] == 0.0) and np.all(out[len(inside):, 3] == 1.0)
    pos = np.array([[p[0], 0.0, p[1]] for p in pts], np.float32)
    nrm = np.tile(np.float32(TDL.UP), (len(pts), 1))
    rays = api.direct_rays(d, [light], pos, nrm)
    t, obj = AO.sphere_hits(rays, (0.0, a, 0.0), Rs)
    assert np.all(t[obj == 0] < 1.0)                                                       # the sphere is nearer than the light
    acc, T, vis = api.direct_reduce(d, [light], pos, nrm, rays, t, obj, terms=True)
    assert np.array_equal(vis[:, 0], np.arange(len(pts)) >= len(inside))
    err = np.abs(sums[:, 0:7].astype(np.float64) - acc)
    assert np.all(err <= R.reduce_bound(acc, T, np.zeros_like(acc), 1))
    p64 = pos.astype(np.float64)
    d2 = p64[:, 0] ** 2 + h * h + p64[:, 2] ** 2
    closed = I[None, :] * (h / np.sqrt(d2) / d2)[:, None] * vis
    assert np.all(np.abs(acc[:, 0:3] - closed) <= 16 * R.U * closed)


def test_a_sphere_beyond_a_point_light_shadows_nothing_but_does_under_a_directional_light():
    pts = [(0.0, 0.0), (0.2, 0.1), (-0.3, 0.2), (0.0, -0.4), (1.0, 0.0), (0.0, 1.5), (-2.0, 2.0)]
    blocker = ((0.0, 4.0, 0.0), 0.5)                       # above the light: t > 1 on every shadow ray
    light = PointLight((0.0, 2.0, 0.0), (9.0, 6.0, 3.0))
    lit, _ = _floor_E(light, pts, lobe="cosine")
    out, _ = _floor_E(light, pts, blocker, lobe="cosine")
    assert np.all(lit[:, 3] == 1.0) and np.array_equal(_u32(out), _u32(lit))
    p64 = np.array([[p[0], 0.0, p[1]] for p in pts], np.float32).astype(np.float64)
    d2 = p64[:, 0] ** 2 + 4.0 + p64[:, 2] ** 2
    closed = np.array([9.0, 6.0, 3.0])[None, :] * (2.0 / np.sqrt(d2) / d2)[:, None]
    assert np.all(np.abs(out[:, 0:3] - closed) <= 2.0 ** -23 * closed)                     # one float32 rounding of the sum, and float64's
    sun = DirectionalLight((0.0, -1.0, 0.0), (2.0, 1.5, 1.0))
    lit, _ = _floor_E(sun, pts, lobe="cosine")
    out, _ = _floor_E(sun, pts, blocker, lobe="cosine")
    assert np.all(lit[:, 3] == 1.0) and np.all(lit[:, 0:3] == np.float32([2.0, 1.5, 1.0]))
    assert np.all(out[:4] == 0.0)                          # within 0.5 of the axis: the sphere hides the sun
    assert np.array_equal(_u32(out[4:]), _u32(lit[4:]))


# ---- consumers ------------------------------------------------------------------------------------------------------------------------
CLI_CAMERA = dict(cam_pos=(0.0, 30.0, 50.0), look_at=(0.0, 0.0, 0.0), fov=40.0)


def _cli_renderer(w, h, seed=0, samples=2):
    cam = api.CameraSettings.default().cam_pos(CLI_CAMERA["cam_pos"]).look_at(CLI_CAMERA["look_at"]).field_of_view(CLI_CAMERA["fov"])
    return api.Renderer.default().width(w).height(h).samples(samples).use_bvh(True).camera(cam).seed(seed)


def _term_by_hand(ds, r, d, aov):
    """render_direct's chain: the sample-0 camera rays traced for materials and view, fw_bake_direct on the records in place, the frame in
    float32 with numpy"""
    torch, dev = _torch()
    s = r.settings
    rays = torch.from_numpy(ds.camera_rays(r, 0)).to(dev)
    hit = _lib.hit_fields(ds.trace(rays, s["use_bvh"], seed=s["seed"]))
    table = api.material_direct_table(ds._desc)
    mat = np.where(hit["object"].cpu().numpy() == -1, table.shape[0] - 1, hit["material"].cpu().numpy())
    spec = table[mat]
    out, _, st = ds.bake_direct(d, aov[:, 8:11], aov[:, 4:7], None, rays[:, 3:6], torch.from_numpy(spec).to(dev), 1, seed=s["seed"],
                                use_bvh=s["use_bvh"], flags=s["flags"])
    o, rec = out.cpu().numpy(), aov.cpu().numpy()
    v, inv_pi = rec[:, 3:4], np.float32(1.0 / np.pi)
    term = np.where(spec[:, 3:4] > 0, v * o[:, 4:7], rec[:, 0:3] * ((v * o[:, 0:3]) * inv_pi)).astype(np.float32)
    return term, o, spec, rec, st


@pytest.mark.parametrize("yml", ["three_lights.yml", "ggx_lights.yml"])
def test_render_direct_is_aovs_trace_and_bake_chained(yml):
    from firework_amd import yaml_io
    torch, dev = _torch()
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", yml))
    assert len(scene.lights) == 3
    r = _cli_renderer(32, 24)
    d = DirectLight(1e-3, "renderer")
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        res = r.render_direct(ds, d, aov_samples=1)
        assert r.direct_stats["rays"] > 0
        aov = ds.aovs(r, 1, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
        term, o, spec, rec, st = _term_by_hand(ds, r, d, aov)
    finally:
        ds.close()
    assert st["rays"] == r.direct_stats["rays"]
    assert res.linear.dtype == np.float32 and np.array_equal(_u32(res.linear.reshape(-1, 3)), _u32(term))
    ref8, refg, _ = _lib.denoise(term, rec, None, 32, 24, 0, r.settings["gamma"])
    assert np.array_equal(res.rgb8, ref8) and np.array_equal(_u32(res.gamma), _u32(refg))
    assert np.any(term > 0) and np.any(o[:, 3] == 0.0) and np.any(o[:, 3] == 3.0)          # lit pixels, pixels no light reaches, pixels all three reach
    if yml == "ggx_lights.yml":
        assert np.any(spec[:, 3] > 0) and np.any(o[spec[:, 3] > 0, 4:7] > 0)               # the GgxMat spheres show highlights
    missed = rec[:, 3] == 0.0
    if missed.any():
        assert np.all(spec[missed, 3] == -1.0) and np.all(term[missed] == 0.0)


def test_render_probe_lit_with_direct_is_the_plain_frame_plus_the_term():
    from firework_amd import yaml_io
    torch, dev = _torch()
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "ggx_lights.yml"))
    r = _cli_renderer(32, 24)
    s = r.settings
    d = DirectLight(1e-3, "renderer")
    probes = ProbeSet.grid((-24.0, 2.0, -12.0), (24.0, 12.0, 12.0), (2, 1, 2), 64)
    pd, pr = ProbeDepth(8, 6, 80.0), ProbeRadiance(8, 2, (0.2, 0.6))
    ao = api.AmbientOcclusion(6.0, 16, 1).seed(6)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        maps, _rs, sh, _sums = r.bake_probe_radiance(ds, probes, pr, 1, with_sh=True)
        moments, _ds = r.bake_probe_depth(ds, probes, pd, 1)
        placement = api.neutral_placement(probes.n_probes)
        placement[0, 0:3] = (0.5, 0.25, -0.5)
        aov = ds.aovs(r, 2, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
        term, o, spec, rec, _ = _term_by_hand(ds, r, d, aov)
        branches = dict(plain={}, depth=dict(depth=pd, moments=moments, normal_bias=0.5), placed=dict(placement=placement),
                        radiance=dict(radiance=pr, maps=maps), ao=dict(ao=ao, ao_rounds=1))
        for name, kw in branches.items():
            today = r.render_probe_lit(ds, probes, sh, aov_samples=2, **kw)
            none = r.render_probe_lit(ds, probes, sh, aov_samples=2, direct=None, **kw)
            assert np.array_equal(today.rgb8, none.rgb8) and np.array_equal(_u32(today.gamma), _u32(none.gamma)), name
            assert np.array_equal(_u32(today.linear), _u32(none.linear)), name
            res = r.render_probe_lit(ds, probes, sh, aov_samples=2, direct=d, **kw)
            want = (today.linear.reshape(-1, 3) + term).astype(np.float32)
            assert np.array_equal(_u32(res.linear.reshape(-1, 3)), _u32(want)), name
            ref8, refg, _ = _lib.denoise(want, rec, None, 32, 24, 0, s["gamma"])
            assert np.array_equal(res.rgb8, ref8) and np.array_equal(_u32(res.gamma), _u32(refg)), name
            # it differs from today's frame only where E or S is not zero
            differs = np.any(_u32(res.linear.reshape(-1, 3)) != _u32(today.linear.reshape(-1, 3)), axis=1)
            lit = np.any(o[:, 0:3] != 0.0, axis=1) | np.any(o[:, 4:7] != 0.0, axis=1)
            assert differs.any() and not np.any(differs & ~lit), name
    finally:
        ds.close()


def test_bake_lightmap_with_direct_adds_the_irradiance_at_the_texels():
    torch, dev = _torch()
    scene = TDL._floor_scene()
    scene.add_light(TDL.POINT)
    r = api.Renderer.default().samples(2).use_bvh(True).seed(9)
    lm = LM.flat_quad(8, 8, -2.0, -1.5, 2.5, 2.0, y=0.0, u0=0.1, v0=0.15, u1=0.9, v1=0.8, directions=16).seed(5)
    d = DirectLight(1e-3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        today, sums0 = r.bake_lightmap(ds, lm, 2, dilate=2)
        none, sums1 = r.bake_lightmap(ds, lm, 2, dilate=2, direct=None)
        assert np.array_equal(_u32(today), _u32(none)) and np.array_equal(_u32(sums0), _u32(sums1))
        covered = lm.covered().astype(np.int64)
        flat = today.reshape(-1, 4)
        assert 0 < covered.size < 64 and np.all(flat[covered, 0:3] == 0.0) and np.all(flat[covered, 3] == 1.0)      # a black sky: nothing without direct
        lit, sums2 = r.bake_lightmap(ds, lm, 2, dilate=2, direct=d)
        assert np.array_equal(_u32(sums2), _u32(sums0))                                    # the rays' own sums stay
        rec, own, _ = _lib.lightmap_texels(lm, on_device=True)
        ids = torch.nonzero(own != -1).flatten().to(torch.int32).contiguous()
        out, _, _ = ds.bake_direct(d, rec[:, 0:3], rec[:, 4:7], ids, seed=9)
        with pytest.raises(ValueError, match="cosine"):
            r.bake_lightmap(ds, lm, 1, direct=DirectLight(1e-3, "renderer"))
    finally:
        ds.close()
    E, h = out.cpu().numpy(), rec.cpu().numpy()
    assert np.array_equal(covered, ids.cpu().numpy().astype(np.int64))
    # dilation is fw_lightmap_dilate applied by hand to (0 + E, 1) on the covered texels
    image = np.zeros((64, 4), np.float32)
    image[covered, 0:3], image[covered, 3] = E[covered, 0:3], 1.0
    assert np.array_equal(_u32(lit), _u32(api.lightmap_dilate(image.reshape(8, 8, 4), 2)))
    assert np.array_equal(_u32(r.lightmap_direct.reshape(-1, 3)), _u32(E[:, 0:3]))
    # each covered texel is I cos / d^2 at the texel's record: the statement within the derived bound, the closed form to the float32
    # rounding of the stored ray (2^-24 per component, entering 1 / d^2 twice and the cosine once)
    pos, nrm = h[:, 0:3], h[:, 4:7]
    ids32 = covered.astype(np.uint32)
    rays = api.direct_rays(d, [TDL.POINT], pos, nrm, ids32)
    assert np.all(np.any(rays != 0.0, axis=1))
    acc, T, _ = api.direct_reduce(d, [TDL.POINT], pos, nrm, rays, np.zeros(covered.size, np.float32), np.full(covered.size, R.MISS), ids32, terms=True)
    assert np.all(np.abs(E[covered, 0:7].astype(np.float64) - acc) <= R.reduce_bound(acc, T, np.zeros_like(acc), 1))
    o = pos[covered].astype(np.float64) + float(np.float32(1e-3)) * np.array([0.0, 1.0, 0.0])
    to = np.array(TDL.POINT.position, np.float64) - o
    d2 = (to * to).sum(axis=1)
    closed = np.array(TDL.POINT.intensity, np.float64)[None, :] * (to[:, 1] / np.sqrt(d2) / d2)[:, None]
    assert np.all(np.abs(E[covered, 0:3] - closed) <= 2.0 ** -20 * closed)


def test_cli_round_trip(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    from firework_amd import yaml_io
    yml = os.path.join(ROOT, "scenes", "ggx_lights.yml")
    scene = yaml_io.load_scene(yml)
    base = ["--scene-file", yml, "-s", "2"]
    view = ["--width", "24", "--height", "16", "--aov-samples", "2"]
    r = _cli_renderer(24, 16)
    # --direct-light alone
    png = str(tmp_path / "direct.png")
    assert main(base + view + ["--direct-light", "--direct-bias", "0.01", "-o", png]) == 0
    img = np.asarray(Image.open(png).convert("RGB"))
    want = r.render_direct(scene, DirectLight(0.01), 2).rgb8
    assert img.shape == (16, 24, 3) and np.array_equal(img.reshape(-1, 3), want.reshape(-1, 3)) and img.max() > 0 and img.min() == 0
    # --probe-lit with and without --direct-light
    probes_npz = str(tmp_path / "p.npz")
    bake = ["--bake-probes", "2,1,2", "--probe-min=-24,2,-12", "--probe-max", "24,12,12", "--probe-dirs", "64", "--probe-rounds", "1"]
    assert main(base + bake + ["-o", probes_npz]) == 0
    with np.load(probes_npz) as z:
        grid, sh = ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"], True), z["sh"]
    lit, plain = str(tmp_path / "lit.png"), str(tmp_path / "plain.png")
    assert main(base + view + ["--probe-lit", probes_npz, "--direct-light", "-o", lit]) == 0
    assert main(base + view + ["--probe-lit", probes_npz, "-o", plain]) == 0
    a, b = (np.asarray(Image.open(p).convert("RGB")).reshape(-1, 3) for p in (lit, plain))
    assert np.array_equal(a, r.render_probe_lit(scene, grid, sh, aov_samples=2, direct=DirectLight()).rgb8.reshape(-1, 3))
    assert np.array_equal(b, r.render_probe_lit(scene, grid, sh, aov_samples=2).rgb8.reshape(-1, 3)) and not np.array_equal(a, b)
    assert np.all(a.astype(int) >= b.astype(int))                                          # light is only added
    # --bake-lightmap with and without --lightmap-direct
    floor = Scene.new()
    grey = floor.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    mesh = TriangleMesh.new([[-12.0, 0.0, 12.0], [12.0, 0.0, 12.0], [12.0, 0.0, -12.0], [-12.0, 0.0, -12.0]], [0, 1, 2, 0, 2, 3], [[0.0, 1.0, 0.0]] * 4,
                            [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], grey)
    floor.add_object(RenderObject.new(mesh))
    floor.add_object(RenderObject.new(Sphere.new(4.0, grey)).position(0.0, 4.0, 0.0))
    floor.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    floor.add_light(PointLight((6.0, 14.0, 3.0), (900.0, 800.0, 700.0)))
    yml2 = str(tmp_path / "s.yml")
    yaml_io.save_scene(floor, yml2)
    floor = yaml_io.load_scene(yml2)
    assert len(floor.lights) == 1
    base2 = ["--scene-file", yml2, "-s", "1", "--seed", "3"]
    lm_args = ["--bake-lightmap", "0,8,8", "--lightmap-dirs", "16", "--lightmap-rounds", "1"]
    npz, npz0 = str(tmp_path / "lm.npz"), str(tmp_path / "lm0.npz")
    assert main(base2 + lm_args + ["--lightmap-direct", "-o", npz]) == 0
    assert main(base2 + lm_args + ["-o", npz0]) == 0
    with np.load(npz) as z, np.load(npz0) as z0:
        assert sorted(set(z.files) - set(z0.files)) == ["direct"]
        for k in z0.files:
            if k != "irradiance":
                assert np.array_equal(z[k], z0[k]), k
        r2 = api.Renderer.default().samples(1).use_bvh(True).seed(3)
        lm = api.Lightmap.of(floor, 0, 8, 8, 16).seed(3)
        irr, _ = r2.bake_lightmap(floor, lm, 1, 2, direct=DirectLight())
        assert np.array_equal(_u32(z["irradiance"]), _u32(irr)) and np.array_equal(_u32(z["direct"]), _u32(r2.lightmap_direct))
        assert z["direct"].shape == (8, 8, 3) and z["direct"].max() > 0 and z["direct"].min() == 0.0      # open floor, and the sphere's shadow
        assert np.all(z["irradiance"][..., 0:3] >= z0["irradiance"][..., 0:3])
