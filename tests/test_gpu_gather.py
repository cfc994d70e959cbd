"""The final gather on the GPU (fw_hit_surface, fw_gather_reduce, fw_bake_gather).

k_hit_surface against the CPU oracle's texture and environment lookups at the hit's own (u, v, point) and the float32 statement of normal,
distance and kind, bit for bit, over every material and texture kind, misses, flipped normals, rays that are never traced and hit records
that name nothing in the scene; k_gather_reduce against api.gather_reduce bit for bit (the statement has only +, x, a comparison and one
rounding: every operation is IEEE-determined); the bake against the public calls chained by hand, bit for bit, for every chunking, every
form of the probe lookup, progressively, with the delta lights, with fw_render left as it was; and five known answers."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, yaml_io
from firework_amd.api import (AmbientOcclusion, ColorEnv, DirectLight, EmissiveMat, FinalGather, LambertianMat, ProbeDepth, RenderObject, Scene,
                              Sphere, XYRect, XZRect, YZRect)

import gather_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DIRECTIONS = [1, 3, 63, 64, 65, 200]            # one ray, below a wave, a wave's tail, a wave, a wave plus one, strides and a tail
u32 = R.u32


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _hits_tensor(hits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.float32).reshape(-1, 12)).to(dev)


# ---- fw_hit_surface -----------------------------------------------------------------------------------------------------------------
def _at_least_five(scene, rays, material, hit, normal):
    """the condition of the surface test on a trace's result (the oracle's or the device's): every material kind, every texture kind,
    misses and normals that face away from their ray occur at least five times; returns the counts"""
    kinds = np.array([{"LambertianMat": 0, "MetalMat": 1, "DielectricMat": 2, "EmissiveMat": 3, "IsotropicMat": 4, "GgxMat": 5}[type(m).__name__]
                      for m in scene.materials])
    ok = R.traced(rays)
    counts = {f"kind {k}": int(np.sum(hit & ok & (kinds[np.where(hit, material, 0)] == k))) for k in range(6)}
    tex = np.array([R.texture_kind_of(scene, m) or "" for m in range(len(scene.materials))])
    for t in R.TEXTURE_KINDS:
        counts[t] = int(np.sum(hit & ok & (tex[np.where(hit, material, 0)] == t)))
    counts["miss"] = int(np.sum(~hit & ok))
    d = rays[:, 3:]
    with np.errstate(all="ignore"):
        counts["flipped"] = int(np.sum(hit & ok & ((normal[:, 0] * d[:, 0] + normal[:, 1] * d[:, 1]) + normal[:, 2] * d[:, 2] > 0)))
        counts["unnormalised"] = int(np.sum(hit & ok & (np.abs(R.length32(normal) - 1.0) > 0.01)))
    counts["not traced"] = int(np.sum(~ok))
    return counts


@pytest.mark.parametrize("env, perlin", [("color", True), ("sky", True), ("color", False)])
def test_surface_records_against_the_oracle(oracle, env, perlin):
    torch, dev = _torch()
    scene, targets = R.surface_scene(R.environments()[env], perlin)
    twin, _ = R.surface_scene(R.environments()[env], perlin, ggx=False)                       # the oracle's: a MetalMat where the GgxMat is
    rays = R.surface_rays(targets)
    assert 200 <= rays.shape[0] <= 600
    # the rays are chosen on the CPU: the oracle's trace says that every case occurs, before the device is asked
    ora = oracle.trace(twin, rays, use_bvh=True)
    need = _at_least_five(scene, rays, np.nan_to_num(ora[:, 8]).astype(np.int64), ora[:, 0] == 1, ora[:, 5:8])
    skip = () if perlin else ("perlin", "turbulence", "marble")
    assert all(v >= 5 for k, v in need.items() if k not in skip), need
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        for bvh in (True, False):
            hits = ds.trace(rays, bvh)
            got = _at_least_five(scene, rays, hits["material"].astype(np.int64), hits["object"] != R.NO_HIT, hits["normal"])
            assert all(v >= 5 for k, v in got.items() if k not in skip), got
            surf = ds.hit_surface(rays, hits)
            assert surf.shape == (rays.shape[0], 16) and surf.dtype == np.float32
            want = R.surface_reference(oracle, scene, twin, rays, hits)
            for name, cols in list(_lib.SURFACE_COLUMNS.items()) + [("pad", [11, 15])]:
                ok = R.same_bits(surf[:, cols], want[:, cols])
                ok = ok.all(axis=1) if ok.ndim == 2 else ok
                assert ok.all(), (env, perlin, bvh, name, int((~ok).sum()), np.nonzero(~ok)[0][:5], surf[~ok][:2], want[~ok][:2])
            # emission and the environment are not clamped
            assert surf[surf[:, 3] == 3.0][:, 12:15].max() == 15.0 and surf[surf[:, 3] == -1.0][:, 12:15].max() > 1.0
            # device arrays, on a side stream, into the caller's tensor: the same bits
            d_rays, d_hits = torch.from_numpy(rays).to(dev), _hits_tensor(hits, dev)
            out = torch.full((rays.shape[0], 16), NAN, dtype=torch.float32, device=dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                assert ds.hit_surface(d_rays, d_hits, out=out) is out
            side.synchronize()
            assert np.array_equal(u32(out.cpu().numpy()), u32(surf)), (env, perlin, bvh)
            assert np.array_equal(u32(ds.hit_surface(d_rays, ds.trace(d_rays, bvh)).cpu().numpy()), u32(surf))
        # records that name nothing in the scene are refused per record, whatever else they hold
        bad = hits.copy()
        hit = np.nonzero(hits["object"] != R.NO_HIT)[0]
        bad["material"][hit[0]], bad["object"][hit[1]], bad["material"][hit[2]] = len(scene.materials), len(scene.render_objects), 0xFFFFFFFF
        bad["object"][hit[3]] = 0xFFFFFFFE
        odd = ds.hit_surface(rays, bad)
        assert np.all(odd[hit[:4], 3] == -2.0) and np.all(np.delete(odd[hit[:4]], 3, axis=1) == 0.0)
        rest = np.setdiff1d(np.arange(rays.shape[0]), hit[:4])
        assert np.array_equal(u32(odd[rest]), u32(surf[rest]))
        assert ds.hit_surface(rays[:0], hits[:0]).shape == (0, 16)
    finally:
        ds.close()


# ---- fw_gather_reduce ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIRECTIONS)
def test_reduce_equals_the_float64_statement(D):
    torch, dev = _torch()
    rng = np.random.default_rng(D)
    n = 20
    s, E, Ed = R.synthetic_records(n, D, rng, unusable=3)
    assert set(np.unique(s[:, 3])) == {-2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0} or D < 63
    assert np.any(E < 0)
    side = torch.cuda.Stream(device=dev)
    for direct in (None, Ed):
        acc = api.gather_reduce(s, E, D, direct)
        assert np.all(acc[n - 3:] == 0.0)
        M = n + 3
        id_lists = {"none": None, "ascending": np.arange(M, dtype=np.uint32)[np.sort(rng.permutation(M)[:n])], "permuted": rng.permutation(M).astype(np.uint32)[:n]}
        for kind, ids in id_lists.items():
            what = f"D {D} direct {direct is not None} ids {kind}"
            at = np.arange(n) if ids is None else ids.astype(np.int64)
            prior = np.full((M, 4), NAN, np.float32)                                      # pre-filled sums are added to, the others stay
            prior[at] = rng.uniform(-2.0, 2.0, size=(n, 4)).astype(np.float32)
            host = prior.copy()
            assert _lib.gather_reduce(s, E, D, host, direct, ids) is host
            rest = np.setdiff1d(np.arange(M), at)
            assert np.array_equal(u32(host[rest]), u32(prior[rest])), what
            assert np.array_equal(u32(host[at]), u32(R.add_to(prior[at], acc))), what
            d_ids = None if ids is None else torch.from_numpy(ids.astype(np.int32)).to(dev)
            d_s, d_E = torch.from_numpy(s).to(dev), torch.from_numpy(E).to(dev)
            d_Ed = None if direct is None else torch.from_numpy(direct).to(dev)
            for _ in range(2):                                                             # two runs are bit-equal
                d_sums = torch.from_numpy(prior).to(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    assert _lib.gather_reduce(d_s, d_E, D, d_sums, d_Ed, d_ids) is d_sums
                side.synchronize()
                assert np.array_equal(u32(d_sums.cpu().numpy()), u32(host)), what
        zero = _lib.gather_reduce(s, E, D, np.zeros((n, 4), np.float32), direct)
        assert np.array_equal(u32(zero), u32(acc.astype(np.float32))), D
    # a point's sums are its own rays'
    for p in (0, n - 4):
        one = _lib.gather_reduce(s[p * D:(p + 1) * D], E[p * D:(p + 1) * D], D, np.zeros((1, 4), np.float32), Ed[p * D:(p + 1) * D])
        assert np.array_equal(u32(one[0]), u32(zero[p])), (D, p)


# ---- fw_bake_gather -----------------------------------------------------------------------------------------------------------------
def _renderer(use_bvh, seed=11):
    cam = api.CameraSettings.default().cam_pos((0.0, 3.0, 14.0)).look_at((0.0, 0.0, 0.0)).field_of_view(60.0)
    return api.Renderer.default().width(24).height(16).samples(2).use_bvh(use_bvh).seed(seed).camera(cam)


def _points(n, rng):
    """receivers around the surface scene: on the floor, between the spheres, three unusable"""
    pos = np.stack([rng.uniform(-14, 14, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-3, 5, n)], axis=1).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm[:, 1] = np.abs(nrm[:, 1]) + 0.5
    pos[1, 0], nrm[4], nrm[7, 2] = NAN, 0.0, INF
    return pos, nrm


def _lookup(grid, sh, form, surf):
    """the public probe lookup of `form` at surface records read in place"""
    p, nr = surf[:, 8:11], surf[:, 4:7]
    if form["placement"] is not None:
        return _lib.probe_irradiance_placed(grid, sh, form["placement"], p, nr, form["depth"], form["moments"], form["normal_bias"])
    if form["depth"] is not None:
        return _lib.probe_irradiance_vis(grid, sh, form["depth"], form["moments"], p, nr, form["normal_bias"])
    return _lib.probe_irradiance(grid, sh, p, nr)


def _chained(ds, g, grid, sh, form, pos, nrm, ids, use_bvh, seed, rounds, first_round=0, sums=None):
    """fw_ao_rays, fw_trace_rays, fw_hit_surface, the lookup, (fw_bake_direct,) fw_gather_reduce by hand, on the device over all points"""
    torch, dev = _torch()
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pos, d_nrm, d_sh = to(pos), to(nrm), to(sh)
    d_ids = None if ids is None else to(ids.astype(np.int32))
    d_form = dict(form, moments=to(form["moments"]), placement=to(form["placement"]))
    if sums is None:
        sums = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=dev)
    seen = set()
    for rd in range(first_round, first_round + rounds):
        rays = _lib.ao_rays(g.ao(), d_pos, d_nrm, d_ids, rd)
        hits = ds.trace(rays, use_bvh, seed=seed + rd)
        surf = ds.hit_surface(rays, hits)
        seen |= set(np.unique(surf[:, 3].cpu().numpy()).tolist())
        irr = _lookup(grid, d_sh, d_form, surf)
        direct = None
        if g.direct:
            direct, _s, _st = ds.bake_direct(DirectLight(g.direct_bias, "cosine", False), surf[:, 8:11], surf[:, 4:7], rounds=1, seed=seed + rd, use_bvh=use_bvh)
            assert float(direct[:, 0:3].max()) > 0.0
        _lib.gather_reduce(surf, irr, g.directions, sums, direct, d_ids)
    assert {-2.0, -1.0, 0.0, 3.0, 4.0} <= seen, seen
    return sums.cpu().numpy()


def _forms(grid, rng):
    depth = ProbeDepth(8, 2, 12.0)
    mean = rng.uniform(1.0, 8.0, size=(grid.n_probes, 8, 8)).astype(np.float32)
    moments = np.stack([mean, mean * mean + rng.uniform(0.0, 2.0, size=mean.shape).astype(np.float32)], axis=-1).astype(np.float32)
    placement = np.concatenate([rng.uniform(-0.4, 0.4, size=(grid.n_probes, 3)), (rng.uniform(size=(grid.n_probes, 1)) > 0.2)], axis=1).astype(np.float32)
    none = dict(depth=None, moments=None, normal_bias=0.0, placement=None)
    return dict(plain=none, vis=dict(none, depth=depth, moments=moments, normal_bias=0.05), placed=dict(none, placement=placement),
                placed_vis=dict(depth=depth, moments=moments, normal_bias=0.05, placement=placement))


@pytest.mark.parametrize("form_name, direct", [("plain", False), ("vis", False), ("placed", False), ("placed_vis", True), ("plain", True)])
def test_bake_equals_its_composition_and_is_progressive(form_name, direct):
    torch, dev = _torch()
    rng = np.random.default_rng(7)
    n, D, bvh = 23, 33, True
    scene, _ = R.surface_scene(R.environments()["sky"])
    if direct:
        for light in yaml_io.load_scene(os.path.join(ROOT, "scenes", "three_lights.yml")).lights:
            scene.add_light(light)
        assert len(scene.lights) == 3
    pos, nrm = _points(n, rng)
    ok = api.ao_usable(pos, nrm)
    assert ok.sum() == n - 3
    grid, sh = R.random_probes((3, 2, 2), rng)
    form = _forms(grid, rng)[form_name]
    g = FinalGather(D, 1e-3, direct, 2e-3).seed(3)
    args = dict(depth=form["depth"], moments=form["moments"], normal_bias=form["normal_bias"], placement=form["placement"], seed=11, use_bvh=bvh)
    r = _renderer(bvh)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        before = ds.render(r)
        ref = _chained(ds, g, grid, sh, form, pos, nrm, None, bvh, 11, 5)
        assert np.all(ref[~ok] == 0.0) and np.all(ref[ok, 0:3] >= 0.0) and np.any(ref[ok, 0:3] > 0.0) and np.any(ref[ok, 3] > 0.0)
        for chunk in (0, 1, 7, n):
            out, sums, st = ds.bake_gather(g, grid, sh, pos, nrm, None, rounds=5, chunk=chunk, **args)
            assert np.array_equal(u32(sums), u32(ref)), (form_name, chunk)
            assert np.array_equal(u32(out), u32(api.gather_resolve(ref, 5))), (form_name, chunk)
            assert st["rays"] >= int(ok.sum()) * D * 5 and st["ms_render"] > 0, st
            if not direct:
                assert st["rays"] == int(ok.sum()) * D * 5                                # n D rounds minus the zero rays
        assert np.all(out[~ok] == 0.0)
        # progressive: 2 + 3 rounds through sums equal 5 rounds in one call, on the host ...
        out2, sums, _ = ds.bake_gather(g, grid, sh, pos, nrm, None, rounds=2, chunk=7, **args)
        assert np.array_equal(u32(out2), u32(api.gather_resolve(sums, 2)))
        out5, sums5, _ = ds.bake_gather(g, grid, sh, pos, nrm, None, rounds=3, first_round=2, sums=sums, chunk=1, **args)
        assert sums5 is sums and np.array_equal(u32(sums5), u32(ref)) and np.array_equal(u32(out5), u32(api.gather_resolve(ref, 5)))
        # ... and with device tensors on a side stream, through an id list: entries outside the list are not touched
        to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ids = rng.permutation(n).astype(np.uint32)[:15]
        rest = np.setdiff1d(np.arange(n), ids)
        ref_ids = _chained(ds, g, grid, sh, form, pos, nrm, ids, bvh, 11, 5)
        assert np.all(ref_ids[rest] == 0.0)
        d_args = dict(args, moments=to(form["moments"]), placement=to(form["placement"]))
        s0, o0 = np.zeros((n, 4), np.float32), np.full((n, 4), 7.0, np.float32)
        s0[rest] = NAN
        d_s, d_o, d_ids = to(s0), to(o0), to(ids.astype(np.int32))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ds.bake_gather(g, grid, to(sh), to(pos), to(nrm), d_ids, rounds=2, sums=d_s, out=d_o, chunk=0, **d_args)
            o, s, _ = ds.bake_gather(g, grid, to(sh), to(pos), to(nrm), d_ids, rounds=3, first_round=2, sums=d_s, out=d_o, chunk=4, **d_args)
        side.synchronize()
        assert s is d_s and o is d_o
        o, s = o.cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(u32(s[ids]), u32(ref_ids[ids])) and np.all(np.isnan(s[rest]))
        assert np.array_equal(u32(o[ids]), u32(api.gather_resolve(ref_ids[ids], 5))) and np.all(o[rest] == 7.0)
        # timing changes no bit
        _o, sums_t, st = ds.bake_gather(g, grid, sh, pos, nrm, None, rounds=5, chunk=7, flags=A.FW_FLAG_TIME_KERNELS, **args)
        assert np.array_equal(u32(sums_t), u32(ref)) and st["ms_raygen"] > 0 and st["ms_accumulate"] > 0
        # fw_render is left as it was
        after = ds.render(r)
        assert np.array_equal(after.rgb8, before.rgb8) and np.array_equal(u32(after.linear), u32(before.linear))
        assert after.stats["rays"] == before.stats["rays"]
    finally:
        ds.close()


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def _box(material_of):
    scene = Scene.new()
    m = scene.add_material(material_of)
    for rect, k in ((XYRect, -1.0), (XYRect, 1.0), (XZRect, -1.0), (XZRect, 1.0), (YZRect, -1.0), (YZRect, 1.0)):
        scene.add_object(RenderObject.new(rect.new(-1.0, 1.0, -1.0, 1.0, k, m)))
    scene.set_environment(ColorEnv((0.3, 0.3, 0.3)))
    return scene


def _close(got, want, rel=4.0 * 2.0 ** -23):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print("got", got, "want", want, "relative error", np.abs(got - want) / np.abs(want))
    return np.all(np.abs(got - want) <= rel * np.abs(want))


def _bake(scene, g, grid, sh, pos, nrm, rounds=2, bvh=True):
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        out, _s, _ = ds.bake_gather(g, grid, sh, np.asarray(pos, np.float32), np.asarray(nrm, np.float32), None, rounds=rounds, use_bvh=bvh)
        return out
    finally:
        ds.close()


def test_known_answers_in_closed_and_open_scenes():
    """every ray carries the same radiance, so the tolerance is rounding alone: 4 x 2^-23 relative"""
    sh0 = np.array([1.5, 0.75, 2.25], np.float32)
    grid, sh = R.one_probe(sh0)
    pos, nrm = [[0.1, -0.2, 0.3], [0.0, 0.0, 0.0]], [[0.3, 1.0, -0.2], [0.0, 0.0, -1.0]]
    E0 = api.probe_lookup(grid, sh, pos, nrm)
    assert np.array_equal(E0[0], E0[1]) and np.all(E0 > 0)                                    # band 0 alone: the same for every normal
    for D in (65, 64):
        g = FinalGather(D, 0.0).seed(1)
        # (a) inside a closed Lambertian box of albedo a: a E0, no sky
        a = np.array([0.5, 0.25, 0.8], np.float32)
        out = _bake(_box(LambertianMat.with_color(a)), g, grid, sh, pos, nrm)
        assert _close(out[:, 0:3], a.astype(np.float64) * E0) and np.all(out[:, 3] == 0.0)
        # (c) a closed box of EmissiveMat 15: 15 pi — 1 pi if emission were clamped
        out = _bake(_box(EmissiveMat.with_color((15.0, 15.0, 15.0))), g, grid, sh, pos, nrm)
        assert _close(out[:, 0:3], np.full((2, 3), 15.0 * np.pi)) and np.all(out[:, 3] == 0.0)
        # (b) a bare floor under ColorEnv c: pi c, all sky
        c = np.array([0.25, 0.5, 3.0], np.float32)
        scene = Scene.new()
        scene.add_object(RenderObject.new(XZRect.new(-50.0, 50.0, -50.0, 50.0, 0.0, scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5))))))
        scene.set_environment(ColorEnv(c))
        out = _bake(scene, FinalGather(D, 1e-3).seed(1), grid, sh, [[0.5, 0.0, -0.25]], [[0.0, 1.0, 0.0]])
        assert _close(out[:, 0:3], np.pi * c.astype(np.float64)[None]) and np.all(out[:, 3] == 1.0)


def test_the_lookup_takes_the_side_the_ray_arrived_from():
    """(d) a receiver under a ceiling whose stored normal points away from it, probes with a band-1 term: the gathered light is the
    ceiling's albedo x E at the normal that faces the receiver, which differs from E at the stored one"""
    grid, sh = R.one_probe((1.5, 0.75, 2.25), band1=((0.2, 0.1, 0.3), (0.6, 0.3, 0.9), (0.1, 0.2, 0.1)))
    a = np.array([0.5, 0.25, 0.8], np.float32)
    scene = Scene.new()
    scene.add_object(RenderObject.new(XZRect.new(-1e4, 1e4, -1e4, 1e4, 1.0, scene.add_material(LambertianMat.with_color(a)))))
    pos, nrm = np.array([[0.0, 0.0, 0.0]], np.float32), np.array([[0.0, 1.0, 0.0]], np.float32)
    g = FinalGather(64, 0.0).jitter(False)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = _lib.ao_rays(g.ao(), pos, nrm)
        hits = ds.trace(rays, True)
        assert np.all(hits["object"] != R.NO_HIT)
        stored = hits["normal"]
        assert np.all((stored * rays[:, 3:]).sum(axis=1) > 0)                                 # the stored normal points away from every ray
        surf = ds.hit_surface(rays, hits)
        assert np.array_equal(u32(surf[:, 4:7]), u32(-stored))
        out, _s, _ = ds.bake_gather(g, grid, sh, pos, nrm, None, rounds=1)
    finally:
        ds.close()
    facing, away = api.probe_lookup(grid, sh, pos, -stored[:1])[0], api.probe_lookup(grid, sh, pos, stored[:1])[0]
    assert np.all(np.abs(facing - away) > 0.1 * np.abs(facing))
    assert _close(out[0, 0:3], a.astype(np.float64) * facing) and out[0, 3] == 0.0


@pytest.mark.parametrize("D", [64, 200])
def test_a_black_occluder_gives_ambient_occlusion(D):
    """(e) a floor point under a black sphere and ColorEnv c: out / (pi c) and sky are fw_bake_ao's ao at the same D, seed, jitter, bias,
    infinite radius and hard falloff, to 2^-22 absolute.  One round into zeroed sums: the gather rounds a number in [0, 1] once (adding
    to 0 and dividing by 1 are exact), fw_bake_ao rounds O and then 1 - O: three roundings of at most 2^-24 each"""
    c = np.array([0.25, 0.5, 3.0], np.float32)
    scene = Scene.new()
    grey, black = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5))), scene.add_material(LambertianMat.with_color((0.0, 0.0, 0.0)))
    scene.add_object(RenderObject.new(XZRect.new(-50.0, 50.0, -50.0, 50.0, 0.0, grey)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, black)).position(0.25, 1.6, -0.5))
    scene.set_environment(ColorEnv(c))
    grid, sh = R.one_probe((1.5, 0.75, 2.25))
    pos, nrm = np.array([[0.25, 0.0, -0.5], [3.0, 0.0, 1.0]], np.float32), np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        for jitter in (False, True):
            g = FinalGather(D, 1e-3).seed(5).jitter(jitter)
            out, _s, _ = ds.bake_gather(g, grid, sh, pos, nrm, None, rounds=1, seed=2)
            ao, _s, _ = ds.bake_ao(AmbientOcclusion(INF, D, 0, 1e-3).seed(5).jitter(jitter), pos, nrm, None, 1, seed=2)
            ratio = out[:, 0:3].astype(np.float64) / (np.pi * c.astype(np.float64))
            print("D", D, "jitter", jitter, "ao", ao[:, 3], "sky", out[:, 3], "ratio", ratio)
            assert 0.2 < ao[0, 3] < 0.9 and ao[1, 3] > ao[0, 3]
            assert np.all(np.abs(out[:, 3].astype(np.float64) - ao[:, 3]) <= 2.0 ** -22)
            assert np.all(np.abs(ratio - ao[:, 3:4]) <= 2.0 ** -22)
    finally:
        ds.close()


# ---- the Python layer and the CLI -----------------------------------------------------------------------------------------------------
def test_render_probe_lit_with_a_gather_is_its_composition():
    torch, dev = _torch()
    from firework_amd import scenes
    from firework_amd.api import ProbeGrid, ProbeSet
    scene, r = scenes.config("C2_cornell_box", 32, 24, 4)
    for light in yaml_io.load_scene(os.path.join(ROOT, "scenes", "three_lights.yml")).lights:
        scene.add_light(light)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    pd = ProbeDepth(8, 6, 800.0)
    g = FinalGather(33, 0.5).seed(6)
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sh, _sums = r.bake_probes(ds, probes, 1)
        moments, _dsums = r.bake_probe_depth(ds, probes, pd, 1)
        aov = ds.aovs(r, 4, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        d_sh, d_mom = torch.from_numpy(sh).to(dev), torch.from_numpy(moments).to(dev)
        grid = ProbeGrid.of(probes, True)
        inv_pi, one = np.float32(1.0 / np.pi), np.float32(1.0)
        v = rec[:, 3:4]
        for depth, direct in ((None, None), (pd, None), (None, DirectLight(0.25))):
            kw = {} if depth is None else dict(depth=pd, moments=moments, normal_bias=2.0)
            res = r.render_probe_lit(ds, probes, sh, aov_samples=4, gather=g, gather_rounds=2, direct=direct, **kw)
            gg = FinalGather(33, 0.5, direct is not None, 0.25 if direct is not None else g.direct_bias).seed(6)
            Eg, _s, _ = ds.bake_gather(gg, grid, d_sh, aov[:, 8:11], aov[:, 4:7], None, depth, None if depth is None else d_mom,
                                       2.0 if depth is not None else 0.0, None, 2, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
            E = Eg.cpu().numpy()
            assert np.any(E[:, 0:3] > 0) and np.all(E[rec[:, 3] == 0.0] == 0.0)
            want = (rec[:, 0:3] * (v * (E[:, 0:3] * inv_pi) + (one - v))).astype(np.float32)
            if direct is not None:
                want = (want + r._direct_term(ds, direct, aov, None)[0].cpu().numpy()).astype(np.float32)
            assert np.array_equal(u32(res.linear), u32(want)), (depth, direct)
            ref8, refg, _ = _lib.denoise(want, rec, None, 32, 24, 0, s["gamma"])
            assert np.array_equal(res.rgb8, ref8) and np.array_equal(u32(res.gamma), u32(refg)), (depth, direct)
            # gather=None: the calls and the bits of the call without the argument
            plain, none = r.render_probe_lit(ds, probes, sh, aov_samples=4, direct=direct, **kw), r.render_probe_lit(ds, probes, sh, aov_samples=4, direct=direct, gather=None, **kw)
            assert np.array_equal(u32(plain.linear), u32(none.linear)) and np.array_equal(plain.rgb8, none.rgb8)
            assert not np.array_equal(u32(plain.linear), u32(res.linear))
        # render_gather: the records and the bake chained
        E, sky, sums = r.render_gather(ds, g, probes, sh, rounds=2, samples=4)
        Eg, sg, _ = ds.bake_gather(g, grid, d_sh, aov[:, 8:11], aov[:, 4:7], None, rounds=2, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        assert E.shape == (24, 32, 3) and sky.shape == (24, 32) and sums.shape == (24, 32, 4)
        assert np.array_equal(u32(E.reshape(-1, 3)), u32(Eg.cpu().numpy()[:, 0:3])) and np.array_equal(u32(sky.reshape(-1)), u32(Eg.cpu().numpy()[:, 3]))
        assert np.array_equal(u32(sums.reshape(-1, 4)), u32(sg.cpu().numpy()))
        for bad in (dict(ao=AmbientOcclusion(10.0)), dict(radiance=api.ProbeRadiance(4, 2, [0.5]), maps=np.zeros((8, 16, 4), np.float32))):
            with pytest.raises(ValueError, match="gather"):
                r.render_probe_lit(ds, probes, sh, gather=g, **bad)
    finally:
        ds.close()


def test_cli_round_trip(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    yml = os.path.join(ROOT, "scenes", "three_lights.yml")
    base = ["--scene-file", yml, "-s", "2", "--seed", "3"]
    npz, png, plain = str(tmp_path / "p.npz"), str(tmp_path / "g.png"), str(tmp_path / "plain.png")
    assert main(base + ["--bake-probes", "2,2,3", "--probe-min=-12,0.05,-12", "--probe-max", "12,9,12", "--probe-dirs", "32", "--probe-depth", "8", "-o", npz]) == 0
    lit = ["--width", "16", "--height", "16", "--aov-samples", "2", "--probe-lit", npz]
    assert main(base + lit + ["--probe-gather", "33,2", "--gather-bias", "0.01", "--direct-light", "-o", png]) == 0
    assert main(base + lit + ["--direct-light", "-o", plain]) == 0
    scene = yaml_io.load_scene(yml)
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(16).height(16).samples(2).use_bvh(True).camera(cam).seed(3)
    with np.load(npz) as z:
        grid = api.ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"])
        want = r.render_probe_lit(scene, grid, z["sh"], 2, depth=ProbeDepth(int(z["depth_res"]), int(z["depth_sharpness"]), float(z["depth_max"])),
                                  moments=z["depth"], direct=DirectLight(1e-3), gather=FinalGather(33, 0.01).seed(3), gather_rounds=2).rgb8
    img = np.asarray(Image.open(png).convert("RGB"))
    assert img.shape == (16, 16, 3) and np.array_equal(img.reshape(-1, 3), want.reshape(-1, 3))
    assert not np.array_equal(img, np.asarray(Image.open(plain).convert("RGB")))
