"""The reflection gather on the GPU (fw_reflect_rays, fw_reflect_reduce, fw_bake_reflect).

k_reflect_rays against api.reflect_rays: the same rays dead and alive, origins and directions within one float32 ulp at each vector's
scale (§9k's bound, the one tests/test_gpu_ao.py uses), the weights within one float32 ulp; k_reflect_reduce against api.reflect_reduce
bit for bit (the statement has only +, x, comparisons and one rounding: every operation is IEEE-determined); the bake against the
public calls chained by hand, bit for bit, for every chunking and every form of the probe lookup, progressively, with the delta lights,
with fw_render left as it was; the albedo under a constant environment against fw_ggx_terms; the parallax test that the radiance maps
cannot pass; render_probe_lit(reflect=) against its composition; the CLI's round trip."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, yaml_io
from firework_amd.api import (ColorEnv, DirectLight, EmissiveMat, FinalGather, GgxMat, LambertianMat, PointLight, ProbeDepth, ProbeRadiance,
                              ProbeSet, ReflectionGather, RenderObject, Scene, Sphere, XYRect, XZRect, YZRect)

import reflect_ref as R
from test_reflect_cpu import ESTIMATOR_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DIRECTIONS = [1, 3, 63, 64, 65, 200]            # the gather tests': one ray, below a wave, a wave's tail, a wave, a wave plus one, a tail
u32 = R.u32


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _columns(a, dev):
    """the device twin of a host (n, 3) array that is contiguous or a column range of a contiguous record array: the same layout"""
    import torch
    base = a if a.base is None else a.base
    t = torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    if base is a:
        return t
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 4
    return t[:, off:off + 3]


def assert_vectors_close(got, ref, what):
    """per component |gpu - ref| <= 2^-23 x the largest magnitude among that 3-vector's reference components; every entry finite"""
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.all(np.isfinite(got)), what
    g, r = got.astype(np.float64).reshape(-1, 3), ref.astype(np.float64).reshape(-1, 3)
    bound = 2.0 ** -23 * np.abs(r).max(axis=1, keepdims=True)
    err = np.abs(g - r)
    assert np.all(err <= bound), (what, float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[:4])


# ---- fw_reflect_rays ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, stride, with_ids, rnd, jitter", R.ray_cases())
def test_rays_and_weights_match_the_numpy_statement(D, stride, with_ids, rnd, jitter):
    """37 points, the records read in place at strides 3, 12 and 16, with and without ids, rounds 0 and 1, rho from 0.03 to 1, views from
    head-on to grazing.  test_reflect_cpu asserts that no ray of these cases lies within 1e-9 of the horizon, so dead and alive must agree
    for every ray: none is left out of the comparison."""
    torch, dev = _torch()
    reflect, pos, nrm, view, spec, ids = R.case_inputs(D, stride, with_ids, jitter)
    what = f"D {D} stride {stride} ids {with_ids} round {rnd} jitter {jitter}"
    ref, ref_w, t = api.reflect_rays(reflect, pos, nrm, view, spec, ids, rnd, terms=True)
    host, host_w = _lib.reflect_rays(reflect, pos, nrm, view, spec, ids, rnd)
    m = 37 if ids is None else ids.size
    assert host.shape == (m * D, 6) and host_w.shape == (m * D, 2) and host.dtype == host_w.dtype == np.float32, what
    alive = ref_w[:, 0] > 0
    assert np.array_equal(host_w[:, 0] > 0, alive) and 0 < alive.sum() < alive.size, what                  # dead and alive agree for every ray
    assert not host[~alive].any() and not host_w[~alive].any(), what
    assert np.all(np.any(host[alive, 3:6] != 0, axis=1)), what
    unusable = ~np.repeat(t["usable"], D)
    assert unusable.sum() >= 3 * D and not host[unusable].any() and not host_w[unusable].any(), what
    assert_vectors_close(host[:, 0:3], ref[:, 0:3], what + " origins")
    assert_vectors_close(host[:, 3:6], ref[:, 3:6], what + " directions")
    for k, name in ((0, "g"), (1, "s")):
        err, ulp = np.abs(host_w[:, k].astype(np.float64) - ref_w[:, k]), R.ulp32(ref_w[:, k])
        assert np.all(err <= ulp), (what, name, float((err / ulp).max()))
    # device tensors, read in place with the same strides: the host call's bits
    d_ids = None if ids is None else torch.from_numpy(ids.astype(np.int32)).to(dev)
    out, w = torch.full((m * D, 6), NAN, dtype=torch.float32, device=dev), torch.full((m * D, 2), NAN, dtype=torch.float32, device=dev)
    got = _lib.reflect_rays(reflect, _columns(pos, dev), _columns(nrm, dev), _columns(view, dev), torch.from_numpy(spec).to(dev), d_ids, rnd, out=out, weights=w)
    assert got[0] is out and got[1] is w
    assert np.array_equal(u32(out.cpu().numpy()), u32(host)) and np.array_equal(u32(w.cpu().numpy()), u32(host_w)), what
    # another round or another seed: other rays
    if jitter:
        assert not np.array_equal(_lib.reflect_rays(reflect, pos, nrm, view, spec, ids, rnd + 1)[0], host), what
        other = ReflectionGather(D).bias(0.01).seed(R.SEED + 1)
        assert not np.array_equal(_lib.reflect_rays(other, pos, nrm, view, spec, ids, rnd)[0], host), what


# ---- fw_reflect_reduce --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIRECTIONS)
def test_reduce_equals_the_float64_statement(D):
    torch, dev = _torch()
    rng = np.random.default_rng(D)
    n = 20
    s, E, Ed = R.synthetic_records(n, D, rng, unusable=3)
    w, s = R.synthetic_weights(n, D, rng, s)
    w.reshape(n, D, 2)[n - 3:] = 0.0
    assert set(np.unique(s[:, 3])) == {-2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0} or D < 63
    assert np.any(E < 0) and np.any(w[:, 0] == 0)
    side = torch.cuda.Stream(device=dev)
    for direct in (None, Ed):
        acc = api.reflect_reduce(s, E, w, D, direct)
        assert np.all(acc[n - 3:] == 0.0)
        M = n + 3
        id_lists = {"none": None, "ascending": np.arange(M, dtype=np.uint32)[np.sort(rng.permutation(M)[:n])], "permuted": rng.permutation(M).astype(np.uint32)[:n]}
        for kind, ids in id_lists.items():
            what = f"D {D} direct {direct is not None} ids {kind}"
            at = np.arange(n) if ids is None else ids.astype(np.int64)
            prior = np.full((M, 8), NAN, np.float32)                                      # pre-filled sums are added to, the others stay
            prior[at] = rng.uniform(-2.0, 2.0, size=(n, 8)).astype(np.float32)
            host = prior.copy()
            assert _lib.reflect_reduce(s, E, w, D, host, direct, ids) is host
            rest = np.setdiff1d(np.arange(M), at)
            assert np.array_equal(u32(host[rest]), u32(prior[rest])), what
            assert np.array_equal(u32(host[at]), u32(R.add_to(prior[at], acc))), what
            d_ids = None if ids is None else torch.from_numpy(ids.astype(np.int32)).to(dev)
            d_s, d_E, d_w = torch.from_numpy(s).to(dev), torch.from_numpy(E).to(dev), torch.from_numpy(w).to(dev)
            d_Ed = None if direct is None else torch.from_numpy(direct).to(dev)
            for _ in range(2):                                                             # two runs are bit-equal
                d_sums = torch.from_numpy(prior).to(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    assert _lib.reflect_reduce(d_s, d_E, d_w, D, d_sums, d_Ed, d_ids) is d_sums
                side.synchronize()
                assert np.array_equal(u32(d_sums.cpu().numpy()), u32(host)), what
        zero = _lib.reflect_reduce(s, E, w, D, np.zeros((n, 8), np.float32), direct)
        assert np.array_equal(u32(zero), u32(acc.astype(np.float32))), D
    # a point's sums are its own rays'
    for p in (0, n - 4):
        sl = slice(p * D, (p + 1) * D)
        one = _lib.reflect_reduce(s[sl], E[sl], w[sl], D, np.zeros((1, 8), np.float32), Ed[sl])
        assert np.array_equal(u32(one[0]), u32(zero[p])), (D, p)


# ---- fw_bake_reflect ----------------------------------------------------------------------------------------------------------------
def _room(light=False):
    """a closed room, x and z in [-4, 4], y in [0, 5], with a glossy floor, coloured Lambertian walls, an emissive panel in the ceiling
    and a Lambertian sphere standing on the floor; light: a point light under the ceiling"""
    scene = Scene.new()
    floor = scene.add_material(GgxMat.new((0.9, 0.7, 0.5), 0.2))
    red, green, white = (scene.add_material(LambertianMat.with_color(c)) for c in ((0.7, 0.2, 0.2), (0.2, 0.7, 0.2), (0.7, 0.7, 0.7)))
    lamp = scene.add_material(EmissiveMat.with_color((6.0, 5.0, 4.0)))
    scene.add_object(RenderObject.new(XZRect.new(-4.0, 4.0, -4.0, 4.0, 0.0, floor)))
    scene.add_object(RenderObject.new(XZRect.new(-4.0, 4.0, -4.0, 4.0, 5.0, white)))
    scene.add_object(RenderObject.new(XZRect.new(-1.5, 1.5, -1.5, 1.5, 4.99, lamp)))
    scene.add_object(RenderObject.new(YZRect.new(0.0, 5.0, -4.0, 4.0, -4.0, red)))
    scene.add_object(RenderObject.new(YZRect.new(0.0, 5.0, -4.0, 4.0, 4.0, green)))
    scene.add_object(RenderObject.new(XYRect.new(-4.0, 4.0, 0.0, 5.0, -4.0, white)))
    scene.add_object(RenderObject.new(XYRect.new(-4.0, 4.0, 0.0, 5.0, 4.0, white)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, white)).position(1.5, 1.0, -1.0))
    scene.set_environment(ColorEnv((0.1, 0.2, 0.4)))
    if light:
        scene.add_light(PointLight((-1.0, 4.0, 1.0), (20.0, 20.0, 20.0)))
    return scene, (0.9, 0.7, 0.5, 0.2)


def _floor_points(n, rng, spec_row):
    """n receivers on the room's floor seen from an eye at (0, 3, 3.5); three unusable: a NaN position, a zero view, rho = 0"""
    pos = np.stack([rng.uniform(-3.5, 3.5, n), np.zeros(n), rng.uniform(-3.5, 3.5, n)], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (n, 1)) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    view = (pos - np.array([0.0, 3.0, 3.5], np.float32)).astype(np.float32)
    spec = np.tile(np.array([spec_row], np.float32), (n, 1))
    spec[:, 3] = rng.uniform(0.05, 0.6, n)
    pos[1, 0], view[4], spec[7, 3] = NAN, 0.0, 0.0
    return pos, nrm, view, spec


def _renderer(use_bvh, seed=11):
    cam = api.CameraSettings.default().cam_pos((0.0, 3.0, 3.5)).look_at((0.0, 0.5, 0.0)).field_of_view(70.0)
    return api.Renderer.default().width(24).height(16).samples(2).use_bvh(use_bvh).seed(seed).camera(cam)


def _lookup(grid, sh, form, surf):
    """the public probe lookup of `form` at surface records read in place"""
    p, nr = surf[:, 8:11], surf[:, 4:7]
    if form["placement"] is not None:
        return _lib.probe_irradiance_placed(grid, sh, form["placement"], p, nr, form["depth"], form["moments"], form["normal_bias"])
    if form["depth"] is not None:
        return _lib.probe_irradiance_vis(grid, sh, form["depth"], form["moments"], p, nr, form["normal_bias"])
    return _lib.probe_irradiance(grid, sh, p, nr)


def _chained(ds, g, grid, sh, form, pts, ids, use_bvh, seed, rounds, first_round=0, sums=None):
    """fw_reflect_rays, fw_trace_rays, fw_hit_surface, the lookup, (fw_bake_direct,) fw_reflect_reduce by hand, on the device over all points"""
    torch, dev = _torch()
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pos, d_nrm, d_view, d_spec = (to(a) for a in pts)
    d_sh = to(sh)
    d_ids = None if ids is None else to(ids.astype(np.int32))
    d_form = dict(form, moments=to(form["moments"]), placement=to(form["placement"]))
    if sums is None:
        sums = torch.zeros((pts[0].shape[0], 8), dtype=torch.float32, device=dev)
    seen = set()
    for rd in range(first_round, first_round + rounds):
        rays, w = _lib.reflect_rays(g, d_pos, d_nrm, d_view, d_spec, d_ids, rd)
        hits = ds.trace(rays, use_bvh, seed=seed + rd)
        surf = ds.hit_surface(rays, hits)
        seen |= set(np.unique(surf[:, 3].cpu().numpy()).tolist())
        irr = _lookup(grid, d_sh, d_form, surf)
        direct = None
        if g.direct:
            direct, _s, _st = ds.bake_direct(DirectLight(g._direct_bias, "cosine", False), surf[:, 8:11], surf[:, 4:7], rounds=1, seed=seed + rd, use_bvh=use_bvh)
            assert float(direct[:, 0:3].max()) > 0.0
        _lib.reflect_reduce(surf, irr, w, g.directions, sums, direct, d_ids)
    assert {-2.0, 0.0} <= seen, seen
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
    n, D, bvh = 24, 5, True
    scene, spec_row = _room(light=direct)
    pts = _floor_points(n, rng, spec_row)
    pos, nrm, view, spec = pts
    ok = api.reflect_usable(*pts)
    assert ok.sum() == n - 3
    grid, sh = R.random_probes((3, 2, 2), rng, lo=(-4.0, 0.0, -4.0), hi=(4.0, 5.0, 4.0))
    form = _forms(grid, rng)[form_name]
    g = ReflectionGather(D).bias(1e-3).seed(3)
    if direct:
        g.direct_bias(2e-3)
    args = dict(depth=form["depth"], moments=form["moments"], normal_bias=form["normal_bias"], placement=form["placement"], seed=11, use_bvh=bvh)
    r = _renderer(bvh)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        before = ds.render(r)
        ref = _chained(ds, g, grid, sh, form, pts, None, bvh, 11, 5)
        assert np.all(ref[~ok] == 0.0) and np.all(ref[ok][:, [0, 1, 2, 4, 5, 6]] >= 0.0) and np.any(ref[ok, 0:3] > 0.0) and np.all(ref[ok, 3] > 0.0)
        want_out = api.reflect_resolve(ref, spec, 5)
        assert np.all(want_out[~ok] == 0.0)
        for chunk in (0, 1, 7, n):
            out, sums, st = ds.bake_reflect(g, grid, sh, pos, nrm, view, spec, None, rounds=5, chunk=chunk, **args)
            assert sums.shape == (n, 8) and out.shape == (n, 4)
            assert np.array_equal(u32(sums), u32(ref)), (form_name, chunk)
            assert np.array_equal(u32(out), u32(want_out)), (form_name, chunk)
            assert st["rays"] >= round(float(ref[:, 3].sum()) * D) and st["ms_render"] > 0, st     # the alive rays (dead ones are not traced)
            if not direct:
                assert st["rays"] == round(float(ref[:, 3].astype(np.float64).sum()) * D), st
        # progressive: 2 + 3 rounds through sums equal 5 rounds in one call, on the host ...
        out2, sums, _ = ds.bake_reflect(g, grid, sh, pos, nrm, view, spec, None, rounds=2, chunk=7, **args)
        assert np.array_equal(u32(out2), u32(api.reflect_resolve(sums, spec, 2)))
        out5, sums5, _ = ds.bake_reflect(g, grid, sh, pos, nrm, view, spec, None, rounds=3, first_round=2, sums=sums, chunk=1, **args)
        assert sums5 is sums and np.array_equal(u32(sums5), u32(ref)) and np.array_equal(u32(out5), u32(want_out))
        # ... and with device tensors on a side stream, through an id list: entries outside the list are not touched
        to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ids = rng.permutation(n).astype(np.uint32)[:15]
        rest = np.setdiff1d(np.arange(n), ids)
        ref_ids = _chained(ds, g, grid, sh, form, pts, ids, bvh, 11, 5)
        assert np.all(ref_ids[rest] == 0.0)
        d_args = dict(args, moments=to(form["moments"]), placement=to(form["placement"]))
        s0, o0 = np.zeros((n, 8), np.float32), np.full((n, 4), 7.0, np.float32)
        s0[rest] = NAN
        d_s, d_o, d_ids = to(s0), to(o0), to(ids.astype(np.int32))
        d_pts = [to(a) for a in pts]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ds.bake_reflect(g, grid, to(sh), *d_pts, d_ids, rounds=2, sums=d_s, out=d_o, chunk=0, **d_args)
            o, s, _ = ds.bake_reflect(g, grid, to(sh), *d_pts, d_ids, rounds=3, first_round=2, sums=d_s, out=d_o, chunk=4, **d_args)
        side.synchronize()
        assert s is d_s and o is d_o
        o, s = o.cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(u32(s[ids]), u32(ref_ids[ids])) and np.all(np.isnan(s[rest]))
        assert np.array_equal(u32(o[ids]), u32(api.reflect_resolve(ref_ids[ids], spec[ids], 5))) and np.all(o[rest] == 7.0)
        # timing changes no bit
        _o, sums_t, st = ds.bake_reflect(g, grid, sh, pos, nrm, view, spec, None, rounds=5, chunk=7, flags=A.FW_FLAG_TIME_KERNELS, **args)
        assert np.array_equal(u32(sums_t), u32(ref)) and st["ms_raygen"] > 0 and st["ms_accumulate"] > 0
        # fw_render is left as it was
        after = ds.render(r)
        assert np.array_equal(after.rgb8, before.rgb8) and np.array_equal(u32(after.linear), u32(before.linear))
        assert after.stats["rays"] == before.stats["rays"]
    finally:
        ds.close()


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def _bake(scene, g, grid, sh, pos, nrm, view, spec, rounds, **kw):
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        out, sums, _ = ds.bake_reflect(g, grid, sh, *(np.asarray(a, np.float32) for a in (pos, nrm, view, spec)), None, rounds=rounds, **kw)
        return out, sums
    finally:
        ds.close()


@pytest.mark.parametrize("rho", [0.1, 0.3, 1.0])
def test_albedo_under_a_constant_environment(rho):
    """one GgxMat floor point under a ColorEnv of colour c and nothing else: every alive ray misses, so out / c estimates the
    directional albedo F0 A + B (fw_ggx_terms) within the bound measured on the CPU (test_reflect_cpu), and out is the numpy chain's"""
    c = np.array([0.25, 0.5, 3.0], np.float32)
    f0 = np.array([0.95, 0.64, 0.04], np.float32)
    D, rounds = 256, 4
    grid, sh = R.one_probe((0.0, 0.0, 0.0))
    for mu in (0.2, 0.7, 1.0):
        scene = Scene.new()
        scene.add_object(RenderObject.new(XZRect.new(-50.0, 50.0, -50.0, 50.0, 0.0, scene.add_material(GgxMat.new(tuple(f0), rho)))))
        scene.set_environment(ColorEnv(c))
        pos, nrm = [[0.5, 0.0, -0.25]], [[0.0, 1.0, 0.0]]
        view = [[np.sqrt(1.0 - mu * mu), -mu, 0.0]]
        spec = np.array([[f0[0], f0[1], f0[2], rho]], np.float32)
        g = ReflectionGather(D).bias(1e-3).seed(R.SEED)
        out, sums = _bake(scene, g, grid, sh, pos, nrm, view, spec, rounds)
        mu32 = np.float32(mu)
        AB = _lib.ggx_terms(api.GgxTable(), np.array([mu32], np.float32), np.array([rho], np.float32))[0].astype(np.float64)
        want = f0.astype(np.float64) * AB[0] + AB[1]
        got = out[0, 0:3].astype(np.float64) / c.astype(np.float64)
        print(f"mu {mu} rho {rho}: out / c {got}, F0 A + B {want}, error {np.abs(got - want)}, alive {out[0, 3]}, sky {sums[0, 7] / rounds}")
        assert np.all(np.abs(got - want) <= ESTIMATOR_BOUND), (mu, rho)
        assert sums[0, 7] == sums[0, 3] and 0.0 < out[0, 3] <= 1.0                                # every alive ray saw the environment
        # the numpy chain: the statement's rays and weights, every alive ray a miss that brings c
        total = np.zeros((1, 8), np.float32)
        for rd in range(rounds):
            _rays, w = api.reflect_rays(g, pos, nrm, view, spec, round=rd)
            surf = np.zeros((D, 16), np.float32)
            surf[:, 3], surf[:, 12:15] = np.where(w[:, 0] > 0, -1.0, -2.0), c
            total = R.add_to(total, api.reflect_reduce(surf, np.zeros((D, 3), np.float32), w, D))
        chain = api.reflect_resolve(total, spec, rounds)
        assert np.all(np.abs(out[0].astype(np.float64) - chain[0]) <= 1e-6 * np.abs(chain[0].astype(np.float64))), (mu, rho, out, chain)


def test_parallax_the_radiance_maps_cannot_show():
    """A nearly smooth floor (rho = 0.03) seen at 45 degrees: the mirrored ray meets, two units away, a large emissive rectangle — or,
    from a point further along, the black wall beside it.  Facing the rectangle the reflection is e (F0 A + B) and every ray alive;
    facing the wall, with black probes, it is exactly 0 — while the radiance maps baked in the same scene, read along the same mirrored
    direction from where the probes stand, are not 0 there: that is the parallax error the traced reflection does not have."""
    e = np.array([4.0, 3.0, 2.0], np.float32)
    f0, rho = np.array([0.9, 0.6, 0.3], np.float32), np.float32(0.03)
    k = float(np.sqrt(2.0))
    scene = Scene.new()
    floor = scene.add_material(GgxMat.new(tuple(f0), float(rho)))
    lamp, black = scene.add_material(EmissiveMat.with_color(tuple(e))), scene.add_material(LambertianMat.with_color((0.0, 0.0, 0.0)))
    scene.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 40.0, 0.0, floor)))
    scene.add_object(RenderObject.new(YZRect.new(0.0, 30.0, -20.0, 5.0, k, lamp)))             # the plane x = sqrt(2): the emitter for z < 5 ...
    scene.add_object(RenderObject.new(YZRect.new(0.0, 30.0, 5.0, 40.0, k, black)))            # ... and the black wall beside it
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 5.5]], np.float32)
    nrm = np.array([[0.0, 1.0, 0.0]] * 2, np.float32)
    view = np.array([[1.0, -1.0, 0.0]] * 2, np.float32)
    spec = np.array([[f0[0], f0[1], f0[2], rho]] * 2, np.float32)
    probes = ProbeSet.grid((-1.0, 0.5, 3.0), (0.5, 2.0, 8.0), (2, 2, 2), 256).seed(1)
    grid = api.ProbeGrid.of(probes, True)
    sh = np.zeros((grid.n_probes, 9, 3), np.float32)
    out, sums = _bake(scene, ReflectionGather(64).bias(1e-3).seed(R.SEED), grid, sh, pos, nrm, view, spec, 4)
    AB = _lib.ggx_terms(api.GgxTable(), np.array([np.sqrt(0.5)], np.float32), np.array([rho], np.float32))[0].astype(np.float64)
    want = e.astype(np.float64) * (f0.astype(np.float64) * AB[0] + AB[1])
    print("facing the rectangle", out[0], "want", want, "facing the wall", out[1])
    assert out[0, 3] == 1.0 and np.all(np.abs(out[0, 0:3] - want) <= ESTIMATOR_BOUND * e.astype(np.float64))
    assert out[1, 3] == 1.0 and np.all(out[1, 0:3] == 0.0) and not sums[1, [0, 1, 2, 4, 5, 6, 7]].any()
    # the radiance maps of probes standing around the second point, baked in the same scene, along the same mirrored direction
    pr = ProbeRadiance(8, 2, [0.03, 0.5])
    r = api.Renderer.default().samples(1).use_bvh(True).seed(2)
    maps, _sums = r.bake_probe_radiance(scene, probes, pr, 2)
    mirrored = np.array([[1.0, 1.0, 0.0]], np.float32)
    seen = _lib.probe_radiance_lookup(grid, pr, maps, pos[1:2], nrm[1:2], mirrored, np.array([rho], np.float32))
    print("the radiance maps along the mirrored direction at the second point", seen)
    assert np.all(seen[0] > 0.0)


# ---- the Python layer and the CLI -----------------------------------------------------------------------------------------------------
def test_render_probe_lit_with_reflect_is_its_composition():
    torch, dev = _torch()
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "ggx_lights.yml"))
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(16).height(16).samples(2).use_bvh(True).camera(cam).seed(3)
    probes = ProbeSet.grid((-30.0, 1.0, -30.0), (30.0, 25.0, 30.0), (2, 2, 2), 65)
    pd = ProbeDepth(8, 6, 200.0)
    g = ReflectionGather(8).bias(0.05).seed(6)
    fg = FinalGather(9, 0.05).seed(4)
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sh, _sums = r.bake_probes(ds, probes, 1)
        moments, _dsums = r.bake_probe_depth(ds, probes, pd, 1)
        placement = api.neutral_placement(probes.n_probes)
        aov = ds.aovs(r, 4, out=torch.empty((16 * 16, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        S, alive, sums = r.render_reflect(ds, g, probes, sh, rounds=2, samples=4)
        assert S.shape == (16, 16, 3) and alive.shape == (16, 16) and sums.shape == (16, 16, 8)
        rays, spec = r._view_spec(ds, None, 16, 16, dev)
        sp = spec.cpu().numpy()
        glossy = sp[:, 3] > 0
        assert 10 < glossy.sum() < 200 and np.all(alive.reshape(-1)[~glossy] == 0.0) and np.any(S.reshape(-1, 3)[glossy] > 0)
        assert np.all(S.reshape(-1, 3)[~glossy] == 0.0) and np.any(alive.reshape(-1)[glossy] > 0.0)
        out, sg, _ = ds.bake_reflect(g, api.ProbeGrid.of(probes, True), torch.from_numpy(sh).to(dev), aov[:, 8:11], aov[:, 4:7], rays[:, 3:6], spec, None,
                                     rounds=2, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        assert np.array_equal(u32(S.reshape(-1, 3)), u32(out.cpu().numpy()[:, 0:3])) and np.array_equal(u32(sums.reshape(-1, 8)), u32(sg.cpu().numpy()))
        assert np.array_equal(u32(out.cpu().numpy()), u32(api.reflect_resolve(sums.reshape(-1, 8), sp, 2)))
        v, one = rec[:, 3:4], np.float32(1.0)
        branches = (("plain", {}), ("depth", dict(depth=pd, moments=moments, normal_bias=0.5)), ("placement", dict(placement=placement)),
                    ("gather", dict(gather=fg, gather_rounds=2)))
        for name, kw in branches:
            base = r.render_probe_lit(ds, probes, sh, aov_samples=4, **kw)
            none = r.render_probe_lit(ds, probes, sh, aov_samples=4, reflect=None, **kw)
            assert np.array_equal(u32(base.linear), u32(none.linear)) and np.array_equal(base.rgb8, none.rgb8), name      # reflect=None: today's frame
            res = r.render_probe_lit(ds, probes, sh, aov_samples=4, reflect=g, reflect_rounds=2, **kw)
            lk = {k_: v_ for k_, v_ in kw.items() if k_ in ("depth", "moments", "normal_bias", "placement")}
            Sb = r.render_reflect(ds, g, probes, sh, rounds=2, samples=4, **lk)[0].reshape(-1, 3)
            want = (v * Sb + (one - v) * rec[:, 0:3]).astype(np.float32)
            lin, was = res.linear.reshape(-1, 3), base.linear.reshape(-1, 3)
            assert np.array_equal(u32(lin[glossy]), u32(want[glossy])), name                       # glossy pixels: the formula over render_reflect's output
            assert np.array_equal(u32(lin[~glossy]), u32(was[~glossy])), name                      # every other pixel: the frame without reflect
            assert not np.array_equal(u32(lin[glossy]), u32(was[glossy])), name
            ref8, refg, _ = _lib.denoise(np.where(glossy[:, None], want, was).astype(np.float32), rec, None, 16, 16, 0, s["gamma"])
            assert np.array_equal(res.rgb8, ref8) and np.array_equal(u32(res.gamma), u32(refg)), name
        # with direct: the lights at the reflection rays' hits as well, and the receivers' own term added as before
        direct = DirectLight(0.25)
        res = r.render_probe_lit(ds, probes, sh, aov_samples=4, reflect=g, reflect_rounds=2, direct=direct)
        gd = ReflectionGather(8).bias(0.05).seed(6).direct_bias(0.25)
        Sd = r.render_reflect(ds, gd, probes, sh, rounds=2, samples=4)[0].reshape(-1, 3)
        base = r.render_probe_lit(ds, probes, sh, aov_samples=4).linear.reshape(-1, 3)
        mixed = np.where(glossy[:, None], (v * Sd + (one - v) * rec[:, 0:3]).astype(np.float32), base).astype(np.float32)
        want = (mixed + r._direct_term(ds, direct, aov, None)[0].cpu().numpy()).astype(np.float32)
        assert np.array_equal(u32(res.linear.reshape(-1, 3)), u32(want)) and not np.array_equal(Sd, S.reshape(-1, 3))
        for bad in (dict(ao=api.AmbientOcclusion(10.0)), dict(radiance=ProbeRadiance(4, 2, [0.5]), maps=np.zeros((8, 16, 4), np.float32))):
            with pytest.raises(ValueError, match="reflect"):
                r.render_probe_lit(ds, probes, sh, reflect=g, **bad)
    finally:
        ds.close()


def test_cli_round_trip(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    yml = os.path.join(ROOT, "scenes", "ggx_lights.yml")
    base = ["--scene-file", yml, "-s", "2", "--seed", "3"]
    npz, png, plain = str(tmp_path / "p.npz"), str(tmp_path / "r.png"), str(tmp_path / "plain.png")
    assert main(base + ["--bake-probes", "2,2,2", "--probe-min=-30,1,-30", "--probe-max", "30,25,30", "--probe-dirs", "32", "-o", npz]) == 0
    lit = ["--width", "16", "--height", "16", "--aov-samples", "2", "--probe-lit", npz]
    assert main(base + lit + ["--probe-reflect", "8,2", "--reflect-bias", "0.01", "-o", png]) == 0
    assert main(base + lit + ["-o", plain]) == 0
    scene = yaml_io.load_scene(yml)
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(16).height(16).samples(2).use_bvh(True).camera(cam).seed(3)
    with np.load(npz) as z:
        grid = api.ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"])
        want = r.render_probe_lit(scene, grid, z["sh"], 2, reflect=ReflectionGather(8).bias(0.01).seed(3), reflect_rounds=2).rgb8
    img = np.asarray(Image.open(png).convert("RGB"))
    assert img.shape == (16, 16, 3) and np.array_equal(img.reshape(-1, 3), want.reshape(-1, 3))
    assert not np.array_equal(img, np.asarray(Image.open(plain).convert("RGB")))
