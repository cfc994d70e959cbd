"""Irradiance probes baked on the GPU (fw_probe_rays, fw_probe_project, fw_bake_probes).

k_probe_rays against the numpy float64 statement (api.ProbeSet.rays) to one float32 ulp at each vector's scale, origins bit-equal;
k_probe_project against api.sh_project within a bound derived from its construction; fw_bake_probes against its composition from the
three public calls bit for bit, for every chunk size, through sums, on a side stream, under light sampling and with a point light; a
furnace and a sky against closed forms; fw_render left untouched; a NaN position refused.

The projection's bound (tests/probes_ref.py: project_bound).  The kernel forms proj in float64, rounds it to float32 once and adds it to
the running float32 sum with one addition.  Against the float64 reference ref = api.sh_project(...) of the same float32 inputs:
  - float64 inside: each term Y_k a_j / S carries a few roundings and passes through at most ceil(D / 64) sequential additions and 6
    tree levels on the device, D additions in numpy: at most (D + ceil(D / 64) + 40) 2^-53 T, with T = (4 pi / D) sum_j |Y_k a_j / S|;
  - the rounding of proj to float32: at most 2^-24 |proj| (2^-150 where subnormal);
  - the float32 addition: at most 2^-24 |sums_in + proj32|.
Nothing in it is measured: T, ref and sums_in come from the test's own inputs."""
import copy
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import ColorEnv, EmissiveMat, LambertianMat, ProbeSet, RenderObject, Scene, SkyEnv, Sphere

import probes_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(n, d) for n in (1, 3) for d in (1, 63, 64, 65, 200)]     # one entry, a wave's tail, a wave, a wave plus one, strides and a tail
ROUNDS = [0, 5, (1 << 31) + 3]
SEEDS = [0, 7, 0x1234567800000009]                                  # the last one exercises the 64-bit seed fold
FAR = np.array([[3e3, -2e3, 5e3], [3001.25, -1999.5, 5000.125], [2999.0, -2000.75, 4998.5]], np.float32)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def assert_rays_close(got, ref, what):
    """per component |gpu - ref| <= 2^-23 x the largest magnitude among that vector's three reference components (both sides round the
    same float64 expression, whose libm results differ by a few float64 ulps); every entry compared and finite; origins bit-equal"""
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.all(np.isfinite(got)), what
    g, r = got.astype(np.float64).reshape(-1, 2, 3), ref.astype(np.float64).reshape(-1, 2, 3)
    bound = 2.0 ** -23 * np.abs(r).max(axis=2, keepdims=True)
    err = np.abs(g - r)
    assert np.all(err <= bound), (what, float((err / bound).max()), np.argwhere(err > bound)[:4])
    assert np.array_equal(_u32(got[:, :3]), _u32(ref[:, :3])), what


@pytest.mark.parametrize("n,D", SHAPES)
def test_rays_match_the_numpy_statement(n, D):
    import torch
    dev = torch.device("cuda", 0)
    for rnd in ROUNDS:
        for seed in SEEDS:
            for jitter in (True, False):
                probes = ProbeSet(FAR[:n], D).seed(seed).jitter(jitter)
                ref = probes.rays(rnd)
                what = f"{n} x {D} round {rnd} seed {seed:#x} jitter {jitter}"
                assert_rays_close(_lib.probe_rays(probes, rnd), ref, what + " host")
                out = torch.full((n * D, 6), float("nan"), dtype=torch.float32, device=dev)
                assert_rays_close(_lib.probe_rays(probes, rnd, out=out).cpu().numpy(), ref, what + " device")
                if n > 1:                                              # first_probe > 0: the shift is the absolute probe's
                    assert_rays_close(_lib.probe_rays(probes, rnd, first_probe=1, n=n - 1), ref[D:], what + " host from 1")
                    out = torch.full((D, 6), float("nan"), dtype=torch.float32, device=dev)
                    assert_rays_close(_lib.probe_rays(probes, rnd, first_probe=2, n=1, out=out).cpu().numpy(), ref[2 * D:], what + " device from 2")
    a = ProbeSet(FAR[:n], D).seed(7)
    assert not np.array_equal(_lib.probe_rays(a, 0), _lib.probe_rays(a, 1))
    assert not np.array_equal(_lib.probe_rays(a, 0), _lib.probe_rays(ProbeSet(FAR[:n], D).seed(8), 0))


def synthetic_accum(rays, samples, seed):
    """sums of `samples` samples of a radiance with constant, linear and quadratic parts and per-entry noise of both signs"""
    d = rays[:, 3:].astype(np.float64)
    rng = np.random.default_rng(seed)
    L = np.stack([0.7 + 0.5 * d[:, 1] + 0.3 * d[:, 0] * d[:, 2], 1.5 - 0.8 * d[:, 2] + 0.6 * (d[:, 1] ** 2 - 0.2),
                  0.2 + 0.4 * d[:, 0] - 0.9 * d[:, 0] * d[:, 1]], axis=1) + rng.uniform(-2.0, 2.0, (rays.shape[0], 3))
    acc = np.empty((rays.shape[0], 4), np.float32)
    acc[:, :3] = (L * samples).astype(np.float32)
    acc[:, 3] = rng.integers(1, 9, rays.shape[0]) * samples              # (segments: not read)
    return acc


@pytest.mark.parametrize("n,D", SHAPES)
def test_projection_matches_the_float64_statement(n, D):
    import torch
    probes = ProbeSet(FAR[:n], D).seed(7)
    d_rays = _lib.probe_rays(probes, 5, out=torch.full((n * D, 6), float("nan"), dtype=torch.float32, device="cuda"))
    rays = d_rays.cpu().numpy()
    for S in (1, 7):
        acc = synthetic_accum(rays, S, 100 * n + D + S)
        ref = api.sh_project(rays, acc, S, D)
        T = P.abs_terms(api, rays, acc, S, D)
        zero = np.zeros((n, 9, 3), np.float32)
        # host arrays and device tensors, from zero
        got_h = _lib.probe_project(rays, acc, S, D)
        d_acc = torch.from_numpy(acc).cuda()
        got_d = _lib.probe_project(d_rays, d_acc, S, D).cpu().numpy()
        for got in (got_h, got_d):
            err = np.abs(got.astype(np.float64) - ref)
            bound = P.project_bound(ref, T, zero, D)
            assert np.all(err <= bound), (n, D, S, float((err / bound).max()))
        assert np.array_equal(_u32(got_h), _u32(got_d))
        assert np.array_equal(_u32(_lib.probe_project(d_rays, d_acc, S, D).cpu().numpy()), _u32(got_d))          # two runs: bit-equal
        # non-zero incoming sums are added to
        before = np.random.default_rng(S).uniform(-3.0, 3.0, (n, 9, 3)).astype(np.float32)
        d_sums = torch.from_numpy(before.copy()).cuda()
        assert _lib.probe_project(d_rays, d_acc, S, D, sums=d_sums) is d_sums
        got = d_sums.cpu().numpy()
        err = np.abs(got.astype(np.float64) - (before.astype(np.float64) + ref))
        bound = P.project_bound(ref, T, before, D)
        assert np.all(err <= bound), (n, D, S, float((err / bound).max()))
        assert np.array_equal(_u32(got), _u32(before + got_d))                                                   # one float32 addition
        h_sums = before.copy()
        _lib.probe_project(rays, acc, S, D, sums=h_sums)
        assert np.array_equal(_u32(h_sums), _u32(got))
        # a probe's coefficients do not depend on its neighbours: permute the probes and the outputs permute
        if n > 1:
            perm = np.array([2, 0, 1])
            pr = np.ascontiguousarray(rays.reshape(n, D, 6)[perm].reshape(-1, 6))
            pa = np.ascontiguousarray(acc.reshape(n, D, 4)[perm].reshape(-1, 4))
            assert np.array_equal(_u32(_lib.probe_project(torch.from_numpy(pr).cuda(), torch.from_numpy(pa).cuda(), S, D).cpu().numpy()),
                                  _u32(got_d[perm]))


def _with(r, **settings):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    rr.settings.update(settings)
    return rr


def chained(ds, r, probes, rounds, first_round=0, sums=None):
    """the three public calls by hand, on the device, over the whole set: (sh, sums, rays traced)"""
    import torch
    s = r.settings
    n, D = probes.n_probes, probes.directions
    if sums is None:
        sums = torch.zeros((n, 9, 3), dtype=torch.float32, device="cuda")
    traced = 0
    for rnd in range(first_round, first_round + rounds):
        rays = _lib.probe_rays(probes, rnd, out=torch.empty((n * D, 6), dtype=torch.float32, device="cuda"))
        res = ds.render_rays(rays, s["samples"], 0, None, seed=s["seed"] + rnd, use_bvh=s["use_bvh"], paths_per_batch=s["paths_per_batch"],
                             flags=s["flags"])
        traced += res.stats["rays"]
        _lib.probe_project(rays, res.accum, s["samples"], D, sums=sums)
    sh = (sums.cpu().numpy().astype(np.float64) / float(first_round + rounds)).astype(np.float32)
    return sh, sums.cpu().numpy(), traced


def assert_bake_equals(ds, r, probes, rounds, ref, what):
    sh_ref, sums_ref, traced = ref
    for chunk in (1, 2, 0):
        sh, sums = r.bake_probes(ds, probes, rounds, chunk=chunk)
        assert np.array_equal(_u32(sums), _u32(sums_ref)), (what, chunk)
        assert np.array_equal(_u32(sh), _u32(sh_ref)), (what, chunk)
        assert r.probe_stats["rays"] == traced, (what, chunk)
        assert r.probe_stats["n_batches"] >= rounds * (1 if chunk == 0 else -(-probes.n_probes // chunk)) and r.probe_stats["ms_render"] > 0


@pytest.mark.parametrize("name,bvh,positions", [("conics", False, [[0.0, 2.0, 0.0], [1.5, 3.0, 1.0], [-2.0, 1.5, 0.5]]),
                                                ("C3_suzanne", True, [[0.0, 0.0, 3.0], [2.0, 1.0, 0.5], [-1.5, 0.5, 2.0]])])
def test_bake_equals_its_composition(name, bvh, positions):
    import torch
    scene, r = scenes.config(name, 8, 8, 4)
    r = _with(r, use_bvh=bvh, seed=11)
    probes = ProbeSet(positions, 65).seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ref = chained(ds, r, probes, 3)
        assert ref[2] >= 3 * 65 * 4 * 3 and np.abs(ref[1]).max() > 0
        assert_bake_equals(ds, r, probes, 3, ref, name)
        # progressive: 1 + 2 rounds through sums equal 3 rounds in one call (host arrays, and the composition's own two calls)
        sh1, sums = r.bake_probes(ds, probes, 1, chunk=2)
        c1 = chained(ds, r, probes, 1)
        assert np.array_equal(_u32(sums), _u32(c1[1])) and np.array_equal(_u32(sh1), _u32(c1[0])) and np.array_equal(_u32(sh1), _u32(sums))
        sh3, sums3 = r.bake_probes(ds, probes, 2, first_round=1, sums=sums, chunk=1)
        assert sums3 is sums
        assert np.array_equal(_u32(sums3), _u32(ref[1])) and np.array_equal(_u32(sh3), _u32(ref[0]))
        # device tensors on a side stream
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            d_sh1, d_sums = r.bake_probes(ds, probes, 1, on_device=True, chunk=2)
            d_sh, d_sums2 = r.bake_probes(ds, probes, 2, first_round=1, sums=d_sums, chunk=0)
        side.synchronize()
        assert d_sh.is_cuda and d_sums2 is d_sums
        assert np.array_equal(_u32(_host(d_sums)), _u32(ref[1])) and np.array_equal(_u32(_host(d_sh)), _u32(ref[0]))
        assert np.array_equal(_u32(_host(d_sh1)), _u32(c1[0]))
        # timing changes no bit, and the two kernels' time is reported
        t = _with(r, flags=r.settings["flags"] | A.FW_FLAG_TIME_KERNELS)
        sh_t, sums_t = t.bake_probes(ds, probes, 3, chunk=2)
        assert np.array_equal(_u32(sums_t), _u32(ref[1]))
        assert t.probe_stats["ms_raygen"] > 0 and t.probe_stats["ms_accumulate"] > 0 and t.probe_stats["ms_render"] >= t.probe_stats["ms_raygen"]
    finally:
        ds.close()


def test_bake_under_light_sampling_and_with_a_point_light():
    from firework_amd import yaml_io
    # cornell under FW_FLAG_LIGHT_SAMPLING: the composition holds and the flag is in force
    scene, r = scenes.config("C2_cornell_box", 8, 8, 4)
    probes = ProbeSet([[278.0, 278.0, 278.0], [100.0, 400.0, 150.0], [450.0, 60.0, 500.0]], 65).seed(5)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        plain, ls = _with(r, seed=5), _with(r, seed=5).light_sampling()
        ref = chained(ds, ls, probes, 3)
        assert_bake_equals(ds, ls, probes, 3, ref, "cornell light sampling")
        assert not np.array_equal(_u32(plain.bake_probes(ds, probes, 3)[1]), _u32(ref[1]))
    finally:
        ds.close()
    # a scene whose lights are a point, a spot and a directional light
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "three_lights.yml"))
    assert len(scene.lights) > 0
    r = api.Renderer.default().samples(4).use_bvh(True).seed(9)
    probes = ProbeSet([[0.0, 1.0, 0.0], [1.0, 0.5, 1.0], [-1.0, 2.0, 0.5]], 65).seed(5)
    desc = scene.to_desc()
    ds = _lib.DeviceScene(desc)
    try:
        ref = chained(ds, r, probes, 3)
        assert_bake_equals(ds, r, probes, 3, ref, "three lights")
        ds.set_lights([])
        assert not np.array_equal(_u32(r.bake_probes(ds, probes, 3)[1]), _u32(ref[1]))     # the lights were honoured
    finally:
        ds.close()


def test_furnace():
    """a probe off-centre inside a closed emitting sphere under a black environment: every path ends on the emitter with Le, so the
    projection is the constant's: c0 = 2 sqrt(pi) Le, and all nine equal api.sh_project of the constant on the same rays"""
    Le = np.array([2.0, 0.75, 3.5])
    scene = Scene.new()
    m = scene.add_material(EmissiveMat.with_color(tuple(Le)))
    scene.add_object(RenderObject.new(Sphere.new(10.0, m)).position(0.0, 0.0, 0.0))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    D = 200
    probes = ProbeSet([[3.0, -2.0, 1.0]], D).seed(4)
    r = api.Renderer.default().samples(1).use_bvh(True).seed(2)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        for bvh in (False, True):
            sh, sums = _with(r, use_bvh=bvh).bake_probes(ds, probes, 1)
            rays = _lib.probe_rays(probes, 0)
            acc = np.zeros((D, 4), np.float32)
            acc[:, :3] = Le.astype(np.float32)
            ref = api.sh_project(rays, acc, 1, D)
            bound = P.project_bound(ref, P.abs_terms(api, rays, acc, 1, D), np.zeros((1, 9, 3), np.float32), D)
            err = np.abs(sums.astype(np.float64) - ref)
            assert np.all(err <= bound), (bvh, float((err / bound).max()))
            c0 = 2.0 * np.sqrt(np.pi) * Le.astype(np.float32).astype(np.float64)
            assert np.all(np.abs(sums[0, 0].astype(np.float64) - c0) <= bound[0, 0] + 2.0 ** -50 * c0), bvh
            assert np.array_equal(_u32(sh), _u32(sums))
    finally:
        ds.close()


def test_sky():
    """a sky seen from a probe whose rays all miss the one small sphere far below: sh equals the projection of the analytic sky on the
    same rays, and the irradiance on +-y the closed form within the lattice's C / D bound.
    The bound of sh against api.sh_project(analytic sky): per round project_bound, plus the float32 evaluation of the sky in the shader —
    t = 0.5 (y + 1) and (1 - t) h + t z are five float32 roundings of values at most max(h, z) <= 1, so the radiance is within
    5 x 2^-24 of the float64 sky and the projection within 5 x 2^-24 T1, T1 = (4 pi / D) sum_j |Y_k|; sh = sums / rounds adds one more
    rounding, 2^-24 |sh|."""
    hor, zen = np.array([1.0, 1.0, 1.0]), np.array([0.5, 0.7, 1.0])
    scene = Scene.new()
    m = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(0.001, m)).position(0.3, -1000.0, 0.2))
    scene.set_environment(SkyEnv(tuple(zen), tuple(hor)))
    D, rounds = 256, 4
    probes = ProbeSet([[1.0, 2.0, -3.0]], D).seed(6)
    r = api.Renderer.default().samples(1).use_bvh(True).seed(1)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        per_round = [_lib.probe_rays(probes, k) for k in range(rounds)]
        for rays in per_round:
            assert np.all(ds.trace(rays, True)["object"] == A.FW_NO_HIT)
        sh, sums = r.bake_probes(ds, probes, rounds)
    finally:
        ds.close()
    ref = np.zeros((1, 9, 3))
    bound = np.zeros((1, 9, 3))
    for rays in per_round:
        d = rays[:, 3:].astype(np.float64)
        acc = np.zeros((D, 4))
        acc[:, :3] = hor + 0.5 * (d[:, 1:2] + 1.0) * (zen - hor)
        proj = api.sh_project(rays, acc, 1, D)
        T1 = (4.0 * np.pi / D) * np.abs(api.sh_basis(d)).sum(axis=0)[None, :, None]
        # (sums before this round: the rounds so far, within their own bounds — |ref| + bound bounds them)
        bound = bound + P.project_bound(proj, P.abs_terms(api, rays, acc, 1, D), np.abs(ref) + bound, D) + 5.0 * 2.0 ** -24 * T1
        ref = ref + proj
    assert np.all(np.abs(sums.astype(np.float64) - ref) <= bound), float((np.abs(sums - ref) / bound).max())
    sh_bound = bound / rounds + 2.0 ** -24 * (np.abs(ref) / rounds + bound)
    assert np.all(np.abs(sh.astype(np.float64) - ref / rounds) <= sh_bound)
    # the irradiance on +-y against the closed form: the lattice's error of every coefficient (mean of the rounds' errors, each within
    # C_k / D), plus the float32 bound above, weighted by the cosine lobe's factors
    normals = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    closed = np.pi * (hor + zen) / 2.0 + (np.pi / 3.0) * (zen - hor) * normals[:, 1:2]
    sky = lambda x: hor + 0.5 * (x[..., 1:2] + 1.0) * (zen - hor)                          # noqa: E731
    coeff = np.array([[P.quadrature_bound(lambda x, k=k, c=c: api.sh_basis(x)[..., k] * sky(x)[..., c], D) for c in range(3)] for k in range(9)])
    weight = np.abs(api.sh_basis(normals) * api._SH_COSINE)                                 # (2, 9)
    E = api.sh_irradiance(sh[0], normals)
    assert np.all(np.abs(E - closed) <= weight @ (coeff + sh_bound[0])), np.abs(E - closed)


@pytest.mark.parametrize("graph", [None, "1"])
def test_render_untouched(graph):
    """fw_render before and after a bake is bit-identical; under GRAPH its repeated frame is still replayed (bit 31)"""
    scene, r = scenes.config("C2_cornell_box", 48, 32, 4)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        with _lib.options(GRAPH=graph):
            before = [ds.render(r) for _ in range(3)]
            for chunk in (3, 0):
                r.bake_probes(ds, probes, 2, chunk=chunk)
                assert r.probe_stats["reserved"] & 0x80000000 == 0
            after = [ds.render(r) for _ in range(2)]
        for a in before[1:] + after:
            assert np.array_equal(a.rgb8, before[0].rgb8)
            assert np.array_equal(_u32(a.linear), _u32(before[0].linear))
            assert a.stats["rays"] == before[0].stats["rays"]
        if graph:
            assert before[2].stats["reserved"] & 0x80000000 and after[1].stats["reserved"] & 0x80000000
    finally:
        ds.close()


def test_non_finite_position_is_refused():
    scene, r = scenes.config("conics", 8, 8, 2)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        good = ProbeSet([[0.0, 2.0, 0.0], [1.0, 2.0, 0.0]], 63).seed(1)
        first = r.bake_probes(ds, good, 1)[1]
        bad = ProbeSet([[0.0, 2.0, 0.0], [1.0, float("nan"), 0.0]], 63).seed(1)
        sums = np.full((2, 9, 3), 7.0, np.float32)
        with pytest.raises(_lib.FireworkError) as e:
            r.bake_probes(ds, bad, 1, sums=sums)
        assert e.value.status == A.FW_ERR_BAD_ARG and "probe 1 " in str(e.value)
        assert np.all(sums == 7.0)                                                       # refused before any launch
        with pytest.raises(_lib.FireworkError):
            _lib.probe_rays(bad, 0)
        assert np.array_equal(_u32(r.bake_probes(ds, good, 1)[1]), _u32(first))           # the next call is unaffected
    finally:
        ds.close()
