"""Every emitter sampled at surface points on the GPU (fw_scene_emitters, fw_emitters_rays, fw_emitters_reduce, fw_bake_emitters and
FW_GATHER_NO_EMITTERS).

k_emitters_rays against api.emitters_rays: the picks equal (float64 + - x / and compares only), rays and weights to one float32 unit in
the last place with the same entries dead, at points the statement keeps clear of its liveness boundaries; one-emitter scenes equal to
fw_area_rays bit for bit; k_emitters_reduce against its statement bit for bit; the records of a resident scene, moved and re-created;
the bake against the public calls chained by hand for two chunkings and progressively; fw_bake_gather with the new flag against its
chain with fw_area_mask over the emitters' objects; the closed forms of tests/test_emitters_surface_cpu.py on the device; a textured
mesh lamp; the Python layer and the CLI."""
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, yaml_io
from firework_amd.api import AreaLight, CheckerTexture, Disk, EmissiveMat, EmitterLights, FinalGather, Rect3d, RenderObject, Rotor3

import area_ref as AR
import emitters_surface_ref as R
import gather_ref as G

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F32 = np.float32
u32 = AR.u32


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _to(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _receivers(n, rng):
    """points below and between the entries of R.mixed_records, normals mostly upwards; four unusable"""
    pos = rng.uniform(-3.0, 3.0, (n, 3)).astype(F32)
    nrm = rng.normal(size=(n, 3)).astype(F32)
    nrm[:, 1] = np.abs(nrm[:, 1]) + 0.3
    pos[1, 0], nrm[4], nrm[7, 2], pos[9, 1] = NAN, 0.0, INF, -INF
    return pos, nrm


# ---- fw_emitters_rays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 64, 200])
@pytest.mark.parametrize("N", [1, 2, 5, 1025])
def test_rays_equal_the_statement(N, S):
    """300 points through a permuted id list cross the 256-entry chunk edge at every S; N = 1025 is above the LDS table (K = 2)"""
    torch, dev = _torch()
    rng = np.random.default_rng(N * 1000 + S)
    rec, _codes = R.mixed_records(N, rng)
    rec[0, 15] = max(rec[0, 15], 0.5)
    cdf, total = _lib.emitters_cdf(rec[:, 15])
    assert total > 0 and np.array_equal(cdf.view(np.uint64), api.emitters_cdf(rec[:, 15])[0].view(np.uint64))
    n = 300
    M = n + 40
    pos, nrm = _receivers(M, rng)
    if rec[0, 1] == 0:
        pos[11] = rec[0, 2:5]                                                                 # inside the first sphere
    for jitter in (True, False):
        em = EmitterLights(S, 1e-3).seed(9).jitter(jitter)
        for rd in (0, 3):
            # points of which no entry lies within 1e-9 of a liveness boundary in the statement (the input changes, not the rule)
            mg = R.liveness_margins(em, rec, cdf, pos, nrm, rd)
            clear = ~np.any(mg < 1e-9, axis=1)
            assert clear.sum() >= n + 20
            ids = rng.permutation(np.nonzero(clear)[0]).astype(np.uint32)[:n]
            want, ww, wp = api.emitters_rays(em, rec, cdf, pos, nrm, ids, rd)
            rays, w, picks = _lib.emitters_rays(em, rec, cdf, pos, nrm, ids, rd)
            what = (N, S, jitter, rd)
            assert rays.shape == (n * S, 6) and w.shape == (n * S,) and picks.shape == (n * S,) and rays.dtype == F32 and picks.dtype == np.uint32
            assert np.array_equal(picks, wp), what
            dead = ww == 0
            assert np.array_equal(w == 0, dead) and 0.01 < dead.mean() < 0.9, (what, dead.mean())
            assert np.all(rays[dead] == 0) and np.all(picks[dead] == R.DEAD)
            assert AR.ulps(rays, want).max() <= 1 and AR.ulps(w, ww).max() <= 1, (what, AR.ulps(rays, want).max(), AR.ulps(w, ww).max())
            if N > 1 and (S > 1 or jitter):
                assert np.unique(picks[~dead]).size > 1 and np.all(rec[picks[~dead], 15] > 0)
            # device arrays on a side stream into the caller's tensors: the host call's bits
            d_rays, d_w = torch.full((n * S, 6), NAN, dtype=torch.float32, device=dev), torch.full((n * S,), NAN, dtype=torch.float32, device=dev)
            d_p = torch.full((n * S,), 7, dtype=torch.int32, device=dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                o, ow, op = _lib.emitters_rays(em, rec, cdf, _to(pos, dev), _to(nrm, dev), _to(ids.astype(np.int32), dev), rd, out=d_rays, weights=d_w, picks=d_p)
            side.synchronize()
            assert o is d_rays and ow is d_w and op is d_p
            assert np.array_equal(u32(d_rays.cpu().numpy()), u32(rays)) and np.array_equal(u32(d_w.cpu().numpy()), u32(w)), what
            assert np.array_equal(d_p.cpu().numpy().view(np.uint32), picks), what
    one = _lib.emitters_rays(EmitterLights(S, 1e-3).seed(9), rec, cdf, pos, nrm, ids[5:6], 3)
    full = _lib.emitters_rays(EmitterLights(S, 1e-3).seed(9), rec, cdf, pos, nrm, ids, 3)
    assert np.array_equal(u32(one[0]), u32(full[0].reshape(n, -1)[5].reshape(-1, 6))) and np.array_equal(u32(one[1]), u32(full[1].reshape(n, -1)[5]))
    assert np.array_equal(one[2], full[2].reshape(n, -1)[5])


@pytest.mark.parametrize("which", ["sphere", "rect"])
def test_one_emitter_scenes_are_the_area_lattice(which):
    """a scene whose only emitter is one sphere or one rectangle: fw_area_rays' rays and weights at Ln = 1, bit for bit"""
    rng = np.random.default_rng(12)
    pos, nrm = _receivers(300, rng)
    ds = _lib.DeviceScene(AR.case_scene("sphere" if which == "sphere" else "rect-off-axis").to_desc())
    try:
        rec, codes = ds.emitters()
        lights = ds.area_lights()
    finally:
        ds.close()
    assert rec.shape == (1, 16) and np.array_equal(u32(rec[:, :14]), u32(lights[:, :14])) and codes.tolist() == [[0, 0]]
    cdf, _t = _lib.emitters_cdf(rec[:, 15])
    assert cdf.tolist() == [1.0]
    for S, rd in ((1, 0), (5, 3), (64, 0), (200, 3)):
        rays, w, picks = _lib.emitters_rays(EmitterLights(S, 1e-3).seed(9), rec, cdf, pos, nrm, None, rd)
        ar, aw = _lib.area_rays(AreaLight(S, 1e-3).seed(9), lights, pos, nrm, None, rd)
        assert np.array_equal(u32(rays), u32(ar)) and np.array_equal(u32(w), u32(aw)) and (w > 0).mean() > 0.3, (S, rd)
        assert np.all(picks[w > 0] == 0) and np.all(picks[w == 0] == R.DEAD)


# ---- fw_emitters_reduce ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 15, 64, 200])
def test_reduce_equals_the_float64_statement(S):
    torch, dev = _torch()
    rng = np.random.default_rng(S)
    n = 21
    picks, w, hits, surface, codes = R.synthetic_entries(n, S, rng)
    ho, hp = hits.view(np.uint32)[:, 10], hits.view(np.uint32)[:, 11]
    acc = api.emitters_reduce(picks, w, ho, hp, surface, codes, S)
    assert np.any(acc[:, 3] > 0) and (S < 5 or np.all(acc[:, 3] < 1))
    hd = np.zeros(n * S, _lib.HIT_DTYPE)
    hd.view(np.uint32).reshape(-1, 12)[:] = hits.view(np.uint32)
    rows = n + 3
    for kind, ids in (("none", None), ("permuted", rng.permutation(rows).astype(np.uint32)[:n])):
        at = np.arange(n) if ids is None else ids.astype(np.int64)
        prior = np.full((rows, 4), NAN, F32)
        prior[at] = rng.uniform(-2.0, 2.0, size=(n, 4)).astype(F32)
        host = prior.copy()
        assert _lib.emitters_reduce(picks, w, hd, surface, codes, S, host, ids) is host
        rest = np.setdiff1d(np.arange(rows), at)
        assert np.array_equal(u32(host[rest]), u32(prior[rest])), (S, kind)
        assert np.array_equal(u32(host[at]), u32(G.add_to(prior[at], acc))), (S, kind)
        for _ in range(2):                                                                     # two runs are bit-equal
            d_sums = _to(prior, dev)
            got = _lib.emitters_reduce(_to(picks.view(np.int32), dev), _to(w, dev), _to(hits, dev), _to(surface, dev), codes, S, d_sums,
                                       None if ids is None else _to(ids.astype(np.int32), dev))
            assert got is d_sums and np.array_equal(u32(d_sums.cpu().numpy()), u32(host)), (S, kind)
    one = _lib.emitters_reduce(picks[3 * S:4 * S], w[3 * S:4 * S], hd[3 * S:4 * S], surface[3 * S:4 * S], codes, S, np.zeros((1, 4), F32))
    assert np.array_equal(u32(one[0]), u32(acc[3].astype(F32)))


# ---- fw_scene_emitters ----------------------------------------------------------------------------------------------------------------
def test_scene_records_follow_updates():
    scene = R.lit_room()
    desc = scene.to_desc()
    ds = _lib.DeviceScene(desc)
    try:
        rec, codes = ds.emitters()
        want, wcodes = _lib.emitters_records(desc)
        assert rec.shape == (1 + 1 + 6 + 8 + 1, 16) and np.array_equal(u32(rec), u32(want)) and np.array_equal(codes, wcodes)
        assert sorted(set(rec[:, 1].tolist())) == [0.0, 2.0, 4.0, 5.0, 9.0] and sorted(set(codes[:, 0].tolist())) == [1, 3, 4, 5, 6]
        lights = ds.area_lights()
        assert np.array_equal(u32(rec[0, :14]), u32(lights[0, :14])) and np.array_equal(u32(rec[1, :14]), u32(lights[1, :14]))
        again = ds.emitters()
        assert np.array_equal(u32(again[0]), u32(rec))
        # fw_scene_update: every kind follows its object
        for i, p in ((1, (1.5, -0.5, 2.0)), (3, (-5.0, 4.0, 1.0)), (4, (7.0, 1.5, -2.0)), (5, (-2.0, 7.0, -5.0)), (6, (5.0, 6.0, 3.0))):
            scene.render_objects[i].position(*p)
        scene.render_objects[5].rotate(Rotor3.from_rotation_xz(0.8))
        ds.update(scene)
        moved, mcodes = ds.emitters()
        want, wcodes = _lib.emitters_records(scene.to_desc())
        assert np.array_equal(u32(moved), u32(want)) and np.array_equal(mcodes, wcodes) and np.array_equal(mcodes, codes)
        assert np.all(np.any(moved[:, 2:14] != rec[:, 2:14], axis=1)) and np.array_equal(moved[:, 14:16], rec[:, 14:16])
    finally:
        ds.close()


def test_records_survive_a_scene_that_is_created_again():
    """a light moved far away raises the meshes' reach, so fw_scene_update creates the scene again behind the handle:
    the records — a mesh lamp's triangles read back from the new allocation among them — are the new scene's, and a bake on the handle
    equals a bake on a fresh scene bit for bit"""
    from firework_amd import scenes
    s, _r = scenes.config("C3_suzanne", 40, 32, 4)
    s.add_object(RenderObject.new(R.grid_mesh(2, 1.0, s.add_material(EmissiveMat.with_color((3.0, 5.0, 2.0))))).rotate(Rotor3.from_rotation_xy(1.2))
                 .position(9.0, 2.0, 0.0))
    pos = np.array([[5.0, 2.0, 0.0], [6.0, 3.0, 1.0], [5.0, 1.0, -2.0]], F32)
    nrm = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, 0.0, 1.0]], F32)
    em = EmitterLights(16, 1e-3).seed(2)
    ds = _lib.DeviceScene(s.to_desc())
    try:
        before, _c = ds.emitters()
        assert before.shape[0] >= 9 and np.array_equal(u32(before), u32(_lib.emitters_records(s.to_desc())[0]))
        light = s.render_objects[int(ds.area_lights()[0, 0])]
        light.position(1.0e4, 0.0, 0.0)
        ds.update(s)
        moved, mcodes = ds.emitters()
        want, wcodes = _lib.emitters_records(s.to_desc())
        assert np.array_equal(u32(moved), u32(want)) and np.array_equal(mcodes, wcodes) and not np.array_equal(moved, before)
        got = ds.bake_emitters(em, pos, nrm, None, rounds=2, seed=3)[1]
        for _ in range(2):
            assert np.array_equal(u32(ds.bake_emitters(em, pos, nrm, None, rounds=2, seed=3)[1]), u32(got))
    finally:
        ds.close()
    fresh = _lib.DeviceScene(s.to_desc())
    try:
        want = fresh.bake_emitters(em, pos, nrm, None, rounds=2, seed=3)[1]
    finally:
        fresh.close()
    assert np.array_equal(u32(got), u32(want)) and np.any(want[:, 0:3] > 0)


# ---- fw_bake_emitters and the gather's complement ---------------------------------------------------------------------------------------
def _every_material_scene():
    """§9z's scene of every material (two emissive spheres, one textured, a ConstantMedium among the occluders) plus a mesh lamp, a
    partial disk and an emissive Rect3d"""
    scene, _ = G.surface_scene(G.environments()["sky"])
    scene.add_object(RenderObject.new(R.grid_mesh(2, 1.5, scene.add_material(EmissiveMat.with_color((6.0, 2.0, 7.0))))).rotate(Rotor3.from_rotation_yz(0.5))
                     .position(-6.0, 5.0, 3.0))
    scene.add_object(RenderObject.new(Disk.partial(1.5, 250.0, 0.4, scene.add_material(EmissiveMat.with_color((1.0, 6.0, 2.0)))))
                     .rotate(Rotor3.from_rotation_xy(0.3)).position(6.0, 4.0, 3.0))
    scene.add_object(RenderObject.new(Rect3d.with_size((2.0, 1.0, 2.0), scene.add_material(EmissiveMat.with_color((3.0, 1.0, 0.5))))).position(0.0, 7.0, 2.0))
    return scene


def _points(n, rng):
    pos = np.stack([rng.uniform(-14, 14, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-3, 5, n)], axis=1).astype(F32)
    nrm = rng.normal(size=(n, 3)).astype(F32)
    nrm[:, 1] = np.abs(nrm[:, 1]) + 0.5
    pos[1, 0], nrm[4], nrm[7, 2] = NAN, 0.0, INF
    return pos, nrm


def _chained(ds, em, rec, codes, cdf, pos, nrm, ids, use_bvh, seed, rounds, first_round=0):
    """fw_emitters_rays, fw_trace_rays, fw_hit_surface and fw_emitters_reduce by hand, on the device over all points"""
    torch, dev = _torch()
    d_pos, d_nrm = _to(pos, dev), _to(nrm, dev)
    d_ids = None if ids is None else _to(ids.astype(np.int32), dev)
    sums = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=dev)
    kinds = set()
    for rd in range(first_round, first_round + rounds):
        rays, w, picks = _lib.emitters_rays(em, rec, cdf, d_pos, d_nrm, d_ids, rd)
        hits = ds.trace(rays, use_bvh, seed=seed + rd)
        surf = ds.hit_surface(rays, hits)
        _lib.emitters_reduce(picks, w, hits, surf, codes, em.samples, sums, d_ids)
        p = picks.cpu().numpy().view(np.uint32)
        kinds |= set(rec[p[p != R.DEAD], 1].tolist())
    return sums.cpu().numpy(), kinds


def test_bake_equals_its_composition_and_is_progressive():
    torch, dev = _torch()
    rng = np.random.default_rng(7)
    n, S, bvh = 23, 16, True
    pos, nrm = _points(n, rng)
    ok = api.ao_usable(pos, nrm)
    em = EmitterLights(S, 1e-3).seed(3)
    ds = _lib.DeviceScene(_every_material_scene().to_desc())
    try:
        rec, codes = ds.emitters()
        cdf, total = _lib.emitters_cdf(rec[:, 15])
        assert rec.shape[0] == 2 + 8 + 1 + 6 and total > 0
        ref, kinds = _chained(ds, em, rec, codes, cdf, pos, nrm, None, bvh, 11, 5)
        assert kinds == {0.0, 4.0, 5.0, 9.0}
        assert np.all(ref[~ok] == 0.0) and np.any(ref[ok, 0:3] > 0.0) and np.any((ref[ok, 3] > 0.0) & (ref[ok, 3] < 5.0)) and np.all(np.isfinite(ref))
        for chunk in (0, 7):
            out, sums, st = ds.bake_emitters(em, pos, nrm, None, rounds=5, chunk=chunk, seed=11, use_bvh=bvh)
            assert np.array_equal(u32(sums), u32(ref)), chunk
            assert np.array_equal(u32(out), u32(api.emitters_resolve(ref, 5))), chunk
            assert 0 < st["rays"] <= int(ok.sum()) * S * 5 and st["ms_render"] > 0, st
        out2, sums, _ = ds.bake_emitters(em, pos, nrm, None, rounds=2, chunk=7, seed=11, use_bvh=bvh)
        assert np.array_equal(u32(out2), u32(api.emitters_resolve(sums, 2)))
        out5, sums5, _ = ds.bake_emitters(em, pos, nrm, None, rounds=3, first_round=2, sums=sums, chunk=0, seed=11, use_bvh=bvh)
        assert sums5 is sums and np.array_equal(u32(sums5), u32(ref)) and np.array_equal(u32(out5), u32(api.emitters_resolve(ref, 5)))
        # device tensors on a side stream, through an id list: entries outside the list are not touched
        ids = rng.permutation(n).astype(np.uint32)[:15]
        rest = np.setdiff1d(np.arange(n), ids)
        ref_ids, _k = _chained(ds, em, rec, codes, cdf, pos, nrm, ids, bvh, 11, 5)
        s0, o0 = np.zeros((n, 4), F32), np.full((n, 4), 7.0, F32)
        s0[rest] = NAN
        d_s, d_o, d_ids = _to(s0, dev), _to(o0, dev), _to(ids.astype(np.int32), dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ds.bake_emitters(em, _to(pos, dev), _to(nrm, dev), d_ids, rounds=2, sums=d_s, out=d_o, chunk=0, seed=11, use_bvh=bvh)
            o, s, _ = ds.bake_emitters(em, _to(pos, dev), _to(nrm, dev), d_ids, rounds=3, first_round=2, sums=d_s, out=d_o, chunk=7, seed=11, use_bvh=bvh,
                                       flags=A.FW_FLAG_TIME_KERNELS)
        side.synchronize()
        assert s is d_s and o is d_o
        o, s = o.cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(u32(s[ids]), u32(ref_ids[ids])) and np.all(np.isnan(s[rest]))
        assert np.array_equal(u32(o[ids]), u32(api.emitters_resolve(ref_ids[ids], 5))) and np.all(o[rest] == 7.0)
    finally:
        ds.close()
    # a scene without emitters: zeros, nothing traced
    bare = api.Scene.new()
    bare.add_object(RenderObject.new(api.XZRect.new(-30.0, 30.0, -8.0, 8.0, -2.0, bare.add_material(api.LambertianMat.with_color((0.5, 0.5, 0.5))))))
    ds = _lib.DeviceScene(bare.to_desc())
    try:
        assert ds.emitters()[0].shape == (0, 16)
        out, sums, st = ds.bake_emitters(em, pos, nrm, None, rounds=2, out=np.full((n, 4), 7.0, F32))
        assert np.all(out == 0.0) and np.all(sums == 0.0) and st["rays"] == 0
    finally:
        ds.close()


def _gather_chain(ds, g, grid, sh, pos, nrm, use_bvh, seed, rounds, objects):
    torch, dev = _torch()
    d_pos, d_nrm, d_sh = _to(pos, dev), _to(nrm, dev), _to(sh, dev)
    sums = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=dev)
    masked = set()
    for rd in range(rounds):
        rays = _lib.ao_rays(g.ao(), d_pos, d_nrm, None, rd)
        hits = ds.trace(rays, use_bvh, seed=seed + rd)
        surf = ds.hit_surface(rays, hits)
        if objects is not None:
            before = (surf[:, 3] == 3.0).cpu().numpy()
            _lib.area_mask(hits, surf, objects)
            gone = before & (surf[:, 3] == -2.0).cpu().numpy()
            masked |= set(hits.cpu().numpy().view(np.uint32)[gone, 10].tolist())
        irr = _lib.probe_irradiance(grid, d_sh, surf[:, 8:11], surf[:, 4:7])
        _lib.gather_reduce(surf, irr, g.directions, sums)
    return sums.cpu().numpy(), masked


def test_gather_without_the_emitters():
    rng = np.random.default_rng(8)
    n, D = 40, 64
    pos, nrm = _points(n, rng)
    pos[10:16] = [(-6.0, 2.0, 3.0), (6.0, 1.5, 3.0), (0.0, 4.0, 3.0), (-5.0, 2.5, 2.5), (5.5, 2.0, 3.5), (0.5, 5.0, 2.5)]      # under the three lamps
    nrm[10:16] = (0.0, 1.0, 0.0)
    grid, sh = G.random_probes((3, 2, 2), rng)
    ds = _lib.DeviceScene(_every_material_scene().to_desc())
    try:
        _rec, codes = ds.emitters()
        objects = np.unique(codes[:, 0]).astype(np.uint32)
        lights = ds.area_lights()
        plain, lamps = FinalGather(D, 1e-3).seed(3), FinalGather(D, 1e-3, no_lights=True).seed(3)
        masking = FinalGather(D, 1e-3, no_emitters=True).seed(3)
        ref_masked, hidden = _gather_chain(ds, masking, grid, sh, pos, nrm, True, 11, 3, objects)
        ref_lamps, _ = _gather_chain(ds, lamps, grid, sh, pos, nrm, True, 11, 3, lights)
        ref_plain, _ = _gather_chain(ds, plain, grid, sh, pos, nrm, True, 11, 3, None)
        n_obj = int(objects.max())                                                              # the mesh, the disk and the box are the last three objects
        assert {n_obj - 2, n_obj - 1, n_obj} <= hidden <= set(objects.tolist()), (hidden, objects)
        assert not np.array_equal(ref_masked, ref_plain) and not np.array_equal(ref_masked, ref_lamps)
        for chunk in (0, 7):
            out, sums, _ = ds.bake_gather(masking, grid, sh, pos, nrm, None, rounds=3, chunk=chunk, seed=11)
            assert np.array_equal(u32(sums), u32(ref_masked)) and np.array_equal(u32(out), u32(api.gather_resolve(ref_masked, 3))), chunk
            out, sums, _ = ds.bake_gather(plain, grid, sh, pos, nrm, None, rounds=3, chunk=chunk, seed=11)      # flags 0 and 4: the bits of before
            assert np.array_equal(u32(sums), u32(ref_plain)), chunk
            out, sums, _ = ds.bake_gather(lamps, grid, sh, pos, nrm, None, rounds=3, chunk=chunk, seed=11)
            assert np.array_equal(u32(sums), u32(ref_lamps)), chunk
        with pytest.raises(_lib.FireworkError) as e:
            ds.bake_gather(FinalGather(D, 1e-3, no_lights=True, no_emitters=True), grid, sh, pos, nrm, None, rounds=1)
        assert e.value.status == A.FW_ERR_BAD_ARG and "gather flags" in str(e.value)
    finally:
        ds.close()


# ---- known answers --------------------------------------------------------------------------------------------------------------------
DISK_CASES = ("annulus", "disk", "five", "sector")


@pytest.mark.parametrize("name, use_bvh", [(n, b) for n in sorted(R.cases()) for b in (False, True) if not (b and n in DISK_CASES)])
def test_known_answers_on_the_device(name, use_bvh):
    """tests/test_emitters_surface_cpu.py's closed forms and tolerances (MEASURED x MARGIN: the statement's own error at this S, rounds
    and seed), with the scene really traced: a box's far faces are hidden by the box itself.  Every case through the linear object list
    (use_bvh=False), and every case without a Disk through the TLAS as well: under use_bvh a Disk is tested only where the ray meets the
    reference's own degenerate box for it (disk.rs:85-90, OF_GATE), so a lone unrotated disk is as good as invisible there — the
    scene's rule, which the path tracer follows too, not the sampler's"""
    point, normal, E = R.cases()[name]
    ds = _lib.DeviceScene(R.case_scene(name).to_desc())
    try:
        out, _s, st = ds.bake_emitters(EmitterLights(R.S, 0.0).seed(R.SEED), np.array([point], F32), np.array([normal], F32), None, rounds=R.ROUNDS,
                                       use_bvh=use_bvh)
    finally:
        ds.close()
    err = float(np.max(np.abs(out[0, 0:3].astype(np.float64) - E) / E))
    print(f"{name}: closed form {E}, device {out[0]}, relative error {err:.4e} (allowed {R.MARGIN * R.MEASURED[name]:.4e})")
    assert 0 < st["rays"] <= R.S * R.ROUNDS
    assert err <= R.MARGIN * R.MEASURED[name]
    assert (out[0, 3] == 1.0) == (name not in ("face", "five"))


def test_a_textured_mesh_lamp():
    """a checker on the mesh lamp: the sums equal the numpy statement fed the device's own picks, weights, hits and fw_hit_surface
    records, bit for bit; both of the checker's colours arrive; every sum is finite"""
    tex = CheckerTexture.with_colors((6.0, 0.5, 0.0), (0.0, 2.5, 7.0), 1.5)
    rng = np.random.default_rng(4)
    pos, nrm = R.floor_points(40, rng, 9.0)
    em = EmitterLights(64, 1e-3).seed(2)
    ds = _lib.DeviceScene(R.lit_room(EmissiveMat.new(tex)).to_desc())
    try:
        rec, codes = ds.emitters()
        cdf, _t = _lib.emitters_cdf(rec[:, 15])
        want = np.zeros((40, 4), F32)
        colours = set()
        for rd in range(2):
            rays, w, picks = _lib.emitters_rays(em, rec, cdf, pos, nrm, None, rd)
            hits = ds.trace(rays, True, seed=5 + rd)
            surf = ds.hit_surface(rays, hits)
            on_mesh = (surf[:, 3] == 3.0) & (hits["object"] == 5) & (w > 0)
            colours |= {tuple(c) for c in surf[on_mesh][:, 12:15].tolist()}
            want = G.add_to(want, api.emitters_reduce(picks, w, hits["object"], hits["prim"], surf, codes, 64))
        _o, sums, _ = ds.bake_emitters(em, pos, nrm, None, rounds=2, seed=5)
    finally:
        ds.close()
    assert colours == {(6.0, 0.5, 0.0), (0.0, 2.5, 7.0)}
    assert np.array_equal(u32(sums), u32(want)) and np.all(np.isfinite(sums)) and np.all(sums[:, 0:3] > 0) and np.all(sums[:, 3] > 0)


# ---- the Python layer and the CLI -----------------------------------------------------------------------------------------------------
def _room_renderer(w, h):
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    return api.Renderer.default().width(w).height(h).samples(2).use_bvh(True).camera(cam).seed(3)


def test_render_probe_lit_with_the_split_is_its_composition():
    torch, dev = _torch()
    from firework_amd.api import ProbeGrid, ProbeSet
    r = _room_renderer(32, 24)
    probes = ProbeSet.grid((-12.0, 0.5, -12.0), (12.0, 8.0, 12.0), (2, 2, 2), 65)
    g, em = FinalGather(33, 0.01).seed(6), EmitterLights(8, 0.01).seed(6)
    s = r.settings
    ds = _lib.DeviceScene(R.lit_room().to_desc())
    try:
        sh, _sums = r.bake_probes(ds, probes, 1)
        aov = ds.aovs(r, 4, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        grid = ProbeGrid.of(probes, True)
        res = r.render_probe_lit(ds, probes, sh, aov_samples=4, gather=g, gather_rounds=2, emitters=em, emitters_rounds=3)
        Eg, _s, _ = ds.bake_gather(FinalGather(33, 0.01, no_emitters=True).seed(6), grid, _to(sh, dev), aov[:, 8:11], aov[:, 4:7], None, rounds=2,
                                   seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        Ee, _s, _ = ds.bake_emitters(em, aov[:, 8:11], aov[:, 4:7], None, rounds=3, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        Eg, Ee = Eg.cpu().numpy(), Ee.cpu().numpy()
        assert np.any(Ee[:, 0:3] > 0) and np.any((Ee[:, 3] > 0) & (Ee[:, 3] < 1)) and r.emitters_stats["rays"] > 0
        inv_pi, one = F32(1.0 / np.pi), F32(1.0)
        v = rec[:, 3:4]
        want = (rec[:, 0:3] * (v * ((Eg[:, 0:3] + Ee[:, 0:3]) * inv_pi) + (one - v))).astype(F32)
        assert np.array_equal(u32(res.linear), u32(want))
        ref8, refg, _ = _lib.denoise(want, rec, None, 32, 24, 0, s["gamma"])
        assert np.array_equal(res.rgb8, ref8) and np.array_equal(u32(res.gamma), u32(refg))
        a = r.render_probe_lit(ds, probes, sh, aov_samples=4, gather=g, gather_rounds=2)
        b = r.render_probe_lit(ds, probes, sh, aov_samples=4, gather=g, gather_rounds=2, emitters=None)
        assert np.array_equal(u32(a.linear), u32(b.linear)) and not np.array_equal(u32(a.linear), u32(res.linear))
        with pytest.raises(ValueError, match="twice"):
            r.render_probe_lit(ds, probes, sh, emitters=em)
        with pytest.raises(ValueError, match="exclude"):
            r.render_probe_lit(ds, probes, sh, gather=g, emitters=em, area=AreaLight(4))
        only = r.render_emitters(ds, em, rounds=3, aov_samples=4)
        want = (rec[:, 0:3] * ((v * Ee[:, 0:3]) * inv_pi)).astype(F32)
        assert np.array_equal(u32(only.linear), u32(want))
    finally:
        ds.close()


def test_cli_round_trip(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    yml = str(tmp_path / "room.yml")
    yaml_io.save_scene(R.lit_room(), yml)
    base = ["--scene-file", yml, "-s", "2", "--seed", "3", "--width", "16", "--height", "16", "--aov-samples", "2"]
    npz, png, split = str(tmp_path / "p.npz"), str(tmp_path / "a.png"), str(tmp_path / "s.png")
    assert main(base + ["--emitter-light", "4,2", "--emitter-bias", "0.01", "-o", png]) == 0
    assert main(["--scene-file", yml, "-s", "2", "--seed", "3", "--bake-probes", "2,2,2", "--probe-min=-12,0.5,-12", "--probe-max", "12,8,12", "--probe-dirs", "32",
                 "-o", npz]) == 0
    assert main(base + ["--probe-lit", npz, "--probe-gather", "9", "--emitter-light", "4", "-o", split]) == 0
    scene = yaml_io.load_scene(yml)
    r = _room_renderer(16, 16)
    want = r.render_emitters(scene, EmitterLights(4, 0.01).seed(3), 2, 2).rgb8
    img = np.asarray(Image.open(png).convert("RGB"))
    assert img.shape == (16, 16, 3) and np.array_equal(img.reshape(-1, 3), want.reshape(-1, 3)) and img.max() > 0
    with np.load(npz) as z:
        grid = api.ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"])
        want = r.render_probe_lit(scene, grid, z["sh"], 2, gather=FinalGather(9, 1e-3).seed(3), emitters=EmitterLights(4, 1e-3).seed(3)).rgb8
    img = np.asarray(Image.open(split).convert("RGB"))
    assert np.array_equal(img.reshape(-1, 3), want.reshape(-1, 3))
