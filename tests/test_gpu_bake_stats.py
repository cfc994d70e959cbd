"""The fw_stats of the chunked entry points (fw_bake_probes, fw_bake_lightmap, fw_render_model, fw_render_views, and the traced bakes
fw_bake_probe_depth, fw_bake_ao and fw_relocate_probes) against the same work made by hand, one public call per chunk: every counter is
the sum over the chunks, the generator's and the reducer's bytes come on top (the traced bakes add none), the tree sizes and `reserved`
are the last chunk's, and the per-class times are reported with FW_FLAG_TIME_KERNELS and zero without it.
The shapes are the smallest with a chunk boundary and a ragged last chunk; the sums and frames are compared bit for bit as well, so the
hand-made chunks are known to be the call's own."""
import copy

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import (AmbientOcclusion, CameraModel, ProbeDepth, ProbeRelocation, ProbeSet, RenderObject, Rotor3, orbit_cameras)

import lightmap_ref as R

pytestmark = pytest.mark.gpu

SCENES = [("conics", False), ("C3_suzanne", True)]
POSITIONS = {"conics": [[0.0, 2.0, 0.0], [1.5, 3.0, 1.0], [-2.0, 1.5, 0.5], [0.5, 2.5, -1.0], [-1.0, 3.5, 1.5]],
             "C3_suzanne": [[0.0, 0.0, 3.0], [2.0, 1.0, 0.5], [-1.5, 0.5, 2.0], [1.0, -0.5, 2.5], [-2.0, 1.5, 1.0]]}
SUMMED = ("samples", "rays", "n_batches", "n_extend_launches", "n_shade_launches", "deposits", "parked_rays", "algorithmic_bytes",
          "bytes_extend", "bytes_shade")
LATEST = ("tlas_nodes", "blas_nodes", "reserved")
CLASSES = ("ms_raygen", "ms_extend", "ms_shade", "ms_accumulate")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _with(r, **settings):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    rr.settings.update(settings)
    return rr


def _timed(r):
    return _with(r, flags=r.settings["flags"] | A.FW_FLAG_TIME_KERNELS)


def assert_counters(total, parts, gen_bytes, red_bytes, what):
    """total: the call's stats; parts: the stats of the hand-made chunks in the call's order; gen_bytes / red_bytes: what the call's
    generator and reducer move on top of the chunks' renders"""
    assert len(parts) >= 2, what
    for f in SUMMED:
        assert total[f] == sum(p[f] for p in parts), (what, f)
    depth = np.sum([np.array(p["rays_per_depth"], np.uint64) for p in parts], axis=0)
    assert [int(x) for x in total["rays_per_depth"]] == [int(x) for x in depth], what
    assert total["rays"] == int(depth.sum()) > 0, what
    assert total["bytes_raygen"] == sum(p["bytes_raygen"] for p in parts) + gen_bytes, what
    assert total["bytes_accumulate"] == sum(p["bytes_accumulate"] for p in parts) + red_bytes, what
    for f in LATEST:
        assert total[f] == parts[-1][f], (what, f)


def assert_times(plain, timed, what):
    """without FW_FLAG_TIME_KERNELS no class time is reported, only the whole render's; with it every class has one"""
    for f in CLASSES:
        assert plain[f] == 0.0, (what, f)
        assert timed[f] > 0, (what, f)
    assert plain["ms_render"] > 0 and timed["ms_render"] >= timed["ms_raygen"], what


def assert_trace_counters(total, parts, what):
    """assert_counters for the traced bakes: the parts are fw_trace_rays' stats, which count no rays per depth, and the call's generator
    and reducer add no bytes of their own"""
    assert len(parts) >= 2, what
    for f in SUMMED:
        assert total[f] == sum(p[f] for p in parts), (what, f)
    depth = np.sum([np.array(p["rays_per_depth"], np.uint64) for p in parts], axis=0)
    assert [int(x) for x in total["rays_per_depth"]] == [int(x) for x in depth], what
    assert total["rays"] > 0, what
    assert total["bytes_raygen"] == sum(p["bytes_raygen"] for p in parts), what
    assert total["bytes_accumulate"] == sum(p["bytes_accumulate"] for p in parts), what
    for f in LATEST:
        assert total[f] == parts[-1][f], (what, f)


def assert_trace_times(plain, timed, what):
    """a traced bake's own two kernels: their time joins ms_render always, and ms_raygen / ms_accumulate only with FW_FLAG_TIME_KERNELS"""
    assert plain["ms_raygen"] == 0.0 and plain["ms_accumulate"] == 0.0 and plain["ms_render"] > 0, what
    assert timed["ms_raygen"] > 0 and timed["ms_accumulate"] > 0, what


def _render_chunk(ds, r, rays, samples, rnd, key_base):
    s = r.settings
    return ds.render_rays(rays, samples, 0, None, key_base=key_base, seed=s["seed"] + rnd, use_bvh=s["use_bvh"],
                          paths_per_batch=s["paths_per_batch"], flags=s["flags"])


@pytest.mark.parametrize("name,bvh", SCENES)
def test_bake_probes_stats_are_its_chunks(name, bvh):
    import torch
    N, D, S, ROUNDS, CHUNK = 5, 16, 2, 2, 2
    scene, r = scenes.config(name, 8, 8, S)
    r = _with(r, use_bvh=bvh, seed=11)
    probes = ProbeSet(POSITIONS[name], D).seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sums = torch.zeros((N, 9, 3), dtype=torch.float32, device="cuda")
        parts, gen, red = [], 0, 0
        for rnd in range(ROUNDS):
            for p0 in range(0, N, CHUNK):
                k = min(CHUNK, N - p0)
                rays = _lib.probe_rays(probes, rnd, p0, k, out=torch.empty((k * D, 6), dtype=torch.float32, device="cuda"))
                res = _render_chunk(ds, r, rays, S, rnd, p0 * D)
                _lib.probe_project(rays, res.accum, S, D, sums=sums[p0:p0 + k])
                parts.append(res.stats)
                gen += k * D * 24                          # the generator's stores
                red += k * D * 40 + k * 216                # the projection's loads and its sums
        assert len(parts) == ROUNDS * 3 and N % CHUNK
        _, got = r.bake_probes(ds, probes, ROUNDS, chunk=CHUNK)
        plain = r.probe_stats
        assert np.array_equal(_u32(got), _u32(sums.cpu().numpy())), name
        assert_counters(plain, parts, gen, red, name)
        t = _timed(r)
        _, got_t = t.bake_probes(ds, probes, ROUNDS, chunk=CHUNK)
        assert np.array_equal(_u32(got_t), _u32(got)), name
        assert_counters(t.probe_stats, parts, gen, red, name + " timed")
        assert_times(plain, t.probe_stats, name)
    finally:
        ds.close()


@pytest.mark.parametrize("name,bvh", SCENES)
def test_bake_lightmap_stats_are_its_chunks(name, bvh):
    import torch
    D, S, ROUNDS, CHUNK = 4, 2, 2, 7
    scene, r = scenes.config(name, 8, 8, S)
    r = _with(r, use_bvh=bvh, seed=11)
    lm = R.flat_quad(8, 8, -1.5, -1.0, 1.5, 1.0, directions=D)           # one quad over the whole 8 x 8 map
    lm.placement(RenderObject.new(lm.mesh).rotate(Rotor3.from_rotation_xy(0.3) * Rotor3.from_rotation_yz(-0.2)).position(0.2, 2.5, 0.4))
    lm.seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        _, own, n_cov = _lib.lightmap_texels(lm, on_device=True)
        ids = torch.nonzero(own != -1).reshape(-1).to(torch.int32)
        assert ids.numel() == n_cov and n_cov > CHUNK and n_cov % CHUNK          # a boundary and a ragged last chunk
        sums = torch.zeros((8, 8, 4), dtype=torch.float32, device="cuda")
        parts, gen, red = [], 0, 0
        for rnd in range(ROUNDS):
            for q0 in range(0, n_cov, CHUNK):
                k = min(CHUNK, n_cov - q0)
                rays = _lib.lightmap_rays(lm, rnd, q0, k, out=torch.empty((k * D, 6), dtype=torch.float32, device="cuda"))
                res = _render_chunk(ds, r, rays, S, rnd, q0 * D)
                _lib.lightmap_reduce(res.accum, S, D, sums, texel_ids=ids[q0:q0 + k])
                parts.append(res.stats)
                gen += k * D * 24 + k * 36                 # the generator's stores, its records and ids
                red += k * D * 16 + k * 28                 # the reduction's loads and its sums
        _, got = r.bake_lightmap(ds, lm, ROUNDS, dilate=0, chunk=CHUNK)
        plain = r.lightmap_stats
        assert np.array_equal(_u32(got), _u32(sums.cpu().numpy())), name
        assert_counters(plain, parts, gen, red, name)
        t = _timed(r)
        _, got_t = t.bake_lightmap(ds, lm, ROUNDS, dilate=0, chunk=CHUNK)
        assert np.array_equal(_u32(got_t), _u32(got)), name
        assert_counters(t.lightmap_stats, parts, gen, red, name + " timed")
        assert_times(plain, t.lightmap_stats, name)
    finally:
        ds.close()


@pytest.mark.parametrize("name,bvh", SCENES)
def test_render_model_stats_are_its_chunks(name, bvh):
    import torch
    W, H, S, CHUNK = 8, 4, 3, 2
    scene, r = scenes.config(name, W, H, S)
    r = _with(r, use_bvh=bvh, seed=11)
    s = r.settings
    model = CameraModel.panorama(r._camera._cam_pos, W, H).seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        accum = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        parts, gen = [], 0
        for first in range(0, S, CHUNK):
            k = min(CHUNK, S - first)
            rays = _lib.model_rays(model, first, k, out=torch.empty((k, W * H, 6), dtype=torch.float32, device="cuda"))
            res = ds.render_rays(rays, k, first, accum, seed=s["seed"], use_bvh=s["use_bvh"], gamma=s["gamma"],
                                 paths_per_batch=s["paths_per_batch"], flags=s["flags"])
            parts.append(res.stats)
            gen += k * W * H * 24                          # the generator's stores
        assert len(parts) == 2 and S % CHUNK
        got = r.render_model(ds, model, S, chunk=CHUNK)
        assert np.array_equal(_u32(got.accum), _u32(accum.cpu().numpy())) and np.array_equal(got.rgb8, res.rgb8.cpu().numpy()), name
        assert_counters(got.stats, parts, gen, 0, name)
        timed = _timed(r).render_model(ds, model, S, chunk=CHUNK)
        assert np.array_equal(_u32(timed.accum), _u32(got.accum)), name
        assert_counters(timed.stats, parts, gen, 0, name + " timed")
        assert_times(got.stats, timed.stats, name)
    finally:
        ds.close()


@pytest.mark.parametrize("name,bvh", SCENES)
def test_render_views_stats_are_its_groups(name, bvh):
    """paths_per_batch of two and a half views' pixels at one sample: five views go in groups of 2, 2 and 1 (as test_gpu_views.py's
    test_small_batch_budgets_and_view_groups forces them), and a call of a group's own cameras is that one group"""
    W, H, S, PER = 8, 8, 2, 2
    scene, r = scenes.config(name, W, H, S)
    r = _with(r, use_bvh=bvh, seed=11).paths_per_batch(PER * W * H + W * H // 2)
    cams = orbit_cameras(r._camera, 5)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        groups = [ds.render_views(r, cams[v0:v0 + PER]) for v0 in range(0, len(cams), PER)]
        assert len(groups) == 3 and len(cams) % PER
        got = ds.render_views(r, cams)
        assert np.array_equal(_u32(got.linear_rgb), _u32(np.concatenate([g.linear_rgb for g in groups]))), name
        parts = [g.stats for g in groups]
        assert_counters(got.stats, parts, 0, 0, name)
        timed = ds.render_views(_timed(r), cams)
        assert np.array_equal(_u32(timed.linear_rgb), _u32(got.linear_rgb)), name
        assert_counters(timed.stats, parts, 0, 0, name + " timed")
        assert_times(got.stats, timed.stats, name)
    finally:
        ds.close()


def _trace_chunk(ds, r, rays, rnd, key_base, parts):
    s, st = r.settings, {}
    hits = ds.trace(rays, s["use_bvh"], seed=s["seed"] + rnd, key_base=key_base, stats=st)
    parts.append(st)
    return hits


@pytest.mark.parametrize("name,bvh", SCENES)
def test_bake_probe_depth_stats_are_its_chunks(name, bvh):
    import torch
    N, D, ROUNDS, CHUNK, RES = 5, 16, 2, 2, 4
    scene, r = scenes.config(name, 8, 8, 1)
    r = _with(r, use_bvh=bvh, seed=11)
    probes = ProbeSet(POSITIONS[name], D).seed(3)
    pd = ProbeDepth(RES, 6, 20.0)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sums = torch.zeros((N, RES, RES, 4), dtype=torch.float32, device="cuda")
        parts = []
        for rnd in range(ROUNDS):
            for p0 in range(0, N, CHUNK):
                k = min(CHUNK, N - p0)
                rays = _lib.probe_rays(probes, rnd, p0, k, out=torch.empty((k * D, 6), dtype=torch.float32, device="cuda"))
                hits = _trace_chunk(ds, r, rays, rnd, p0 * D, parts)
                _lib.probe_depth_reduce(pd, rays, hits, D, sums=sums[p0:p0 + k])
        assert len(parts) == ROUNDS * 3 and N % CHUNK
        _, got = r.bake_probe_depth(ds, probes, pd, ROUNDS, chunk=CHUNK)
        plain = r.probe_depth_stats
        assert np.array_equal(_u32(got), _u32(sums.cpu().numpy())) and np.any(got[..., 2] > 0), name
        assert_trace_counters(plain, parts, name)
        t = _timed(r)
        _, got_t = t.bake_probe_depth(ds, probes, pd, ROUNDS, chunk=CHUNK)
        assert np.array_equal(_u32(got_t), _u32(got)), name
        assert_trace_counters(t.probe_depth_stats, parts, name + " timed")
        assert_trace_times(plain, t.probe_depth_stats, name)
    finally:
        ds.close()


@pytest.mark.parametrize("name,bvh", SCENES)
def test_bake_ao_stats_are_its_chunks(name, bvh):
    import torch
    N, D, ROUNDS, CHUNK = 5, 16, 2, 2
    scene, r = scenes.config(name, 8, 8, 1)
    r = _with(r, use_bvh=bvh, seed=11)
    s = r.settings
    pos = np.array(POSITIONS[name], np.float32)
    nrm = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (N, 1))           # down, towards each scene's floor
    nrm[2] = 0.0                                                            # no rays are generated for it: its chunk traces fewer
    ok = api.ao_usable(pos, nrm)
    assert ok.tolist() == [True, True, False, True, True]
    ao = AmbientOcclusion(50.0, D, 1).seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        d_pos, d_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
        sums = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
        parts = []
        for rnd in range(ROUNDS):
            for q0 in range(0, N, CHUNK):
                k = min(CHUNK, N - q0)
                ids = torch.arange(q0, q0 + k, dtype=torch.int32, device="cuda")      # the points [q0, q0 + k) of the call
                rays = _lib.ao_rays(ao, d_pos, d_nrm, ids, rnd)
                hits = _trace_chunk(ds, r, rays, rnd, q0 * D, parts)
                _lib.ao_reduce(ao, rays, hits, sums, ids)
        assert len(parts) == ROUNDS * 3 and N % CHUNK
        assert parts[1]["rays"] == D and parts[0]["rays"] == 2 * D          # the zero rays of the point without a normal are not traced
        bake = dict(seed=s["seed"], use_bvh=s["use_bvh"], chunk=CHUNK)
        _, got, plain = ds.bake_ao(ao, pos, nrm, None, ROUNDS, flags=s["flags"], **bake)
        assert np.array_equal(_u32(got), _u32(sums.cpu().numpy())) and np.all(got[2] == 0.0) and np.any(got[ok] != 0.0), name
        assert_trace_counters(plain, parts, name)
        _, got_t, timed = ds.bake_ao(ao, pos, nrm, None, ROUNDS, flags=s["flags"] | A.FW_FLAG_TIME_KERNELS, **bake)
        assert np.array_equal(_u32(got_t), _u32(got)), name
        assert_trace_counters(timed, parts, name + " timed")
        assert_trace_times(plain, timed, name)
    finally:
        ds.close()


@pytest.mark.parametrize("name,bvh", SCENES)
def test_relocate_probes_stats_are_its_chunks(name, bvh):
    import torch
    N, D, STEPS, CHUNK = 5, 16, 2, 2
    scene, r = scenes.config(name, 8, 8, 1)
    r = _with(r, use_bvh=bvh, seed=11)
    probes = ProbeSet(POSITIONS[name], D).seed(3)
    rl = ProbeRelocation(3.0, 0.25, (4.0, 4.0, 4.0), steps=STEPS)          # every scene's floor is nearer than min_front to some probe
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        pl = api.neutral_placement(N)
        survey = torch.empty((N, 3, 4), dtype=torch.float32, device="cuda")
        parts, moved_any = [], False
        for i in range(STEPS + 1):                                           # the last pass classifies only
            at = probes.moved(pl)                                            # re-formed on the host from the placement, as the call does
            d_pl = torch.from_numpy(pl).cuda()
            for p0 in range(0, N, CHUNK):
                k = min(CHUNK, N - p0)
                rays = _lib.probe_rays(at, i, p0, k, out=torch.empty((k * D, 6), dtype=torch.float32, device="cuda"))
                hits = _trace_chunk(ds, r, rays, i, p0 * D, parts)
                _lib.probe_survey(rays, hits, D, out=survey[p0:p0 + k])
                _lib.probe_relocate_step(rl, survey[p0:p0 + k], d_pl[p0:p0 + k], D, move=i < STEPS)
            after = d_pl.cpu().numpy()
            stated = api.probe_relocate_step(rl, survey.cpu().numpy(), pl, D, move=i < STEPS)      # the numpy statement, on the CPU
            moved_any = moved_any or bool(np.any(stated[:, 0:3] != pl[:, 0:3]))
            pl = after
        assert len(parts) == (STEPS + 1) * 3 and N % CHUNK
        assert moved_any and np.any(pl[:, 0:3] != 0.0), name
        got_pl, got_sv = r.relocate_probes(ds, probes, rl, chunk=CHUNK)
        plain = r.probe_place_stats
        assert np.array_equal(_u32(got_pl), _u32(pl)) and np.array_equal(_u32(got_sv), _u32(survey.cpu().numpy())), name
        assert_trace_counters(plain, parts, name)
        t = _timed(r)
        got_t, _sv = t.relocate_probes(ds, probes, rl, chunk=CHUNK)
        assert np.array_equal(_u32(got_t), _u32(got_pl)), name
        assert_trace_counters(t.probe_place_stats, parts, name + " timed")
        assert_trace_times(plain, t.probe_place_stats, name)
    finally:
        ds.close()
