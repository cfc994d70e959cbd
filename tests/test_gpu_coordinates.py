"""Ray queries and renders far from the origin and at extreme scales (tests/coord_scenes.py) against the CPU oracle, with zero
tolerance.  The walks cull with boxes grown relative to the items' sizes and compute a plane's distance as one fma whose rounding
grows with the ray origin's coordinate (fw_kernels.hip: wide_step); these scenes move |origin| / item size up to 2^20 and rescale the
baseline scenes by 2^-10 ... 2^12, under every walk (WIDE f32 / q8 / 0, the median tree, device-built trees, the exact walk)."""
import time

import numpy as np
import pytest

import coord_scenes as C
from firework_amd import _abi as A
from firework_amd import _lib
from test_gpu_device_build import _assert_same
from test_gpu_parity import check
from test_gpu_trace import adversarial_set, compare, secondary_set

pytestmark = pytest.mark.gpu

FAMILY = C.family()
IDS = [f[0] for f in FAMILY]
OPTIONS = [{}, dict(WIDE="f32"), dict(WIDE="q8"), dict(WIDE="0"), dict(BVH="median"), dict(EXACT_ALL="1")]


@pytest.fixture(scope="module")
def ray_sets(oracle):
    """Per scene: (scene, renderer, {mode: [(label, rays, oracle records)]}), made once with the default options."""
    cache = {}

    def get(sid):
        if sid not in cache:
            fn, modes = next((f[1], f[2]) for f in FAMILY if f[0] == sid)
            scene, renderer = fn()
            sd = scene.to_desc()
            ds = _lib.DeviceScene(sd)
            try:
                ids = np.unique(np.linspace(0, renderer.settings["width"] * renderer.settings["height"] - 1, 768).astype(np.uint32))
                cam = np.concatenate([ds.camera_rays(renderer, s, ids) for s in (0, 7)])
                sec = secondary_set(oracle, sd, renderer, n_paths=48)
                graze, _ = C.grazing_set(scene, renderer, oracle)
                graze = np.concatenate([graze, C.far_origin_set(scene)])
                sets = {}
                for m in modes:
                    adv = adversarial_set(oracle, scene, ds, m, cam, n=384)
                    sets[m] = [(label, r, oracle.trace(sd, r, m)) for label, r in
                               (("camera", cam), ("secondary", sec), ("adversarial", adv), ("grazing", graze))]
            finally:
                ds.close()
            cache[sid] = (scene, renderer, sets)
        return cache[sid]
    return get


@pytest.mark.parametrize("sid", IDS)
def test_trace_parity_far_and_rescaled(ray_sets, sid):
    scene, renderer, sets = ray_sets(sid)
    opts = OPTIONS + ([dict(BUILD="device")] if sid.startswith("a_") else [])
    t0 = time.time()
    for opt in opts:
        with _lib.options(**opt):
            ds = _lib.DeviceScene(scene.to_desc())        # the walk options apply to scenes created after them
            try:
                for m, rows in sets.items():
                    for label, rays, ref in rows:
                        compare(ds.trace(rays, m), ref, f"{sid} {opt} use_bvh={m} {label}")
            finally:
                ds.close()
    print(f"{sid}: {sum(r[1].shape[0] for rows in sets.values() for r in rows)} rays x {len(opts)} options, {time.time() - t0:.2f} s")


RENDERS = [pytest.param(f[0], m, id=f"{f[0]}-bvh{m}") for f in FAMILY for m in f[2]]


@pytest.mark.parametrize("sid,m", RENDERS)
def test_render_parity_far_and_rescaled(oracle, sid, m):
    fn = next(f[1] for f in FAMILY if f[0] == sid)
    scene, renderer = fn()
    check(oracle, scene, renderer.use_bvh(bool(m)))


@pytest.mark.parametrize("case", [c[0] for c in C.MESH_CASES])
def test_device_build_of_far_meshes(case):
    """the device builder's fmin / fmax and (int) conversions of centre keys on the triangle boxes of the far meshes, as given and
    as the host pads them (0.001 on thin axes)"""
    scene, _ = C.far_mesh(case)
    s = scene.render_objects[0].obj
    tri = s.verts[s.indicies.reshape(-1, 3)]
    b = np.concatenate([tri.min(axis=1), tri.max(axis=1)], axis=1).astype(np.float32)
    _assert_same(b, f"{case} triangle boxes")
    thin = (b[:, 3:] - b[:, :3]) < np.float32(0.001)
    pad = b.copy()
    pad[:, :3] = np.where(thin, b[:, :3] - np.float32(0.001), b[:, :3])
    pad[:, 3:] = np.where(thin, b[:, 3:] + np.float32(0.001), b[:, 3:])
    _assert_same(pad, f"{case} padded boxes")


def _compare_inplane(gpu, ora, what):
    """compare() for rays whose oracle t may be 0/0: the hit flag, and for hits the material, the normal and t, NaN-aware, bit for bit"""
    hit, ohit = gpu["object"] != A.FW_NO_HIT, ora[:, 0] == 1
    bad = np.nonzero(hit != ohit)[0]
    assert bad.size == 0, f"{what}: hit flag differs for {bad.size} rays, first {bad[:5]}"
    g, o = gpu[hit], ora[hit]
    same = lambda a, b: (np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same(g["t"], o[:, 1]).all(), f"{what}: t differs for {int((~same(g['t'], o[:, 1])).sum())} hits"
    assert same(g["normal"], o[:, 5:8]).all(axis=1).all(), f"{what}: normal differs"
    assert (g["material"] == o[:, 8].astype(np.uint32)).all(), what
    return int(np.isnan(o[:, 1]).sum())


@pytest.mark.parametrize("sid", ["d_C2_2^12", "d_C2_2^-10", "d_R2_2^12"])
def test_rays_inside_a_rect_plane_follow_the_reference(oracle, sid):
    """A ray that starts on a rect and runs inside its plane meets it at t = 0/0; the reference keeps that NaN hit or lets a later test
    replace it, by the order of its tests.  At 2^12 such rays are common among scattered rays (their directions are quantised); they take
    the exact walk (fw_kernels.hip: needs_exact), and the records equal the oracle's, NaN t included, under every walk."""
    scene, renderer = next(f[1] for f in FAMILY if f[0] == sid)()
    rays = C.inplane_set(scene)
    assert rays.shape[0] > 0
    sd = scene.to_desc()
    for m in (1,):         # (the linear scan's record of such a ray still differs: compare() leaves them out; renders under use_bvh = 0 agree)
        ref = oracle.trace(sd, rays, m)
        for opt in ({}, dict(WIDE="q8"), dict(WIDE="0"), dict(BVH="median")):
            with _lib.options(**opt):
                ds = _lib.DeviceScene(sd)
                try:
                    n_nan = _compare_inplane(ds.trace(rays, m), ref, f"{sid} {opt} use_bvh={m}")
                finally:
                    ds.close()
        print(f"{sid} use_bvh={m}: {rays.shape[0]} rays, {n_nan} NaN-t hits")
