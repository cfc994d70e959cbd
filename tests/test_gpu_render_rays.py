"""Rendering along caller-supplied rays on the GPU (fw_render_rays), at zero tolerance.  The identity: fed the rays fw_camera_rays returns
and keyed by the pixel ids, fw_render_rays gives fw_render's frame bit for bit (u8, and the gamma and linear floats compared as uint32)
with the same ray counts — C1-C5, teapot and conics, the config's camera, a pinhole with a -0.0 coordinate and an aperture, both walks,
whole frames and pixel subsets, host arrays and device tensors on a side stream, kernel-selecting options.  Also: chunks of samples equal
one call and fw_render_progressive (accum included), fixed rays equal repeated per-sample rays, reversing rays and keys reverses the
outputs, rays straight into cornell's light give its emission, a pixel-centre panorama reproduces an HDR environment texel for texel,
invalid rays are refused without harm, and fw_render (and its frame graph) is untouched."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, HdrEnvironment, LambertianMat, RenderObject, Scene, Sphere, orthographic_rays,
                              panorama_rays)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [("C1_random_spheres", 40, 24, 6), ("C2_cornell_box", 32, 32, 8), ("C3_suzanne", 40, 24, 4), ("C4a_hdri_test", 32, 32, 4),
          ("C4b_volume_test", 32, 32, 4), ("C5_part2_all", 40, 24, 3), ("teapot", 40, 24, 4), ("conics", 40, 24, 4)]
# tests/test_gpu_trace.py's kernel-selecting options
WALK_OPTIONS = [dict(BVH="median"), dict(WIDE="0"), dict(WIDE="f32"), dict(WIDE="q8"), dict(EXACT_ALL="1"), dict(EXACT_FORM="lane"),
                dict(EXACT_FORM="wave"), dict(NO_DEFER="1"), dict(NO_HIT4="1"), dict(NO_LDS_TREES="1"), dict(NO_LDS_TRIS="1"),
                dict(WAVES="64"), dict(PATHS_PER_BATCH="5000")]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _with(r, cam=None, use_bvh=None, samples=None):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    if cam is not None:
        rr.camera(cam)
    if use_bvh is not None:
        rr.use_bvh(use_bvh)
    if samples is not None:
        rr.samples(samples)
    return rr


def cameras(r):
    """the config's camera; a pinhole with a -0.0 coordinate (24-byte camera rays in fw_render); an aperture"""
    base = r._camera
    p = np.asarray(base._cam_pos, np.float64)
    neg0 = copy.deepcopy(base).cam_pos((-0.0, p[1], p[2])).aperture(0.0)
    ap = copy.deepcopy(base).aperture(0.25)
    return [base, neg0, ap]


def camera_rays(ds, r, first, samples, ids=None):
    return np.stack([ds.camera_rays(r, first + s, ids) for s in range(samples)])


def rays_of(ds, r, rays, samples, first=0, accum=None, keys=None, **kw):
    s = r.settings
    return ds.render_rays(rays, samples, first, accum, keys, seed=s["seed"], use_bvh=s["use_bvh"], gamma=s["gamma"],
                          paths_per_batch=s["paths_per_batch"], **kw)


def assert_same(got, ref, what=""):
    assert np.array_equal(got.rgb8, ref.rgb8), what
    assert np.array_equal(_u32(got.gamma), _u32(ref.gamma)), what
    assert np.array_equal(_u32(got.linear), _u32(ref.linear)), what
    assert got.stats["rays"] == ref.stats["rays"], what
    assert [int(x) for x in got.stats["rays_per_depth"]] == [int(x) for x in ref.stats["rays_per_depth"]], what


def assert_identity(ds, r, ids=None, what=""):
    spp = r.settings["samples"]
    ref = ds.render(r, ids)
    got = rays_of(ds, r, camera_rays(ds, r, 0, spp, ids), spp, keys=ids)
    assert_same(got, ref, what)
    assert got.stats["reserved"] & 0x80000000 == 0
    return got


@pytest.mark.parametrize("name,w,h,spp", SCENES)
def test_identity_with_render(name, w, h, spp):
    scene, r = scenes.config(name, w, h, spp)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ids = np.ascontiguousarray(np.random.default_rng(5).permutation(w * h)[: w * h // 3].astype(np.uint32))
        for k, cam in enumerate(cameras(r)):
            for bvh in (False, True):
                rr = _with(r, cam=cam, use_bvh=bvh)
                assert_identity(ds, rr, None, f"{name} camera {k} bvh {bvh}")
                assert_identity(ds, rr, ids, f"{name} camera {k} bvh {bvh} subset")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["C2_cornell_box", "C3_suzanne", "C5_part2_all"])
def test_identity_under_walk_options(name):
    w, h, spp = {s[0]: s[1:] for s in SCENES}[name]
    scene, r = scenes.config(name, w, h, spp)
    for opt in WALK_OPTIONS:
        with _lib.options(**opt):
            ds = _lib.DeviceScene(scene.to_desc())        # BVH / WIDE apply to scenes created after them
            try:
                for bvh in (False, True):
                    assert_identity(ds, _with(r, use_bvh=bvh), None, f"{name} {opt} bvh {bvh}")
            finally:
                ds.close()


def test_device_tensors_on_a_side_stream():
    import torch
    dev = torch.device("cuda", 0)
    for name in ("C2_cornell_box", "C3_suzanne"):
        scene, r = scenes.config(name, 48, 32, 6)
        ds = _lib.DeviceScene(scene.to_desc())
        try:
            ids = np.ascontiguousarray(np.arange(48 * 32, dtype=np.uint32)[::-3])
            for bvh in (False, True):
                rr = _with(r, use_bvh=bvh)
                for sel in (None, ids):
                    ref = ds.render(rr, sel)
                    rays = torch.from_numpy(camera_rays(ds, rr, 0, 6, sel)).to(dev)
                    keys = None if sel is None else torch.from_numpy(sel.view(np.int32)).to(dev)
                    side = torch.cuda.Stream(device=dev)
                    side.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(side):
                        got = rays_of(ds, rr, rays, 6, keys=keys)
                    side.synchronize()
                    host = type(got)(got.rgb8.cpu().numpy(), got.gamma.cpu().numpy(), got.linear.cpu().numpy(), got.accum.cpu().numpy(), got.stats)
                    assert_same(host, ref, f"{name} bvh {bvh} subset {sel is not None}")
        finally:
            ds.close()


def test_progressive_identity():
    """(0, 3) + (3, 2) + (5, 4) samples equal one call of 9 and equal fw_render_progressive's chunks, accum included, host and device"""
    import torch
    scene, r = scenes.config("C4b_volume_test", 32, 32, 9)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        for bvh in (False, True):
            rr = _with(r, use_bvh=bvh)
            one = rays_of(ds, rr, camera_rays(ds, rr, 0, 9), 9)
            acc = np.zeros((32 * 32, 4), np.float32)
            pacc = np.zeros((32 * 32, 4), np.float32)
            dacc = torch.zeros((32 * 32, 4), dtype=torch.float32, device="cuda")
            for first, n in ((0, 3), (3, 2), (5, 4)):
                rays = camera_rays(ds, rr, first, n)
                got = rays_of(ds, rr, rays, n, first, acc)
                dev = rays_of(ds, rr, torch.from_numpy(rays).cuda(), n, first, dacc)
                ref = ds.render_progressive(_with(rr, samples=n), first, pacc)
                assert_same(got, ref, f"chunk {first} bvh {bvh}")
                assert np.array_equal(_u32(acc), _u32(pacc))
                assert np.array_equal(_u32(dev.accum.cpu().numpy()), _u32(pacc))
                assert np.array_equal(dev.rgb8.cpu().numpy(), ref.rgb8)
            assert np.array_equal(_u32(acc), _u32(one.accum))
            assert np.array_equal(one.rgb8, got.rgb8) and np.array_equal(_u32(one.linear), _u32(got.linear))
            assert_same(one, ds.render(rr), f"one call bvh {bvh}")
    finally:
        ds.close()


def test_fixed_rays_equal_repeated_rays():
    import torch
    scene, r = scenes.config("C2_cornell_box", 32, 32, 5)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        fixed = ds.camera_rays(r, 0)
        rep = np.ascontiguousarray(np.broadcast_to(fixed, (5,) + fixed.shape))
        for bvh in (False, True):
            rr = _with(r, use_bvh=bvh)
            a = rays_of(ds, rr, fixed, 5)
            b = rays_of(ds, rr, rep, 5)
            c = rays_of(ds, rr, torch.from_numpy(fixed).cuda(), 5)
            assert_same(a, b)
            assert np.array_equal(_u32(a.accum), _u32(b.accum))
            assert np.array_equal(c.rgb8.cpu().numpy(), a.rgb8) and np.array_equal(_u32(c.linear.cpu().numpy()), _u32(a.linear))
            # ... and with many samples per batch and few rays: the fixed rays' entries found from the sample quotient
            few = np.ascontiguousarray(fixed[:3])
            d = rays_of(ds, rr, few, 3000)
            e = rays_of(ds, rr, np.ascontiguousarray(np.broadcast_to(few, (3000, 3, 6))), 3000)
            assert_same(d, e)
    finally:
        ds.close()


def test_reversed_rays_and_keys_reverse_the_outputs():
    scene, r = scenes.config("C3_suzanne", 40, 24, 4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ids = np.arange(40 * 24, dtype=np.uint32)
        rays = camera_rays(ds, r, 0, 4)
        fwd = rays_of(ds, r, rays, 4)
        rev = rays_of(ds, r, np.ascontiguousarray(rays[:, ::-1]), 4, keys=np.ascontiguousarray(ids[::-1]))
        assert np.array_equal(rev.rgb8, fwd.rgb8[::-1])
        assert np.array_equal(_u32(rev.gamma), _u32(fwd.gamma[::-1]))
        assert np.array_equal(_u32(rev.linear), _u32(fwd.linear[::-1]))
        assert np.array_equal(_u32(rev.accum), _u32(fwd.accum[::-1]))
        # duplicate keys: allowed, correlated draws — entries with one key and one ray are equal
        dup = rays_of(ds, r, np.ascontiguousarray(np.repeat(rays[:, :1], 5, axis=1)), 4, keys=np.full(5, 7, np.uint32))
        assert all(np.array_equal(_u32(dup.accum[k]), _u32(dup.accum[0])) for k in range(5))
        keyed = rays_of(ds, r, rays, 4, key_base=0)
        assert np.array_equal(_u32(keyed.accum), _u32(fwd.accum))
        shifted = rays_of(ds, r, camera_rays(ds, r, 0, 4, np.arange(100, 140, dtype=np.uint32)), 4, key_base=100)
        ref = ds.render(r, np.arange(100, 140, dtype=np.uint32))
        assert_same(shifted, ref)
    finally:
        ds.close()


def test_rays_into_the_light_give_its_emission():
    """cornell: rays from inside the box straight up into the light (an Emissive scatters nothing) give exactly its emission"""
    scene, r = scenes.cornell_box()
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        xs, zs = np.meshgrid(np.linspace(220.0, 335.0, 8), np.linspace(235.0, 325.0, 4))
        rays = np.zeros((32, 6), np.float32)
        rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 4] = xs.ravel(), 400.0, zs.ravel(), 1.0      # above both boxes
        for bvh in (False, True):
            for spp in (1, 7, 64):
                got = ds.render_rays(rays, spp, use_bvh=bvh)
                assert np.all(got.linear == np.float32(15.0)), (bvh, spp)
                assert np.all(got.rgb8 == 255) and np.all(got.gamma == np.float32(1.0))
                assert np.all(got.accum[:, :3] == np.float32(15.0 * spp))
                assert got.stats["rays"] == 32 * spp and got.stats["rays_per_depth"][1] == 0
    finally:
        ds.close()


def test_panorama_round_trip():
    """A pixel-centre panorama of an HDR environment of distinct texels, at the map's own size and 1 spp, reproduces every texel whose
    ray misses the one small sphere (an empty scene is an error)"""
    W, H = 128, 64
    j, x = np.mgrid[0:H, 0:W]
    hdr = np.stack([(x + 1) / W, (j + 1) / H, (x + W * j + 1) / (W * H) + 0.5], axis=2).astype(np.float32)
    scene = Scene.new()
    m = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, m)).position(0.0, 0.0, 3.0))
    scene.set_environment(HdrEnvironment(hdr))
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = panorama_rays((0.0, 0.0, 0.0), W, H, 0, jitter=False)
        for bvh in (False, True):
            hits = ds.trace(rays, bvh)
            miss = hits["object"] == A.FW_NO_HIT
            assert 0.9 * W * H < miss.sum() < W * H                        # the sphere is seen, and most of the map
            got = ds.render_rays(rays[None], 1, use_bvh=bvh)
            # no pixel is excluded: every centre direction lies half a texel from the boundaries, far beyond float rounding
            assert np.array_equal(_u32(got.linear[miss]), _u32(hdr.reshape(-1, 3)[miss])), bvh
    finally:
        ds.close()


@pytest.mark.parametrize("bad", ["nan", "zero"])
def test_invalid_rays_are_refused(bad):
    import torch
    scene, r = scenes.config("C2_cornell_box", 32, 32, 3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        for bvh in (False, True):
            rr = _with(r, use_bvh=bvh)
            rays = camera_rays(ds, rr, 0, 3)
            broken = rays.copy()
            if bad == "nan":
                broken[1, 17, 4] = np.nan
            else:
                broken[2, 500, 3:] = 0.0
            with pytest.raises(_lib.FireworkError) as e:
                rays_of(ds, rr, broken, 3)
            assert e.value.status == A.FW_ERR_BAD_ARG
            with pytest.raises(_lib.FireworkError) as e:
                rays_of(ds, rr, torch.from_numpy(broken).cuda(), 3)
            assert e.value.status == A.FW_ERR_BAD_ARG
            with pytest.raises(_lib.FireworkError) as e:
                rays_of(ds, rr, np.ascontiguousarray(broken[1 if bad == "nan" else 2]), 3)       # fixed rays
            assert e.value.status == A.FW_ERR_BAD_ARG
            torch.cuda.synchronize()
            assert_identity(ds, rr, None, f"after a refused call, bvh {bvh}")
    finally:
        ds.close()


@pytest.mark.parametrize("graph", [None, "1"])
def test_render_untouched(graph):
    """fw_render before and after render_rays calls is bit-identical; under GRAPH its repeated frame is still replayed (bit 31)"""
    scene, r = scenes.config("C1_random_spheres", 48, 32, 4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = camera_rays(ds, r, 0, 4)
        with _lib.options(GRAPH=graph):
            before = [ds.render(r) for _ in range(3)]
            mid = [rays_of(ds, r, rays, 4) for _ in range(2)]
            after = [ds.render(r) for _ in range(2)]
        for a in before[1:] + after:
            assert np.array_equal(a.rgb8, before[0].rgb8)
            assert np.array_equal(_u32(a.linear), _u32(before[0].linear))
        for m in mid:
            assert_same(m, before[0])
            assert m.stats["reserved"] & 0x80000000 == 0
        if graph:
            assert before[2].stats["reserved"] & 0x80000000 and after[1].stats["reserved"] & 0x80000000
    finally:
        ds.close()


def test_camera_models_chunk_invariance():
    """render_camera_model gives the same bits for any chunk size; orthographic and panorama models through it"""
    import functools
    scene, r = scenes.config("conics", 32, 16, 4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        pano = functools.partial(panorama_rays, r._camera._cam_pos, 32, 16, seed=3)
        ortho = functools.partial(orthographic_rays, r._camera, 6.0, 32, 16, seed=3, device=0)
        for model in (pano, ortho):
            res = [r.render_camera_model(ds, model, 7, chunk=c) for c in (1, 3, 64)]
            for x in res[1:]:
                a = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else t      # noqa: E731
                assert np.array_equal(a(x.rgb8), a(res[0].rgb8)) and np.array_equal(_u32(a(x.linear)), _u32(a(res[0].linear)))
                assert np.array_equal(_u32(a(x.accum)), _u32(a(res[0].accum)))
    finally:
        ds.close()


def test_cli_panorama_and_pinhole(tmp_path):
    """--camera panorama writes a --width x --height image; the default --camera pinhole writes what the fixed camera renders"""
    from PIL import Image
    from firework_amd import yaml_io
    from firework_amd.api import Renderer
    path = tmp_path / "s.yml"
    scene, _r = scenes.config("conics", 8, 8, 1)
    yaml_io.save_scene(scene, str(path))
    pano, pin = tmp_path / "pano.png", tmp_path / "pin.png"
    base = [sys.executable, "-m", "firework_amd", "--scene-file", str(path), "-s", "2"]
    for extra in (["--camera", "panorama", "--width", "128", "--height", "64", "-o", str(pano)],
                  ["--width", "64", "--height", "40", "-o", str(pin)]):
        p = subprocess.run(base + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stderr
    assert Image.open(pano).size == (128, 64)
    cam = CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    ref = Renderer.default().width(64).height(40).samples(2).use_bvh(True).camera(cam).seed(0).render(yaml_io.load_scene(str(path)))
    assert np.array_equal(np.asarray(Image.open(pin)), ref.reshape(40, 64, 3))
