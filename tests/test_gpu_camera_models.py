"""Camera models generated on the GPU (fw_model_rays, fw_render_model, fw_render_model_aovs).  k_model_rays against the numpy float64
statements (api.panorama_rays, orthographic_rays, fisheye_rays) to one float32 ulp at each vector's scale, with panorama origins and
orthographic directions bit-equal; fw_render_model against its composition fw_render_rays(fw_model_rays) bit for bit for every chunk
size, through accum, on a side stream and under light sampling; the panorama round trip through an HDR map; fw_render_model_aovs against
its composition from fw_model_rays and fw_trace_rays bit for bit; denoising at L = 0; fw_render left untouched; the CLI's fisheye."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import CameraModel, CameraSettings, HdrEnvironment, LambertianMat, RenderObject, Scene, Sphere

import denoise_ref as R
from test_camera_models_cpu import build_cpp_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = CameraSettings.default().cam_pos((3.0, 30.0, 50.0)).look_at((0.5, -1.0, 2.0))      # origins far from 0
SIZES = [(1, 1), (7, 3), (64, 1), (65, 3), (300, 7)]       # one pixel; odd; exactly one wave; a wave's tail; several blocks and a tail
SAMPLES = [0, 5, (1 << 31) + 3]
SEEDS = [0, 7, 0x1234567800000009]                         # the last one exercises the 64-bit seed fold


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def models(w, h):
    return dict(panorama=CameraModel.panorama(CAM._cam_pos, w, h), orthographic=CameraModel.orthographic(CAM, 7.5, w, h),
                fisheye=CameraModel.fisheye(CAM, 200.0, w, h))


def assert_rays_close(kind, got, ref, what):
    """per component |gpu - ref| <= 2^-23 x the largest magnitude among that vector's three reference components: both sides round the
    same float64 expression, whose libm results differ by a few float64 ulps, so the float32 values are equal or adjacent — one float32
    ulp at the vector's scale.  Every ray is compared, and every component must be finite (the device buffers are NaN before the call)."""
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.all(np.isfinite(got)), what
    g, r = got.astype(np.float64).reshape(-1, 2, 3), ref.astype(np.float64).reshape(-1, 2, 3)
    bound = 2.0 ** -23 * np.abs(r).max(axis=2, keepdims=True)
    err = np.abs(g - r)
    assert np.all(err <= bound), (what, float((err / bound).max()), np.argwhere(err > bound)[:4])
    if kind == "panorama":
        assert np.array_equal(_u32(got[..., :3]), _u32(ref[..., :3])), what
    if kind == "orthographic":
        assert np.array_equal(_u32(got[..., 3:]), _u32(ref[..., 3:])), what


@pytest.mark.parametrize("kind", ["panorama", "orthographic", "fisheye"])
@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_matches_the_numpy_statement(kind, w, h):
    import torch
    dev = torch.device("cuda", 0)
    for sample in SAMPLES:
        for seed in SEEDS:
            for jitter in (True, False):
                m = models(w, h)[kind].seed(seed).jitter(jitter)
                ref = np.stack([m.rays(sample + k) for k in range(3)])
                what = f"{kind} {w}x{h} sample {sample} seed {seed:#x} jitter {jitter}"
                for n in (1, 3):
                    assert_rays_close(kind, _lib.model_rays(m, sample, n), ref[:n], what + f" host n {n}")
                    out = torch.full((n, w * h, 6), float("nan"), dtype=torch.float32, device=dev)
                    assert_rays_close(kind, _lib.model_rays(m, sample, n, out=out).cpu().numpy(), ref[:n], what + f" device n {n}")
    # a wrong jitter would show far above the bound: samples and seeds give different rays
    m = models(w, h)[kind].seed(7)
    if w * h > 1:
        assert not np.array_equal(_lib.model_rays(m, 0, 1), _lib.model_rays(m, 1, 1))
        assert not np.array_equal(_lib.model_rays(m, 0, 1), _lib.model_rays(models(w, h)[kind].seed(8), 0, 1))


def test_last_sample_range():
    """[2^32 - 2, 2^32) is the last valid range"""
    m = models(7, 3)["fisheye"].seed(7)
    got = _lib.model_rays(m, 0xFFFFFFFE, 2)
    assert_rays_close("fisheye", got, np.stack([m.rays(0xFFFFFFFE), m.rays(0xFFFFFFFF)]), "last samples")
    with pytest.raises(_lib.FireworkError) as e:
        _lib.model_rays(m, 0xFFFFFFFE, 3)
    assert e.value.status == A.FW_ERR_BAD_ARG


def _with(r, **settings):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    rr.settings.update(settings)
    return rr


def composed(ds, r, model, samples, first=0, accum=None):
    """fw_render_rays over fw_model_rays' device rays"""
    import torch
    s = r.settings
    rays = torch.empty((samples, model.width * model.height, 6), dtype=torch.float32, device="cuda")
    _lib.model_rays(model, first, samples, out=rays)
    return ds.render_rays(rays, samples, first, accum, seed=s["seed"], use_bvh=s["use_bvh"], gamma=s["gamma"],
                          paths_per_batch=s["paths_per_batch"], flags=s["flags"])


def assert_same(got, ref, what=""):
    assert np.array_equal(_host(got.rgb8), _host(ref.rgb8)), what
    assert np.array_equal(_u32(_host(got.gamma)), _u32(_host(ref.gamma))), what
    assert np.array_equal(_u32(_host(got.linear)), _u32(_host(ref.linear))), what
    assert np.array_equal(_u32(_host(got.accum)), _u32(_host(ref.accum))), what
    assert got.stats["rays"] == ref.stats["rays"], what
    assert [int(x) for x in got.stats["rays_per_depth"]] == [int(x) for x in ref.stats["rays_per_depth"]], what


def scene_models(r, w, h, seed=3):
    cam = r._camera
    return dict(panorama=CameraModel.panorama(cam._cam_pos, w, h).seed(seed), orthographic=CameraModel.orthographic(cam, 6.0, w, h).seed(seed),
                fisheye=CameraModel.fisheye(cam, 150.0, w, h).seed(seed))


@pytest.mark.parametrize("kind", ["panorama", "orthographic", "fisheye"])
def test_render_model_equals_its_composition(kind):
    import torch
    W, H, S = 32, 16, 7
    scene, r = scenes.config("conics", W, H, S)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        for bvh in (False, True):
            rr = _with(r, use_bvh=bvh, seed=11)
            model = scene_models(rr, W, H)[kind]
            ref = composed(ds, rr, model, S)
            assert ref.stats["rays"] >= W * H * S
            for chunk in (1, 3, 0):
                assert_same(rr.render_model(ds, model, S, chunk=chunk), ref, f"{kind} bvh {bvh} chunk {chunk}")
            # 3 + 4 samples through accum equal one call of 7 (host arrays, and the composition's own two calls)
            acc = np.zeros((W * H, 4), np.float32)
            a = rr.render_model(ds, model, 3, 0, acc, chunk=2)
            ca = composed(ds, rr, model, 3)
            assert_same(a, ca, f"{kind} first 3")
            b = rr.render_model(ds, model, 4, 3, acc, chunk=3)
            assert b.accum is acc
            cb = composed(ds, rr, model, 4, 3, ca.accum)
            assert_same(b, cb, f"{kind} then 4")
            assert a.stats["rays"] + b.stats["rays"] == ref.stats["rays"]
            for x in (b, cb):
                assert np.array_equal(_host(x.rgb8), _host(ref.rgb8)) and np.array_equal(_u32(_host(x.linear)), _u32(_host(ref.linear)))
                assert np.array_equal(_u32(_host(x.accum)), _u32(_host(ref.accum)))
            # device outputs on a side stream
            dev = torch.device("cuda", 0)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                d1 = rr.render_model(ds, model, 3, chunk=2, on_device=True)
                d2 = rr.render_model(ds, model, 4, 3, d1.accum, chunk=1)
            side.synchronize()
            assert d2.rgb8.is_cuda and d2.accum is d1.accum
            assert_same(d2, cb, f"{kind} bvh {bvh} device")
            # the generator's time is reported, and timing changes no bit
            t = _with(rr, flags=rr.settings["flags"] | A.FW_FLAG_TIME_KERNELS).render_model(ds, model, S, chunk=3)
            assert_same(t, ref, f"{kind} timed")
            assert t.stats["ms_raygen"] > 0 and t.stats["ms_render"] >= t.stats["ms_raygen"] and t.stats["n_batches"] >= 3
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["C2_cornell_box", "conics"])
def test_render_model_under_light_sampling(name):
    W, H, S = 32, 16, 7
    scene, r = scenes.config(name, W, H, S)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rr = _with(r, seed=5).light_sampling()
        plain = _with(r, seed=5)
        for kind, model in scene_models(rr, W, H).items():
            ref = composed(ds, rr, model, S)
            for chunk in (1, 3, 0):
                assert_same(rr.render_model(ds, model, S, chunk=chunk), ref, f"{name} {kind} chunk {chunk}")
            if name == "C2_cornell_box":       # the flag is in force: cornell's light is sampled
                assert not np.array_equal(_u32(_host(ref.accum)), _u32(plain.render_model(ds, model, S).accum)), kind
    finally:
        ds.close()


def test_panorama_round_trip_through_render_model():
    """tests/test_gpu_render_rays.py's test_panorama_round_trip with the rays made on the device: a pixel-centre panorama of an HDR
    environment of distinct texels, at the map's own size and 1 spp, reproduces every texel whose ray misses the one small sphere.  No
    pixel is excluded: every centre direction lies half a texel from the boundaries, so one ulp cannot move a lookup."""
    W, H = 128, 64
    j, x = np.mgrid[0:H, 0:W]
    hdr = np.stack([(x + 1) / W, (j + 1) / H, (x + W * j + 1) / (W * H) + 0.5], axis=2).astype(np.float32)
    scene = Scene.new()
    m = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, m)).position(0.0, 0.0, 3.0))
    scene.set_environment(HdrEnvironment(hdr))
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        model = CameraModel.panorama((0.0, 0.0, 0.0), W, H).jitter(False)
        rays = _lib.model_rays(model, 0, 1)[0]
        for bvh in (False, True):
            miss = ds.trace(rays, bvh)["object"] == A.FW_NO_HIT
            assert 0.9 * W * H < miss.sum() < W * H
            got = ds.render_model(model, 1, use_bvh=bvh)
            assert np.array_equal(_u32(got.linear[miss]), _u32(hdr.reshape(-1, 3)[miss])), bvh
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["C2_cornell_box", "conics"])
@pytest.mark.parametrize("kind", ["panorama", "fisheye"])
def test_model_aovs_equal_their_composition(oracle, name, kind):
    """fw_render_model_aovs = denoise_ref.aovs_from_hits over fw_model_rays (sample s) and fw_trace_rays (key_base 0), bit for bit:
    denoise_ref.aovs_composed with the model's rays.  (Scenes without a medium: the media keys of a trace agree for every sample.)"""
    import torch
    W, H, S = 33, 17, 4
    scene, r = scenes.config(name, W, H, 1)
    r.seed(7)
    sd = scene.to_desc()
    ds = _lib.DeviceScene(sd, 0)
    try:
        model = scene_models(r, W, H, seed=9)[kind]
        for bvh in (False, True):
            got = ds.model_aovs(model, S, seed=7, use_bvh=bvh)
            st = ds.aovs_stats
            per = []
            for s in range(S):
                rays = _lib.model_rays(model, s, 1)[0]
                per.append((rays, ds.trace(rays, bvh, seed=7)))
            want = R.aovs_from_hits(sd, per, oracle)
            assert got.shape == (W * H, 12)
            bad = np.nonzero(np.any(_u32(got) != _u32(want), axis=1))[0]
            assert bad.size == 0, (name, kind, bvh, bad[:8], got[bad[:2]], want[bad[:2]])
            assert st["rays"] > 0 and st["n_batches"] >= S
            assert float(got[:, 3].max()) > 0                         # something was hit
            out = torch.full((W * H, 12), float("nan"), dtype=torch.float32, device="cuda")
            assert np.array_equal(_u32(ds.model_aovs(model, S, seed=7, use_bvh=bvh, out=out).cpu().numpy()), _u32(got))
    finally:
        ds.close()


@pytest.mark.parametrize("kind", ["panorama", "orthographic", "fisheye"])
def test_zero_iterations_is_the_raw_frame(kind):
    W, H = 48, 32
    scene, r = scenes.config("C2_cornell_box", W, H, 4)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        model = scene_models(r, W, H)[kind]
        ref = r.render_model(ds, model, 4)
        res = r.render_model_denoised(ds, model, 4, iterations=0, aov_samples=2)
        for x in (res, res.raw):
            assert np.array_equal(x.rgb8, ref.rgb8)
            assert np.array_equal(_u32(x.gamma), _u32(ref.gamma)) and np.array_equal(_u32(x.linear), _u32(ref.linear))
        assert (res.width, res.height) == (W, H) and res.image().shape == (H, W, 3)
        filtered = r.render_model_denoised(ds, model, 4, iterations=3, aov_samples=2)
        assert np.all(np.isfinite(filtered.linear)) and not np.array_equal(_u32(filtered.linear), _u32(ref.linear))
        aov = r.model_aovs(ds, model, 2)
        assert aov["albedo"].shape == (H, W, 3) and aov["coverage"].shape == (H, W)
    finally:
        ds.close()


@pytest.mark.parametrize("graph", [None, "1"])
def test_render_untouched(graph):
    """fw_render before and after the new calls is bit-identical; under GRAPH its repeated frame is still replayed (bit 31)"""
    scene, r = scenes.config("C1_random_spheres", 48, 32, 4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ms = scene_models(r, 48, 32)
        with _lib.options(GRAPH=graph):
            before = [ds.render(r) for _ in range(3)]
            mid = [r.render_model(ds, m, 4, chunk=c) for m in ms.values() for c in (1, 0)]
            _lib.model_rays(ms["fisheye"], 0, 2)
            ds.model_aovs(ms["panorama"], 2)
            after = [ds.render(r) for _ in range(2)]
        for a in before[1:] + after:
            assert np.array_equal(a.rgb8, before[0].rgb8)
            assert np.array_equal(_u32(a.linear), _u32(before[0].linear))
            assert a.stats["rays"] == before[0].stats["rays"]
        for m in mid:
            assert m.stats["reserved"] & 0x80000000 == 0
        if graph:
            assert before[2].stats["reserved"] & 0x80000000 and after[1].stats["reserved"] & 0x80000000
    finally:
        ds.close()


def test_cli_fisheye(tmp_path):
    """--camera fisheye writes a --width x --height image"""
    from PIL import Image
    from firework_amd import yaml_io
    path = tmp_path / "s.yml"
    scene, _r = scenes.config("conics", 8, 8, 1)
    yaml_io.save_scene(scene, str(path))
    out = tmp_path / "fish.png"
    p = subprocess.run([sys.executable, "-m", "firework_amd", "--scene-file", str(path), "-s", "2", "--camera", "fisheye", "--fisheye-fov", "170",
                        "--width", "96", "--height", "40", "-o", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr
    img = Image.open(out)
    assert img.size == (96, 40) and np.asarray(img).std() > 0


def test_cpp_host_equals_the_python_path(tmp_path):
    """include/firework.hpp's Renderer::render_model gives the images of Renderer.render_model for the same scene and models"""
    from firework_amd.api import EmissiveMat, Renderer, XYRect, XZRect, YZRect
    out = subprocess.run([str(build_cpp_host(tmp_path))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    w = Scene.new()
    red = w.add_material(LambertianMat.with_color((0.65, 0.05, 0.05)))
    white = w.add_material(LambertianMat.with_color((0.73, 0.73, 0.73)))
    green = w.add_material(LambertianMat.with_color((0.12, 0.45, 0.15)))
    light = w.add_material(EmissiveMat.with_color((15.0, 15.0, 15.0)))
    w.add_object(RenderObject.new(XZRect.new(213.0, 343.0, 227.0, 332.0, 554.0, light)))
    w.add_object(RenderObject.new(YZRect.new(0.0, 555.0, 0.0, 555.0, 555.0, green)).flip_normals())
    w.add_object(RenderObject.new(YZRect.new(0.0, 555.0, 0.0, 555.0, 0.0, red)))
    w.add_object(RenderObject.new(XZRect.new(0.0, 555.0, 0.0, 555.0, 0.0, white)))
    w.add_object(RenderObject.new(XZRect.new(0.0, 555.0, 0.0, 555.0, 555.0, white)).flip_normals())
    w.add_object(RenderObject.new(XYRect.new(0.0, 555.0, 0.0, 555.0, 555.0, white)).flip_normals())
    cam = CameraSettings.default().cam_pos((278.0, 278.0, -800.0)).look_at((278.0, 270.0, 0.0))
    r = Renderer.default().samples(4).use_bvh(True).seed(5)
    ms = [CameraModel.panorama((278.0, 278.0, 278.0), 24, 10).seed(3), CameraModel.orthographic(cam, 500.0, 24, 10).seed(3),
          CameraModel.fisheye(cam, 150.0, 24, 10).seed(3).jitter(False)]
    ds = _lib.DeviceScene(w.to_desc())
    try:
        want = []
        for m in ms:
            h = 1469598103934665603
            for b in r.render_model(ds, m, 4).rgb8.reshape(-1).tolist():
                h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
            want.append(f"model {m.kind}: 240 pixels {h:016x}")
    finally:
        ds.close()
    assert out.stdout.splitlines()[1:] == want
    assert len(set(want)) == 3
