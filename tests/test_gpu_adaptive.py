"""Adaptive sampling on the GPU (fw_render_adaptive), at zero tolerance everywhere:
- replay: every pixel's per-sample colours (fw_render_progressive, one sample at a time) summed, squared and judged round by round in
  numpy float32 give the device's moments, final counts and round sizes bit for bit;
- every group of pixels that stopped at n samples equals fw_render / fw_render_progressive at n samples (and the CPU oracle for C2, C3);
- extremes, option invariance, isolation from plain renders, device outputs, the CLI and the C++ host."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("adaptive_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_adaptive_cpu.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

MIN, CAP = 4, 64
SCENES = [("C1_random_spheres", 96, 64), ("C2_cornell_box", 64, 64), ("C3_suzanne", 96, 64), ("C4a_hdri_test", 64, 64),
          ("C4b_volume_test", 64, 64), ("teapot", 96, 64), ("conics", 96, 64), ("C5_part2_all", 96, 64)]
TOLERANCES = (0.5, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.002)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _renderer(renderer, samples):
    import copy
    r = copy.copy(renderer)
    r.settings = dict(renderer.settings)
    r.settings["samples"] = int(samples)
    return r


def per_sample_colours(ds, renderer, cap):
    """(P, cap, 3) float32: sample s of every pixel, from fw_render_progressive(first_sample = s, samples = 1) into zeroed sums"""
    r1 = _renderer(renderer, 1)
    n = renderer.settings["width"] * renderer.settings["height"]
    out = np.empty((n, cap, 3), np.float32)
    for s in range(cap):
        acc = np.zeros((n, 4), np.float32)
        ds.render_progressive(r1, s, acc)
        out[:, s] = acc[:, :3]
    return out


def pick_tolerance(colours):
    """The first tolerance whose replay ends at >= 3 distinct counts, min and cap among them"""
    for tol in TOLERANCES:
        _S, _Q, counts, _r = twin.replay(colours, tol, MIN, CAP)
        u = set(np.unique(counts).tolist())
        if len(u) >= 3 and MIN in u and CAP in u:
            return tol
    return None


_cache = {}


def case(name, w, h):
    """(scene, renderer, device scene, per-sample colours, tolerance, adaptive result), once per scene"""
    if name not in _cache:
        scene, renderer = scenes.config(name, w, h, CAP)
        ds = _lib.DeviceScene(scene.to_desc() if hasattr(scene, "to_desc") else scene)
        cols = per_sample_colours(ds, renderer, CAP)
        tol = pick_tolerance(cols)
        assert tol is not None, f"{name}: no tolerance of {TOLERANCES} gives >= 3 distinct counts incl. {MIN} and {CAP}"
        res = ds.render_adaptive(renderer, tol, MIN)
        _cache[name] = (scene, renderer, ds, cols, tol, res)
    return _cache[name]


@pytest.mark.parametrize("name,w,h", SCENES, ids=[s[0] for s in SCENES])
def test_replay_moments_counts_and_rounds(name, w, h):
    _scene, renderer, _ds, cols, tol, res = case(name, w, h)
    S, Q, counts, rounds = twin.replay(cols, tol, MIN, CAP)
    assert _same(res.moments[:, :3], Q), f"{name}: squares differ at {int((_u32(res.moments[:, :3]) != _u32(Q)).any(1).sum())} pixels"
    assert _same(res.accum[:, :3], S)
    assert np.array_equal(res.moments[:, 3], counts.astype(np.float32))
    assert np.array_equal(res.counts.reshape(-1), counts)
    assert res.round_pixels.tolist() == rounds
    assert len(set(counts.tolist())) >= 3 and counts.min() == MIN and counts.max() == CAP
    assert res.stats["samples"] == int(counts.astype(np.int64).sum())


@pytest.mark.parametrize("name,w,h", SCENES, ids=[s[0] for s in SCENES])
def test_each_count_group_equals_a_fixed_count_render(oracle, name, w, h):
    scene, renderer, ds, _cols, _tol, res = case(name, w, h)
    counts = res.counts.reshape(-1)
    for n in np.unique(counts):
        group = np.ascontiguousarray(np.nonzero(counts == n)[0].astype(np.uint32))
        rn = _renderer(renderer, n)
        fixed = ds.render(rn, pixel_ids=group)
        assert np.array_equal(fixed.rgb8, res.rgb8[group]), (name, int(n))
        assert _same(fixed.gamma, res.gamma[group]) and _same(fixed.linear, res.linear[group]), (name, int(n))
        acc = np.zeros((group.size, 4), np.float32)
        prog = ds.render_progressive(rn, 0, acc, pixel_ids=group)
        assert _same(acc, res.accum[group]), (name, int(n))
        assert np.array_equal(prog.rgb8, res.rgb8[group])
        if name in ("C2_cornell_box", "C3_suzanne"):
            ora = oracle.render(scene, rn, pixel_ids=group)
            assert np.array_equal(ora.rgb8, res.rgb8[group]), (name, int(n), int((ora.rgb8 != res.rgb8[group]).sum()))


def test_whole_frame_below_1024_pixels_row_order():
    scene, renderer = scenes.config("C2_cornell_box", 30, 30, 32)
    ds = _lib.DeviceScene(scene.to_desc())
    res = ds.render_adaptive(renderer, 0.05, 4)
    counts = res.counts.reshape(-1)
    for n in np.unique(counts):
        group = np.ascontiguousarray(np.nonzero(counts == n)[0].astype(np.uint32))
        assert np.array_equal(ds.render(_renderer(renderer, n), pixel_ids=group).rgb8, res.rgb8[group])
    cols = per_sample_colours(ds, renderer, 32)
    _S, Q, c2, rounds = twin.replay(cols, 0.05, 4, 32)
    assert _same(res.moments[:, :3], Q) and np.array_equal(counts, c2) and res.round_pixels.tolist() == rounds


def test_huge_tolerance_stops_every_finite_pixel_at_min():
    scene, renderer = scenes.config("C4a_hdri_test", 64, 64, CAP)
    ds = _lib.DeviceScene(scene.to_desc())
    res = ds.render_adaptive(renderer, 1e30, MIN)
    finite = np.isfinite(res.accum[:, :3]).all(1) & np.isfinite(res.moments[:, :3]).all(1)
    counts = res.counts.reshape(-1)
    assert (counts[finite] == MIN).all() and (counts[~finite] == CAP).all()
    fixed = ds.render(_renderer(renderer, MIN))
    assert np.array_equal(fixed.rgb8[finite], res.rgb8[finite]) and _same(fixed.linear[finite], res.linear[finite])


def test_cap_equal_to_min_is_one_round():
    scene, renderer = scenes.config("C2_cornell_box", 64, 48, 8)
    ds = _lib.DeviceScene(scene.to_desc())
    res = ds.render_adaptive(renderer, 1e-6, 8)
    assert res.round_pixels.tolist() == [64 * 48] + [0] * 31
    assert (res.counts == 8).all()
    fixed = ds.render(renderer)
    assert np.array_equal(fixed.rgb8, res.rgb8) and _same(fixed.gamma, res.gamma) and _same(fixed.linear, res.linear)


def test_tiny_tolerance_runs_every_varying_pixel_to_the_cap():
    """tol = 1e-30: (t * t) underflows to 0, so a pixel stops early only where its v <= 0 (its samples are equal, or their variance rounds
    to <= 0); every pixel whose v stays > 0 runs to the cap."""
    scene, renderer = scenes.config("C4b_volume_test", 64, 64, 32)
    ds = _lib.DeviceScene(scene.to_desc())
    res = ds.render_adaptive(renderer, 1e-30, 4)
    cols = per_sample_colours(ds, renderer, 32)
    S, Q, counts, rounds = twin.replay(cols, 1e-30, 4, 32)
    assert np.array_equal(res.counts.reshape(-1), counts) and res.round_pixels.tolist() == rounds
    assert _same(res.moments[:, :3], Q) and _same(res.accum[:, :3], S)
    early = counts < 32
    n = counts[early].astype(np.float32)[:, None]
    with np.errstate(all="ignore"):
        v = (Q[early] - S[early] * (S[early] / n)) / (n - np.float32(1))
    assert (np.isfinite(S[early]).all(1) & (v <= 0).all(1)).all()
    assert (counts == 32).sum() > counts.size // 2


OPTION_SETS = [dict(STREAMS="1"), dict(PATHS_PER_BATCH="3000"), dict(NO_ZERO_SKIP="1"), dict(DEP_PIXEL_MAJOR="1"),
               dict(NO_TILE_ORDER="1"), dict(BVH="median"), dict(WIDE="0"), dict(GRAPH="1")]


@pytest.mark.parametrize("name", ["C2_cornell_box", "C3_suzanne"])
def test_options_do_not_change_the_outputs(name):
    scene, renderer = scenes.config(name, 64, 48, 32)
    desc = scene.to_desc()
    base = _lib.DeviceScene(desc).render_adaptive(renderer, 0.05, 4)
    assert len(base.rounds) >= 3
    for opts in OPTION_SETS:
        with _lib.options(**opts):
            ds = _lib.DeviceScene(desc)            # (BVH / WIDE apply to scenes created under them)
            for _rep in range(2 if "GRAPH" in opts else 1):
                got = ds.render_adaptive(renderer, 0.05, 4)
                for f in ("rgb8", "gamma", "linear", "accum", "moments", "round_pixels"):
                    a, b = getattr(got, f), getattr(base, f)
                    if f == "accum" and "NO_ZERO_SKIP" in opts:      # accum.w counts the segments of the samples that DEPOSITED a record, and
                        a, b = a[:, :3], b[:, :3]                     # NO_ZERO_SKIP deposits the zeros too (as in fw_render_progressive)
                    assert _same(a, b), (name, opts, f)
            ds.close()


def test_plain_renders_around_an_adaptive_render_keep_their_bytes():
    scene, renderer = scenes.config("C1_random_spheres", 96, 64, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    with _lib.options(GRAPH="1"):
        a = [ds.render(renderer) for _ in range(3)]              # the second and third are a captured / replayed frame graph
        assert a[2].stats["reserved"] & 0x80000000
        big = _renderer(renderer, 64)
        big.settings["width"], big.settings["height"] = 400, 300
        ds.render_adaptive(big, 0.02, 4)
        b = [ds.render(renderer) for _ in range(3)]
    for r in a[1:] + b:
        assert np.array_equal(r.rgb8, a[0].rgb8) and _same(r.linear, a[0].linear)


def test_adaptive_after_release_workspace():
    scene, renderer = scenes.config("C2_cornell_box", 64, 48, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    first = ds.render_adaptive(renderer, 0.05, 4)
    _lib.release_workspace(0)
    again = ds.render_adaptive(renderer, 0.05, 4)
    for f in ("rgb8", "linear", "accum", "moments", "round_pixels"):
        assert _same(getattr(first, f), getattr(again, f)), f


def test_device_outputs_equal_host_outputs():
    import torch
    scene, renderer = scenes.config("C3_suzanne", 64, 48, 32)
    ds = _lib.DeviceScene(scene.to_desc())
    host = ds.render_adaptive(renderer, 0.05, 4)
    n = 64 * 48
    dev = torch.device("cuda", 0)
    out = dict(rgb8=torch.full((n, 3), 7, dtype=torch.uint8, device=dev), gamma=torch.full((n, 3), -1.0, device=dev),
               linear=torch.full((n, 3), -1.0, device=dev), accum=torch.full((n, 4), -1.0, device=dev),
               moments=torch.full((n, 4), -1.0, device=dev), round_pixels=torch.full((32,), -1, dtype=torch.int32, device=dev))
    got = ds.render_adaptive(renderer, 0.05, 4, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out["rgb8"].cpu().numpy(), host.rgb8)
    for f in ("gamma", "linear", "accum", "moments"):
        assert _same(out[f].cpu().numpy(), getattr(host, f)), f
    assert out["round_pixels"].cpu().numpy().astype(np.uint32).tolist() == host.round_pixels.tolist()
    assert got.stats["samples"] == host.stats["samples"]


def test_cli_adaptive(tmp_path):
    from firework_amd import yaml_io
    path = tmp_path / "s.yml"
    scene, _r = scenes.config("conics", 8, 8, 1)
    yaml_io.save_scene(scene, str(path))
    out = tmp_path / "o.png"
    p = subprocess.run([sys.executable, "-m", "firework_amd", "--scene-file", str(path), "-s", "32", "--adaptive", "0.05", "--min-samples", "4",
                        "--width", "64", "--height", "48", "-o", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "rounds" in p.stdout and "spp" in p.stdout and out.exists()


CPP = r"""
#include "firework.hpp"
#include <cstdio>
using namespace firework;
int main() {
    Scene world = Scene::new_();
    MaterialIdx red = world.add_material(LambertianMat::with_color({0.65f, 0.05f, 0.05f}));
    MaterialIdx white = world.add_material(LambertianMat::with_color({0.73f, 0.73f, 0.73f}));
    MaterialIdx green = world.add_material(LambertianMat::with_color({0.12f, 0.45f, 0.15f}));
    MaterialIdx light = world.add_material(EmissiveMat::with_color({15.f, 15.f, 15.f}));
    world.add_object(RenderObject::new_(XZRect::new_(213.f, 343.f, 227.f, 332.f, 554.f, light)));
    world.add_object(RenderObject::new_(YZRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, green)).flip_normals());
    world.add_object(RenderObject::new_(YZRect::new_(0.f, 555.f, 0.f, 555.f, 0.f, red)));
    world.add_object(RenderObject::new_(XZRect::new_(0.f, 555.f, 0.f, 555.f, 0.f, white)));
    world.add_object(RenderObject::new_(XZRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, white)).flip_normals());
    world.add_object(RenderObject::new_(XYRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, white)).flip_normals());
    CameraSettings camera = CameraSettings::default_().cam_pos({278.f, 278.f, -800.f}).look_at({278.f, 278.f, 0.f}).field_of_view(40.f);
    Renderer r = Renderer::default_().width(48).height(40).samples(32).camera(camera);
    std::vector<uint32_t> counts;
    std::vector<Color> img = r.render_adaptive(world, 0.05f, 4, &counts);
    unsigned long long h = 1469598103934665603ull, hc = 1469598103934665603ull;
    for (const Color &c : img) for (uint8_t b : {c.r, c.g, c.b}) { h ^= b; h *= 1099511628211ull; }
    for (uint32_t c : counts) { hc ^= c; hc *= 1099511628211ull; }
    std::printf("img=%016llx counts=%016llx\n", h, hc);
    return 0;
}
"""


def test_cpp_host_render_adaptive(tmp_path):
    from firework_amd.api import (CameraSettings, EmissiveMat, LambertianMat, Renderer, RenderObject, Scene, XYRect, XZRect, YZRect)
    src = tmp_path / "adaptive.cpp"
    src.write_text(CPP)
    exe = tmp_path / "adaptive"
    libdir = os.path.join(ROOT, "firework_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", libdir,
                           "-lfirework_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
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
    cam = CameraSettings.default().cam_pos((278.0, 278.0, -800.0)).look_at((278.0, 278.0, 0.0)).field_of_view(40.0)
    res = Renderer.default().width(48).height(40).samples(32).camera(cam).render_adaptive(w, 0.05, 4)
    h = hc = 1469598103934665603
    for b in res.rgb8.reshape(-1).tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    for c in res.counts.reshape(-1).tolist():
        hc = ((hc ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert out.stdout.strip() == f"img={h:016x} counts={hc:016x}"
