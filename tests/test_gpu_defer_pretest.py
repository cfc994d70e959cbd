"""The box-list scan's pre-test (fw_defer_pretest.h: one fma per slab plane, the box grown on the host) picks the rays that go on a
deferred box's list; the exact test decides.  A pre-test that wrongly says "no" loses a hit, so every case here compares the GPU with
the CPU oracle at zero tolerance: the u8 frame, the rays per depth, and — all materials here have constant textures, so the chain state
applies and the pre-gamma means are the oracle's bits — the linear frame.  The host proof of the pre-test itself is
tools/defer_pretest_check.cpp."""
import os
import sys

import numpy as np
import pytest

from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, Cone, EmissiveMat, LambertianMat, Rect3d, RenderObject, Renderer, Rotor3, Scene, XYRect,
                              XZRect, YZRect)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_trace as T  # noqa: E402  (its ray sets and its record comparison)

pytestmark = pytest.mark.gpu

W, H, SPP = 48, 32, 8


def _sized(r):
    return r.width(W).height(H).samples(SPP).use_bvh(False).seed(11)


def cornell():
    sc, r = scenes.cornell_box()
    return sc, _sized(r)


def one_box():
    sc, r = scenes.cornell_box()
    del sc.render_objects[-1:]
    return sc, _sized(r)


def two_boxes_one_unrotated():
    """cornell's room; the short box as it is, the tall one unrotated (to_object_space without a rotation, and a direction component
    of 0 in the world is one in the box's frame)"""
    sc, r = scenes.cornell_box()
    del sc.render_objects[-1:]
    sc.add_object(RenderObject.new(Rect3d.with_size((165.0, 330.0, 165.0), 1)).position(265.0, 0.0, 295.0))
    return sc, _sized(r)


def with_cone():
    """a cone ahead of the two boxes: no longer the SIMPLE set of shapes, the boxes still deferred (k_extend_linear_defer<false>)"""
    sc, r = scenes.cornell_box()
    boxes = sc.render_objects[-2:]
    del sc.render_objects[-2:]
    sc.add_object(RenderObject.new(Cone.new(60.0, 120.0, 1)).position(420.0, 0.0, 120.0))
    sc.render_objects += boxes
    return sc, _sized(r)


def far_box():
    """A floor, a wall, a light and one rotated box about 1e4 from the origin on every axis, the camera one unit in front of the box:
    the margin's origin term and the centre form's cancellation at |o| / extent ~ 2^13"""
    ox, oy, oz = 1e4, 1e4, -1e4
    sc = Scene.new()
    white = sc.add_material(LambertianMat.with_color((0.73, 0.73, 0.73)))
    green = sc.add_material(LambertianMat.with_color((0.12, 0.45, 0.15)))
    light = sc.add_material(EmissiveMat.with_color((6.0, 6.0, 6.0)))
    sc.add_object(RenderObject.new(XZRect.new(ox - 4, ox + 4, oz - 4, oz + 6, oy, white)))
    sc.add_object(RenderObject.new(XZRect.new(ox - 1.5, ox + 1.5, oz, oz + 3, oy + 3.0, light)).flip_normals())
    sc.add_object(RenderObject.new(XYRect.new(ox - 4, ox + 4, oy, oy + 4, oz + 4.0, green)).flip_normals())
    sc.add_object(RenderObject.new(YZRect.new(oy, oy + 4, oz - 4, oz + 6, ox - 3.0, white)))
    sc.add_object(RenderObject.new(Rect3d.with_size((1.0, 1.2, 1.0), white)).rotate(Rotor3.from_rotation_xz(0.4)).position(ox - 0.5, oy, oz + 1.0))
    cam = CameraSettings.default().cam_pos((ox + 0.1, oy + 0.8, oz - 0.2)).look_at((ox, oy + 0.5, oz + 1.5)).field_of_view(60.0)
    return sc, _sized(Renderer.default().camera(cam))


CASES = {
    "cornell": (cornell, "k_extend_linear_defer<true>"),
    "one_box": (one_box, "k_extend_linear_defer<true>"),
    "two_boxes_one_unrotated": (two_boxes_one_unrotated, "k_extend_linear_defer<true>"),
    "far_box": (far_box, "k_extend_linear_defer<true>"),
    "cone": (with_cone, "k_extend_linear_defer<false>"),
}


@pytest.fixture(scope="module")
def frames(oracle):
    """Per case: (scene, renderer, the oracle's frame), made once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            sc, r = CASES[name][0]()
            cache[name] = (sc, r, oracle.render(sc, r))
        return cache[name]
    return get


def same_frame(gpu, cpu, what):
    d8 = int((gpu.rgb8 != cpu.rgb8).sum())
    lin = int((np.ascontiguousarray(gpu.linear, np.float32).view(np.uint32) != np.ascontiguousarray(cpu.linear, np.float32).view(np.uint32)).sum())
    print(f"{what}: u8 differences {d8}, linear words that differ {lin}, rays gpu {gpu.stats['rays']} oracle {cpu.stats['rays']}")
    assert list(gpu.stats["rays_per_depth"]) == list(cpu.stats["rays_per_depth"]), what
    assert d8 == 0, what
    assert lin == 0, what


@pytest.mark.parametrize("name", list(CASES))
def test_frames_are_the_oracles(frames, name):
    sc, r, cpu = frames(name)
    gpu = r.render_full(sc)
    kernels = _lib.last_kernels()
    assert CASES[name][1] in kernels, kernels                               # the pre-test under test ran
    assert any(k.startswith("k_shade") and "chain" in k for k in kernels), kernels      # ... and the linear frame is comparable bit for bit
    same_frame(gpu, cpu, name)


@pytest.mark.parametrize("name", ["cornell", "two_boxes_one_unrotated"])
def test_without_the_lists_the_frame_is_the_same(frames, name):
    sc, r, cpu = frames(name)
    with _lib.options(NO_DEFER="1"):
        plain = r.render_full(sc)
        kernels = _lib.last_kernels()
    assert not any(k.startswith("k_extend_linear_defer") for k in kernels), kernels
    same_frame(plain, cpu, name + " NO_DEFER")
    listed = r.render_full(sc)
    assert np.array_equal(listed.linear, plain.linear) and listed.stats["rays_per_depth"] == plain.stats["rays_per_depth"]


def test_ray_queries_on_the_two_box_scene(oracle, frames):
    """fw_trace_rays through the box-list scan: the camera rays, the secondary rays of real paths and the adversarial set of
    test_gpu_trace.py (axis-parallel directions, signed zeros, origins on surfaces leaving along them) — every record the oracle's."""
    sc, r, _cpu = frames("two_boxes_one_unrotated")
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        cam = T.camera_set(ds, r)
        sets = (("camera", cam), ("secondary", T.secondary_set(oracle, sc, r)), ("adversarial", T.adversarial_set(oracle, sc, ds, 0, cam[:4096])))
        for label, rays in sets:
            gpu = ds.trace(rays, 0)
            assert "k_extend_linear_defer<true>" in _lib.last_kernels(), _lib.last_kernels()
            T.compare(gpu, oracle.trace(sc, rays, 0), f"two boxes, {label}")
    finally:
        ds.close()
