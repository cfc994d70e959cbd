"""Every emitter (FW_FLAG_ALL_EMITTERS) without a GPU: the entry list fw_selftest_emitters reports equals the float64
restatement (tests/emitters_ref.py) on a scene with every entry kind, and the public switch — the flag's value in the header,
Renderer.all_emitters, the C++ Renderer and the CLI."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib
from firework_amd.api import (CheckerTexture, ConstantTexture, Cone, Disk, EmissiveMat, LambertianMat, Rect3d, Renderer, RenderObject, Rotor3,
                              Scene, Sphere, TriangleMesh, XYRect, XZRect, YZRect)

import emitters_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_mesh(n, size=1.0, material=0):
    """an n x n grid of 2 n^2 triangles in the y = 0 plane, [-size, size]^2, with a ripple so that the areas differ"""
    s = np.linspace(-size, size, n + 1)
    X, Z = np.meshgrid(s, s, indexing="ij")
    Y = 0.05 * np.sin(3 * X) * np.cos(2 * Z)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    idx = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            idx += [a, b, c, a, c, d]
    return TriangleMesh(verts, np.array(idx, np.uint32), material=material)


def every_kind_scene():
    scene = Scene.new()
    diff = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    e1 = scene.add_material(EmissiveMat.with_color((4.0, 2.0, 1.0)))
    e2 = scene.add_material(EmissiveMat.with_color((0.5, -3.0, float("nan"))))      # negative and NaN channels count as 0: power 0.5
    black = scene.add_material(EmissiveMat.with_color((0.0, 0.0, 0.0)))           # power 0: no entries
    chk = scene.add_material(EmissiveMat.new(CheckerTexture.new(ConstantTexture.new((9.0, 1.0, 1.0)), ConstantTexture.new((1.0, 9.0, 1.0)), 2.0)))
    scene.add_object(RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, diff)))
    scene.add_object(RenderObject.new(Sphere.new(0.7, e1)).position(1.0, 3.0, 0.0))
    scene.add_object(RenderObject.new(XYRect.new(0, 2, 1, 4, 5, e2)).position(1.0, 2.0, 3.0))
    scene.add_object(RenderObject.new(YZRect.new(-1, 1, 0, 3, 2, chk)))
    scene.add_object(RenderObject.new(Rect3d.with_size((1.0, 2.0, 0.5), e1)).position(-2.0, 1.0, 0.0))
    scene.add_object(RenderObject.new(Disk.partial(1.5, 270.0, 0.5, e2)).rotate(Rotor3.from_rotation_xy(0.4)).position(0.0, 4.0, 0.0))
    mesh = grid_mesh(3, 0.8, material=chk)
    scene.add_object(RenderObject.new(mesh).rotate(Rotor3.from_rotation_yz(0.7)).position(0.0, 5.0, 1.0))     # one mesh, two objects
    scene.add_object(RenderObject.new(mesh).position(3.0, 5.0, -1.0))
    scene.add_object(RenderObject.new(Sphere.new(0.5, black)).position(-3.0, 2.0, 0.0))
    scene.add_object(RenderObject.new(Cone.new(0.5, 1.0, e1)).position(2.5, 0.0, 1.5))                     # never an entry
    scene.add_object(RenderObject.new(Sphere.new(0.5, diff)))
    return scene


def test_table_matches_float64():
    scene = every_kind_scene()
    got = _lib.selftest_emitters(scene.to_desc())
    want = ref.entries(scene)
    for k in ("obj", "prim", "kind"):
        assert np.array_equal(got[k], want[k]), k
    assert np.allclose(got["area"], want["area"], rtol=1e-6, atol=0)
    assert np.allclose(got["weight"], want["weight"], rtol=1e-6, atol=0)
    kinds = set(got["kind"].tolist())
    assert kinds == {A.FW_SHAPE_SPHERE, A.FW_SHAPE_XYRECT, A.FW_SHAPE_YZRECT, A.FW_SHAPE_RECT3D, A.FW_SHAPE_DISK, A.FW_SHAPE_TRIANGLE_MESH}
    assert (got["kind"] == A.FW_SHAPE_RECT3D).sum() == 6 and (got["kind"] == A.FW_SHAPE_TRIANGLE_MESH).sum() == 2 * 18
    objs = set(got["obj"].tolist())
    assert isinstance(scene.render_objects[8].obj, Sphere) and isinstance(scene.render_objects[9].obj, Cone)
    assert 8 not in objs and 9 not in objs and 10 not in objs        # the black sphere, the emissive cone, the diffuse sphere
    assert objs == {1, 2, 3, 4, 5, 6, 7}
    assert np.all(got["weight"] > 0)
    disk = got["kind"] == A.FW_SHAPE_DISK
    assert got["area"][disk][0] == pytest.approx(0.5 * np.radians(270.0) * (1.5 ** 2 - 0.5 ** 2), rel=1e-6)


def test_no_entries():
    scene = Scene.new()
    scene.add_object(RenderObject.new(XZRect.new(-1, 1, -1, 1, 0, scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5))))))
    assert _lib.selftest_emitters(scene.to_desc())["obj"].size == 0


def test_flag_matches_header():
    hdr = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert int(re.search(r"#define FW_FLAG_ALL_EMITTERS (\d+)u", hdr).group(1)) == A.FW_FLAG_ALL_EMITTERS == 16
    assert int(re.search(r"#define FW_EMITTER_RECORD_FLOATS (\d+)", hdr).group(1)) == A.FW_EMITTER_RECORD_FLOATS
    assert int(re.search(r"#define FW_EMITTER_SAMPLE_FLOATS (\d+)", hdr).group(1)) == A.FW_EMITTER_SAMPLE_FLOATS
    assert int(re.search(r"#define FW_ABI_VERSION (\d+)", hdr).group(1)) == 8


def test_renderer_switch():
    r = Renderer.default().light_sampling()
    r.all_emitters()
    assert r.to_params().flags == A.FW_FLAG_LIGHT_SAMPLING | A.FW_FLAG_ALL_EMITTERS
    r.all_emitters(False)
    assert r.to_params().flags == A.FW_FLAG_LIGHT_SAMPLING
    src = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "Renderer all_emitters(bool on = true)" in src and "FW_FLAG_ALL_EMITTERS" in src


def test_cli_accepts_flag():
    out = subprocess.run([sys.executable, "-m", "firework_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--all-emitters" in out.stdout
    src = open(os.path.join(ROOT, "firework_amd", "__main__.py")).read()
    assert "renderer.light_sampling().all_emitters()" in src


def test_selftests_reject_null():
    lib = _lib.load()
    n = C.c_uint32()
    assert lib.fw_selftest_emitters(None, None, 0, C.byref(n)) == A.FW_ERR_BAD_ARG
    x = np.zeros(3, np.float32)
    assert lib.fw_selftest_emitter_sample(None, x.ctypes.data, 1, 1, x.ctypes.data) == A.FW_ERR_BAD_ARG
