"""Light sampling (FW_FLAG_LIGHT_SAMPLING) without a GPU: the light table fw_selftest_lights reports (which objects are
sampled lights, in which frame), the densities the estimator's MIS weights rest on — the direction of n + u with u uniform in the unit
ball (util.rs:36-43's rejection, material.rs:66) follows 2 cos^3 / pi, and u alone (material.rs:201) is uniform — and the public switch:
the flag's value in the header, Renderer.light_sampling and the CLI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import (ConstantMedium, ConstantTexture, Cone, Disk, EmissiveMat, LambertianMat, Rect3d, Renderer, RenderObject,
                              Rotor3, Scene, Sphere, TriangleMesh, XYRect, XZRect, YZRect)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lights_of(scene):
    return _lib.selftest_lights(scene.to_desc())


def test_cornell_light():
    scene, _ = scenes.config("C2_cornell_box", 16, 16, 1)
    L = lights_of(scene)
    assert len(L) == 1
    l0 = L[0]
    assert l0["kind"] == A.FW_SHAPE_XZRECT and l0["area"] == pytest.approx(130 * 105) and l0["p_pick"] == 1.0
    c = l0["corners"]
    assert np.all(c[:, 1] == 554.0)
    assert c[:, 0].min() == 213.0 and c[:, 0].max() == 343.0 and c[:, 2].min() == 227.0 and c[:, 2].max() == 332.0
    assert isinstance(scene.render_objects[l0["obj"]].obj, XZRect)


def test_volume_test_rotated_light():
    scene, _ = scenes.config("C4b_volume_test", 16, 16, 1)
    L = lights_of(scene)
    assert len(L) == 1 and L[0]["kind"] == A.FW_SHAPE_YZRECT and L[0]["area"] == pytest.approx(200.0)
    ro = scene.render_objects[L[0]["obj"]]
    pos = np.asarray(ro._position, np.float64)
    local = np.array([[-3.0, 0.0, 0.0], [-3.0, 20.0, 0.0], [-3.0, 20.0, 10.0], [-3.0, 0.0, 10.0]])     # YZRect (a = y in 0..20, b = z in 0..10) at x = -3
    world = L[0]["corners"] - pos
    # rotated (the rotation is far from the identity: cos_trace < 0.999) and rigidly: R p for an orthonormal R with det 1
    assert not np.allclose(world, local, atol=1e-3)
    R, *_ = np.linalg.lstsq(local, world, rcond=None)
    R = R.T
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-5) and np.linalg.det(R) == pytest.approx(1.0, abs=1e-5)
    assert np.allclose(local @ R.T, world, atol=1e-4)
    assert abs(R[1, 1] - 1.0) < 1e-6        # a rotation in the xz plane leaves y alone


def _scene_with(objs):
    scene = Scene.new()
    emit = scene.add_material(EmissiveMat.with_color((4.0, 4.0, 4.0)))
    diff = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    ids = {}
    for name, make in objs:
        ids[name] = scene.add_object(make(emit, diff))
    return scene, ids


def test_which_objects_are_lights():
    near = Rotor3.from_rotation_xz(0.01)          # cos_trace > 0.999: the reference intersects it unrotated
    cube = TriangleMesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([0, 1, 2], np.uint32), material=0)
    scene, ids = _scene_with([
        ("floor", lambda e, d: RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, d))),
        ("rect", lambda e, d: RenderObject.new(XYRect.new(0, 2, 1, 4, 5, e)).position(1.0, 2.0, 3.0)),
        ("near", lambda e, d: RenderObject.new(XZRect.new(-1, 1, -2, 2, 7, e)).rotate(near).position(0.5, 0.0, 0.0)),
        ("sphere", lambda e, d: RenderObject.new(Sphere.new(1.5, e)).position(3.0, 4.0, 5.0)),
        ("box", lambda e, d: RenderObject.new(Rect3d.with_size((1, 1, 1), e))),
        ("disk", lambda e, d: RenderObject.new(Disk.new(1.0, e))),
        ("cone", lambda e, d: RenderObject.new(Cone.new(1.0, 2.0, e))),
        ("mesh", lambda e, d: RenderObject.new(cube)),
        ("plain_sphere", lambda e, d: RenderObject.new(Sphere.new(1.0, d))),
    ])
    scene.add_volume(RenderObject.new(Sphere.new(2.0, 0)), 0.1, ConstantTexture.new((1.0, 1.0, 1.0)))     # a medium around an emissive sphere shape
    L = lights_of(scene)
    assert [l["obj"] for l in L] == [ids["rect"], ids["near"], ids["sphere"]]
    assert sum(l["p_pick"] for l in L) == pytest.approx(1.0) and all(l["p_pick"] == pytest.approx(1 / 3) for l in L)
    rect = L[0]
    assert rect["kind"] == A.FW_SHAPE_XYRECT and rect["area"] == pytest.approx(6.0)
    assert np.allclose(np.sort(rect["corners"], axis=0), np.sort(np.array([[0, 1, 5], [2, 1, 5], [2, 4, 5], [0, 4, 5]]) + [1, 2, 3], axis=0))
    near_l = L[1]     # listed unrotated: the corners are the object-space ones + the position
    assert np.array_equal(np.sort(near_l["corners"], axis=0),
                          np.sort(np.array([[-1, 7, -2], [1, 7, -2], [1, 7, 2], [-1, 7, 2]], np.float64) + [0.5, 0, 0], axis=0))
    sph = L[2]
    assert sph["kind"] == A.FW_SHAPE_SPHERE and np.array_equal(sph["centre"], [3, 4, 5]) and sph["radius"] == 1.5
    assert sph["area"] == pytest.approx(4 * np.pi * 1.5 ** 2)


def test_no_lights():
    scene, _ = _scene_with([("floor", lambda e, d: RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, d)))])
    assert lights_of(scene) == []


# ---- the densities of §9g -----------------------------------------------------------------------------------------------------------
def _unit_ball(rng, n):
    """util.rs:36-43: 2 u - 1 for u uniform in the unit cube, rejected until |p|^2 < 1 (f32 arithmetic)"""
    out = np.empty((0, 3), np.float32)
    while out.shape[0] < n:
        p = (2.0 * rng.random((2 * n, 3), dtype=np.float32) - 1.0).astype(np.float32)
        out = np.concatenate([out, p[(p * p).sum(1) < 1.0]])
    return out[:n]


def _chi2_ok(counts, expected):
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    dof = len(counts) - 1
    return chi2 < dof + 5 * np.sqrt(2 * dof), chi2


def test_lambertian_density_is_2cos3_over_pi():
    rng = np.random.default_rng(1)
    n = np.array([0.0, 0.0, 1.0], np.float32)
    d = n[None, :] + _unit_ball(rng, 10 ** 6)
    c = d[:, 2] / np.linalg.norm(d, axis=1)
    assert c.min() >= 0.0
    edges = np.linspace(0.0, 1.0, 41)
    counts, _ = np.histogram(c, edges)
    # P(cos in [a, b]) = int 2 c^3 / pi * 2 pi dc = c^4 | a..b
    expected = (edges[1:] ** 4 - edges[:-1] ** 4) * c.size
    ok, chi2 = _chi2_ok(counts, expected)
    assert ok, chi2
    # the general form the kernel evaluates (fw_kernels.hip: scatter_pdf) reduces to it for |n| = 1
    w = np.array([np.sqrt(1 - 0.36), 0.0, 0.6])
    cc = w @ n
    tp, tm = cc + np.sqrt(cc * cc - 1 + 1), max(cc - np.sqrt(cc * cc), 0.0)
    assert (tp ** 3 - tm ** 3) / (4 * np.pi) == pytest.approx(2 * 0.6 ** 3 / np.pi)


def test_isotropic_directions_are_uniform():
    rng = np.random.default_rng(2)
    u = _unit_ball(rng, 10 ** 6).astype(np.float64)
    d = u / np.linalg.norm(u, axis=1)[:, None]
    for axis in range(3):
        counts, _ = np.histogram(d[:, axis], np.linspace(-1, 1, 41))
        ok, chi2 = _chi2_ok(counts, np.full(40, d.shape[0] / 40.0))
        assert ok, (axis, chi2)
    phi = np.arctan2(d[:, 1], d[:, 0])
    counts, _ = np.histogram(phi, np.linspace(-np.pi, np.pi, 37))
    assert _chi2_ok(counts, np.full(36, d.shape[0] / 36.0))[0]


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def test_flag_matches_header():
    hdr = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    m = re.search(r"#define FW_FLAG_LIGHT_SAMPLING (\d+)u", hdr)
    assert m and int(m.group(1)) == A.FW_FLAG_LIGHT_SAMPLING == 4
    assert int(re.search(r"#define FW_LIGHT_RECORD_FLOATS (\d+)", hdr).group(1)) == A.FW_LIGHT_RECORD_FLOATS


def test_renderer_switch():
    r = Renderer.default().time_kernels(True)
    r.light_sampling()
    assert r.to_params().flags == A.FW_FLAG_TIME_KERNELS | A.FW_FLAG_LIGHT_SAMPLING
    r.light_sampling(False)
    assert r.to_params().flags == A.FW_FLAG_TIME_KERNELS


def test_cli_accepts_flag():
    out = subprocess.run([sys.executable, "-m", "firework_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--light-sampling" in out.stdout
    src = open(os.path.join(ROOT, "firework_amd", "__main__.py")).read()
    assert ".light_sampling(opt.light_sampling)" in src


def test_selftest_rejects_null():
    import ctypes as C
    lib = _lib.load()
    n = C.c_uint32()
    assert lib.fw_selftest_lights(None, None, 0, C.byref(n)) == A.FW_ERR_BAD_ARG
