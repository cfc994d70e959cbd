"""Light sampling (FW_FLAG_LIGHT_SAMPLING) on the GPU.  The paths of a light-sampling frame are the default frame's (the same
ray counts per segment, under kernel-selecting options too); scenes where nothing samples a light render the default frame bit for bit;
probes through fw_render_rays meet the known answer a Le int 2 cos^3 / pi dw (rect lights parallel and tilted, a sphere light); over seeds
the frame agrees with the default estimator (cornell, volume_test, a coverage scene); on cornell it has less noise at equal samples; and
subsets, progressive passes, repeats, caller rays and fw_scene_update compose bit for bit."""
import copy

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, CheckerTexture, ConstantTexture, Cone, DielectricMat, EmissiveMat, LambertianMat, MetalMat,
                              Renderer, RenderObject, Rotor3, Scene, Sphere, XYRect, XZRect, YZRect)

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ls(r, on=True, **kw):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    rr.light_sampling(on)
    for k, v in kw.items():
        getattr(rr, k)(v)
    return rr


def _same(a, b):
    assert np.array_equal(a.rgb8, b.rgb8)
    assert np.array_equal(_u32(a.gamma), _u32(b.gamma)) and np.array_equal(_u32(a.linear), _u32(b.linear))


# ---- 1. the paths are the default frame's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1_random_spheres", "C2_cornell_box", "C3_suzanne", "C4a_hdri_test", "C4b_volume_test", "C5_part2_all"])
def test_same_paths(name):
    scene, r = scenes.config(name, 64, 48, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    a, b = ds.render(r), ds.render(_ls(r))
    assert a.stats["rays"] == b.stats["rays"]
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in b.stats["rays_per_depth"]]


@pytest.mark.parametrize("opt", [dict(BVH="median"), dict(WIDE="0"), dict(EXACT_ALL="1")])
@pytest.mark.parametrize("name", ["C2_cornell_box", "C4b_volume_test"])
def test_same_paths_under_options(name, opt):
    scene, r = scenes.config(name, 64, 48, 16)
    r.use_bvh(True)
    ds = _lib.DeviceScene(scene.to_desc())
    with _lib.options(**opt):
        a, b = ds.render(r), ds.render(_ls(r))
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in b.stats["rays_per_depth"]]


# ---- 2. nothing to sample: the default frame --------------------------------------------------------------------------------------------
def _metal_glass_scene():
    scene = Scene.new()
    metal = scene.add_material(MetalMat.new((0.8, 0.7, 0.6), 0.1))
    glass = scene.add_material(DielectricMat.new(1.5))
    light = scene.add_material(EmissiveMat.with_color((5.0, 5.0, 5.0)))
    scene.add_object(RenderObject.new(XZRect.new(-20, 20, -20, 20, 0, metal)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, glass)).position(0.0, 1.0, 0.0))
    scene.add_object(RenderObject.new(XZRect.new(-2, 2, -2, 2, 5, light)))
    cam = CameraSettings.default().cam_pos((0.0, 3.0, 8.0)).look_at((0.0, 1.0, 0.0)).field_of_view(50.0)
    return scene, Renderer.default().width(48).height(32).samples(16).use_bvh(True).camera(cam)


@pytest.mark.parametrize("which", ["metal_glass", "C1_random_spheres", "C4a_hdri_test"])
def test_default_frame_where_nothing_samples(which):
    scene, r = _metal_glass_scene() if which == "metal_glass" else scenes.config(which, 48, 32, 8)
    ds = _lib.DeviceScene(scene.to_desc())
    _same(ds.render(r), ds.render(_ls(r)))


# ---- 3. known answers -----------------------------------------------------------------------------------------------------------------
ALB, LE = 0.5, 4.0


def _probe_scene(light):
    scene = Scene.new()
    floor = scene.add_material(LambertianMat.with_color((ALB, ALB, ALB)))
    emit = scene.add_material(EmissiveMat.with_color((LE, LE, LE)))
    scene.add_object(RenderObject.new(XZRect.new(-1000, 1000, -1000, 1000, 0, floor)))
    if light == "parallel":
        scene.add_object(RenderObject.new(XZRect.new(-1, 1, -0.5, 0.5, 0, emit)).position(0.5, 2.0, 0.0))
    elif light == "tilted":
        scene.add_object(RenderObject.new(XZRect.new(-1, 1, -0.5, 0.5, 0, emit)).rotate(Rotor3.from_rotation_xy(0.6)).position(0.8, 1.5, 0.2))
    else:
        scene.add_object(RenderObject.new(Sphere.new(0.4, emit)).position(0.7, 1.2, -0.3))
    return scene


def _integral(scene, P):
    """int over the light of 2 cos^3(theta) / pi dw seen from floor point P (normal +y), by quadrature"""
    (l,) = _lib.selftest_lights(scene.to_desc())
    P = np.asarray(P, np.float64)
    if l["kind"] == A.FW_SHAPE_SPHERE:
        c, r = l["centre"] - P, l["radius"]
        d = np.linalg.norm(c)
        w = c / d
        cmax = np.sqrt(1 - (r / d) ** 2)
        n = 2000
        ct = 1 - (np.arange(n) + 0.5) / n * (1 - cmax)
        ph = (np.arange(n) + 0.5) / n * 2 * np.pi
        CT, PH = np.meshgrid(ct, ph, indexing="ij")
        ST = np.sqrt(1 - CT ** 2)
        a = np.array([1.0, 0, 0]) if abs(w[0]) < 0.9 else np.array([0, 1.0, 0])
        e1 = np.cross(w, a); e1 /= np.linalg.norm(e1)
        e2 = np.cross(w, e1)
        cy = ST * np.cos(PH) * e1[1] + ST * np.sin(PH) * e2[1] + CT * w[1]
        return float((2 * np.clip(cy, 0, None) ** 3 / np.pi).mean() * 2 * np.pi * (1 - cmax))
    c0, c1, c3 = l["corners"][0], l["corners"][1], l["corners"][3]
    e1, e2 = c1 - c0, c3 - c0
    nl = np.cross(e1, e2); area = np.linalg.norm(nl); nl /= area
    n = 1500
    s = (np.arange(n) + 0.5) / n
    S, T = np.meshgrid(s, s, indexing="ij")
    X = c0[None, None, :] + S[..., None] * e1 + T[..., None] * e2 - P
    d2 = (X ** 2).sum(-1)
    d = np.sqrt(d2)
    cos_t = np.clip(X[..., 1] / d, 0, None)
    cos_l = np.abs((X * nl).sum(-1)) / d
    return float((2 * cos_t ** 3 / np.pi * cos_l / d2).mean() * area)


@pytest.mark.parametrize("light", ["parallel", "tilted", "sphere"])
def test_known_answer(light):
    scene = _probe_scene(light)
    ds = _lib.DeviceScene(scene.to_desc())
    P = [[0.3, 0.0, 0.1], [1.2, 0.0, -0.4], [-0.6, 0.0, 0.5]]
    rays = np.array([[p[0], 0.5, p[2], 0.0, -1.0, 0.0] for p in P], np.float32)
    N = 1 << 16
    nee = ds.render_rays(rays, N, seed=3, flags=A.FW_FLAG_LIGHT_SAMPLING).linear[:, 0].astype(np.float64)
    dflt = ds.render_rays(rays, N, seed=3).linear[:, 0].astype(np.float64)
    for k, p in enumerate(P):
        I = _integral(scene, p)
        want = ALB * LE * I
        assert abs(nee[k] - want) <= 0.01 * want, (light, k, nee[k], want)
        q = I / 1.0       # the default estimator: ALB * LE with probability I (the bounce reaches the light), else 0
        sigma = ALB * LE * np.sqrt(q * (1 - q) / N)
        assert abs(dflt[k] - want) <= 4 * sigma, (light, k, dflt[k], want, sigma)


# ---- 4. no bias ------------------------------------------------------------------------------------------------------------------------
def _coverage_scene():
    scene = Scene.new()
    floor = scene.add_material(LambertianMat.with_color((0.6, 0.6, 0.6)))
    wall = scene.add_material(LambertianMat.with_color((0.3, 0.5, 0.7)))
    e1 = scene.add_material(EmissiveMat.with_color((6.0, 5.0, 4.0)))
    e2 = scene.add_material(EmissiveMat.with_color((2.0, 4.0, 6.0)))
    chk = scene.add_material(EmissiveMat.new(CheckerTexture.new(ConstantTexture.new((8.0, 1.0, 1.0)), ConstantTexture.new((1.0, 8.0, 1.0)), 4.0)))
    metal = scene.add_material(MetalMat.new((0.9, 0.9, 0.9), 0.05))
    glass = scene.add_material(DielectricMat.new(1.5))
    scene.add_object(RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, floor)))
    scene.add_object(RenderObject.new(XYRect.new(-10, 10, 0, 10, -4, wall)))
    scene.add_object(RenderObject.new(XZRect.new(-1, 1, -1, 1, 0, e1)).rotate(Rotor3.from_rotation_xy(0.5)).position(-2.0, 4.0, 0.0))     # rotated
    scene.add_object(RenderObject.new(XZRect.new(-1, 1, -1, 1, 0, e2)).rotate(Rotor3.from_rotation_xy(0.02)).position(2.0, 4.5, -1.0))    # near-identity
    scene.add_object(RenderObject.new(Sphere.new(0.5, e1)).position(0.0, 3.0, 1.0))
    scene.add_object(RenderObject.new(YZRect.new(0, 2, -1, 1, 0, chk)).position(-3.5, 0.0, -1.0))                                        # checker light
    scene.add_object(RenderObject.new(Sphere.new(0.8, metal)).position(-1.2, 0.8, 0.5))
    scene.add_object(RenderObject.new(Sphere.new(0.8, glass)).position(1.3, 0.8, 0.8))
    scene.add_object(RenderObject.new(Sphere.new(0.25, e2)).position(1.3, 0.8, -0.4))                                                  # behind the glass
    scene.add_object(RenderObject.new(Cone.new(0.5, 1.0, e2)).position(2.5, 0.0, 1.5))                                                   # not sampled
    scene.add_volume(RenderObject.new(Sphere.new(0.7, floor)).position(0.0, 0.7, -1.5), 0.8, ConstantTexture.new((0.8, 0.8, 0.8)))
    cam = CameraSettings.default().cam_pos((0.0, 3.0, 9.0)).look_at((0.0, 1.0, 0.0)).field_of_view(45.0)
    return scene, Renderer.default().width(96).height(96).samples(32).use_bvh(True).camera(cam)


def _bias_case(scene, r, seeds=8):
    ds = _lib.DeviceScene(scene.to_desc())
    W, H = r.settings["width"], r.settings["height"]
    def blocks(img):
        lum = img.reshape(H, W, 3).astype(np.float64).mean(-1)
        return lum[:H // 16 * 16, :W // 16 * 16].reshape(H // 16, 16, W // 16, 16).mean((1, 3))
    a = np.stack([blocks(ds.render(_ls(r, False, seed=s)).linear) for s in range(seeds)])
    b = np.stack([blocks(ds.render(_ls(r, True, seed=s)).linear) for s in range(seeds)])
    sigma = np.sqrt((a.var(0, ddof=1) + b.var(0, ddof=1)) / seeds)
    z = np.abs(a.mean(0) - b.mean(0)) / np.maximum(sigma, 1e-12)
    assert z.max() <= 4.0, (z.max(), np.unravel_index(z.argmax(), z.shape))
    ma, mb = a.mean(), b.mean()
    assert abs(ma - mb) <= 0.01 * ma, (ma, mb)


@pytest.mark.parametrize("which", ["C2_cornell_box", "C4b_volume_test", "coverage"])
def test_no_bias(which):
    if which == "coverage":
        scene, r = _coverage_scene()
    elif which == "C2_cornell_box":
        scene, r = scenes.config(which, 128, 128, 64)
    else:
        scene, r = scenes.config(which, 128, 72, 32)
    _bias_case(scene, r)


# ---- 5. less noise ---------------------------------------------------------------------------------------------------------------------
def test_less_noise_cornell():
    scene, r = scenes.config("C2_cornell_box", 256, 256, 64)
    ds = _lib.DeviceScene(scene.to_desc())
    ref = ds.render(_ls(r, False, samples=4096, seed=99)).linear.astype(np.float64)
    rm = lambda x: float(np.sqrt(np.mean((x.astype(np.float64) - ref) ** 2)))
    e_def, e_ls = rm(ds.render(r).linear), rm(ds.render(_ls(r)).linear)
    print(f"cornell 256x256 @64: RMSE default {e_def:.4g}, light sampling {e_ls:.4g}, ratio {e_ls / e_def:.3f}")
    assert e_ls <= 0.5 * e_def, (e_ls, e_def)


# ---- 6. composition --------------------------------------------------------------------------------------------------------------------
def test_composition():
    scene, r = scenes.config("C2_cornell_box", 64, 48, 64)
    ds = _lib.DeviceScene(scene.to_desc())
    rl = _ls(r)
    full = ds.render(rl)
    _same(full, ds.render(rl))                                  # a repeated call
    ids = np.random.default_rng(5).choice(64 * 48, 700, replace=False).astype(np.uint32)
    sub = ds.render(rl, pixel_ids=ids)                          # a pixel subset
    assert np.array_equal(sub.rgb8, full.rgb8[ids]) and np.array_equal(_u32(sub.linear), _u32(full.linear[ids]))
    accum = np.zeros((64 * 48, 4), np.float32)                 # progressive 4 x 16 = 64
    r16 = _ls(r, samples=16)
    for k in range(4):
        res = ds.render_progressive(r16, 16 * k, accum)
    _same(res, full)
    accum64 = np.zeros_like(accum)
    ds.render_progressive(rl, 0, accum64)
    assert np.array_equal(_u32(accum), _u32(accum64))
    rays = np.stack([ds.camera_rays(rl, s) for s in range(64)])   # caller rays = fw_render
    rr = ds.render_rays(rays, 64, seed=rl.settings["seed"], use_bvh=bool(rl.settings["use_bvh"]), flags=A.FW_FLAG_LIGHT_SAMPLING)
    assert np.array_equal(rr.rgb8, full.rgb8) and np.array_equal(_u32(rr.linear), _u32(full.linear))


def test_update_moves_light():
    scene, r = scenes.config("C2_cornell_box", 48, 48, 16)
    rl = _ls(r)
    ds = _lib.DeviceScene(scene.to_desc())
    ds.render(rl)
    (l,) = _lib.selftest_lights(scene.to_desc())
    scene.render_objects[l["obj"]].position(-60.0, -20.0, 40.0)
    ds.update(scene)
    fresh = _lib.DeviceScene(scene.to_desc())
    _same(ds.render(rl), fresh.render(rl))


# ---- 7. the other entry points ---------------------------------------------------------------------------------------------------------
def test_views_and_adaptive_honour_aovs_ignore():
    scene, r = scenes.config("C2_cornell_box", 32, 32, 16)
    rl = _ls(r)
    ds = _lib.DeviceScene(scene.to_desc())
    v = ds.render_views(rl, [r._camera])
    assert np.array_equal(v.rgb8.reshape(-1, 3), ds.render(rl).rgb8)
    ad = ds.render_adaptive(rl, 0.05, 8)
    assert np.isfinite(ad.linear).all()
    assert np.array_equal(_u32(ds.aovs(r, 4)), _u32(ds.aovs(rl, 4)))
