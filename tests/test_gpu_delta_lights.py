"""Point, spot and directional lights (fw_scene_set_lights) on the GPU.  Probes through fw_render_rays onto a Lambertian floor
equal the float64 restatement (tests/delta_lights_ref.py) within 1e-5 — fewer than 100 float32 roundings of 2^-24 each, 6e-6 — and are
exactly 0 outside a spot's cone; a sphere between light and floor shadows exactly, one beyond a point light does not, and under a
directional light it does; the paths are those of the frame without lights; without lights, or without a material that samples them, the
frames are bit for bit what they were; subsets, progressive passes, repeats, caller rays and fw_scene_update compose bit for bit; a point
light of I = Le pi r^2 agrees with a small emissive sphere under the validated estimator of §9g, multi-bounce transport included; the
frame is linear in its lights beside §9g's emitters; and what is out of scope or invalid is refused."""
import copy
import os
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, ColorEnv, DielectricMat, DirectionalLight, EmissiveMat, LambertianMat, MetalMat, PointLight,
                              Renderer, RenderObject, Scene, SpotLight, Sphere, XYRect, XZRect, YZRect)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_lights_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _with(r, **kw):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    for k, v in kw.items():
        getattr(rr, k)(v)
    return rr


def _same(a, b):
    assert np.array_equal(a.rgb8, b.rgb8)
    assert np.array_equal(_u32(a.gamma), _u32(b.gamma)) and np.array_equal(_u32(a.linear), _u32(b.linear))


# ---- 1. exact probes ------------------------------------------------------------------------------------------------------------------
ALB = (0.6, 0.5, 0.4)
UP = (0.0, 1.0, 0.0)
SAMPLES = 16
POINT = PointLight((0.3, 2.0, -0.2), (9.0, 6.0, 3.0))
# axis tilted off the vertical; inner 10 deg, outer 50 deg
SPOT = SpotLight((0.0, 3.0, 0.0), (0.2, -1.0, 0.1), (30.0, 20.0, 10.0), 10.0, 50.0)
SUN = DirectionalLight((0.3, -1.0, 0.2), (2.0, 1.5, 1.0))


def _floor_scene(blocker=None):
    """A Lambertian XZ rectangle of constant albedo under a black ColorEnv; blocker: (centre, radius) of a sphere that emits nothing and
    scatters nothing (a path that meets it ends black, so a probe's value is its light sample alone)"""
    scene = Scene.new()
    floor = scene.add_material(LambertianMat.with_color(ALB))
    scene.add_object(RenderObject.new(XZRect.new(-50, 50, -50, 50, 0, floor)))
    if blocker is not None:
        black = scene.add_material(EmissiveMat.with_color((0.0, 0.0, 0.0)))
        scene.add_object(RenderObject.new(Sphere.new(blocker[1], black)).position(*blocker[0]))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    return scene


def _probe_rays(points):
    return np.array([[p[0], 0.5, p[1], 0.0, -1.0, 0.0] for p in points], np.float32)


def _grid(xs, zs):
    return [(float(x), float(z)) for x in xs for z in zs]


def _probe(light, points, blocker=None):
    scene = _floor_scene(blocker)
    scene.add_light(light)
    ds = _lib.DeviceScene(scene.to_desc())
    return ds.render_rays(_probe_rays(points), SAMPLES, seed=7).linear


def _want(light, points):
    return np.array([R.contribution(light, (p[0], 0.0, p[1]), UP, ALB) for p in points])


def _check_exact(got, want):
    got = got.astype(np.float64)
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"probes: {len(want)} points, max relative error {err[want > 0].max():.3g}")
    assert np.all(err[want > 0] <= 1e-5), (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.all(got[want == 0] == 0.0)


# 83 points, one right under the point light and one far out.  How far: §9g's scatter_pdf takes sqrt(c^2 - |n|^2 + 1), c = cos(theta), whose
# sum passes through values near 1: an absolute error e of about 2^-23 in c^2, hence 3 e / (4 c^2) relative in p_b = (2c)^3 / 4 pi.  That is
# 1.3e-6 at c = 0.26 (the far probe, 7.45 from the light's foot), inside the bound's budget, and unbounded towards grazing incidence (6e-5
# at c = 0.04) for this float32 form whatever the light, so no probe lies further out.
PROBE_POINTS = _grid(np.linspace(-3.1, 3.3, 9), np.linspace(-2.7, 2.9, 9)) + [(0.3, -0.2), (6.0, -5.0)]


def test_probe_point_light():
    want = _want(POINT, PROBE_POINTS)
    assert np.all(want > 0)
    _check_exact(_probe(POINT, PROBE_POINTS), want)


def test_probe_spot_light():
    """Probes inside the inner cone, in the falloff and outside the outer cone.  The smoothstep s(t), t = (c - cos_outer) / (cos_inner -
    cos_outer), turns a relative rounding error e of the cosine c into s'(t) c e / ((cos_inner - cos_outer) s(t)) of s, which grows without
    bound towards the outer edge (s -> 0) for any float32 evaluation.  So the falloff probes are those with t >= 0.3, where that factor is
    at most 1.26 x 0.75 / (0.342 x 0.216) = 13 and e of a few 2^-24 stays inside the bound's budget, and the probes meant to be inside or
    outside keep 1e-3 of cosine from their edge, far more than c's error.  Chosen from the geometry, before anything is rendered."""
    l = SPOT.to_abi()
    ci, co = float(l.cos_inner), float(l.cos_outer)
    pts, kinds = [], []
    near_axis = [(0.6, 0.3), (0.5, 0.2), (0.7, 0.45), (0.45, 0.4), (0.8, 0.3)]          # the axis meets the floor at (0.6, 0.3)
    for p in _grid(np.linspace(-6.0, 6.3, 13), np.linspace(-6.2, 6.0, 13)) + near_axis:
        c = R.spot_cosine(SPOT, (p[0], 0.0, p[1]))
        kind = "inner" if c >= ci + 1e-3 else "outside" if c <= co - 1e-3 else "falloff" if (c <= ci - 1e-3 and (c - co) / (ci - co) >= 0.3) else None
        if kind:
            pts.append(p)
            kinds.append(kind)
    kinds = np.array(kinds)
    assert (kinds == "inner").sum() >= 3 and (kinds == "falloff").sum() >= 10 and (kinds == "outside").sum() >= 20, kinds
    want = _want(SPOT, pts)
    full = _want(PointLight(SPOT.position, SPOT.intensity), pts)
    assert np.all(want[kinds == "inner"] == full[kinds == "inner"]) and np.all(want[kinds == "outside"] == 0)
    assert np.all((want[kinds == "falloff"] > 0) & (want[kinds == "falloff"] < full[kinds == "falloff"]))
    got = _probe(SPOT, pts)
    _check_exact(got, want)
    assert np.all(got[kinds == "outside"] == 0.0)


def test_probe_hard_edged_spot():
    spot = SpotLight((0.0, 2.0, 0.0), (0.0, -1.0, 0.0), (8.0, 8.0, 8.0), 45.0, 45.0)       # the edge at radius 2 on the floor
    pts = [(0.0, 0.0), (1.0, 1.0), (1.9, 0.0), (0.0, -1.95), (2.1, 0.0), (0.0, 2.05), (1.6, 1.6), (-3.0, 0.5)]
    want = _want(spot, pts)
    assert (want[:, 0] > 0).tolist() == [True, True, True, True, False, False, False, False]
    _check_exact(_probe(spot, pts), want)


def test_probe_directional_light():
    want = _want(SUN, PROBE_POINTS)
    assert np.all(want > 0) and np.all(want == want[0])
    _check_exact(_probe(SUN, PROBE_POINTS), want)


def test_probe_two_lights_pick_one_each_sample():
    """Two lights: each sample picks one with p = 1/2 and adds its contribution / p, so a probe's mean over n samples is
    2 (k A + (n - k) B) / n for the single-light values A, B and a whole number k of samples that picked the first; the picks are fair."""
    scene = _floor_scene()
    scene.add_light(POINT)
    scene.add_light(SUN)
    ds = _lib.DeviceScene(scene.to_desc())
    a, b = _want(POINT, PROBE_POINTS)[:, 0], _want(SUN, PROBE_POINTS)[:, 0]
    pts = [p for p, x, y in zip(PROBE_POINTS, a, b) if abs(x - y) > 0.1 * y][:64]          # (k is read off A - B)
    assert len(pts) >= 48
    a, b = _want(POINT, pts)[:, 0], _want(SUN, pts)[:, 0]
    got = ds.render_rays(_probe_rays(pts), SAMPLES, seed=7).linear[:, 0].astype(np.float64)
    k = (got - 2 * b) / (2 * (a - b)) * SAMPLES            # the number of samples that picked the point light
    assert np.all(np.abs(k - np.round(k)) < 1e-3) and np.all((np.round(k) >= 0) & (np.round(k) <= SAMPLES))
    assert 0.4 * SAMPLES <= k.mean() <= 0.6 * SAMPLES, k.mean()            # >= 768 fair picks: within 5 standard deviations of a half


# ---- 2. shadows -----------------------------------------------------------------------------------------------------------------------
def test_shadow_of_a_sphere_under_a_point_light():
    light = PointLight((0.0, 4.0, 0.0), (9.0, 6.0, 3.0))
    # sphere of radius 0.5 half-way: the umbra on the floor is the disc of radius 4 tan(asin(0.25)) = 1.033
    umbra = [(0.0, 0.0), (0.5, 0.3), (-0.7, 0.0), (0.0, 0.9), (-0.6, -0.6)]
    outside = [(1.5, 0.0), (0.0, -1.6), (2.0, 2.0), (-3.0, 1.0), (1.2, 1.2)]
    lit = _probe(light, umbra + outside)
    shadowed = _probe(light, umbra + outside, blocker=((0.0, 2.0, 0.0), 0.5))
    assert np.all(lit > 0)
    assert np.all(shadowed[:len(umbra)] == 0.0)
    assert np.array_equal(_u32(shadowed[len(umbra):]), _u32(lit[len(umbra):]))


def test_sphere_beyond_a_point_light_shadows_nothing_but_does_under_a_directional_light():
    pts = [(0.0, 0.0), (0.2, 0.1), (-0.3, 0.2), (0.0, -0.4), (1.0, 0.0), (0.0, 1.5), (-2.0, 2.0)]
    blocker = ((0.0, 4.0, 0.0), 0.5)                       # above the light: t > 1 on every shadow ray
    light = PointLight((0.0, 2.0, 0.0), (9.0, 6.0, 3.0))
    lit = _probe(light, pts)
    assert np.all(lit > 0)
    assert np.array_equal(_u32(_probe(light, pts, blocker)), _u32(lit))
    sun = DirectionalLight((0.0, -1.0, 0.0), (2.0, 1.5, 1.0))
    lit, shadowed = _probe(sun, pts), _probe(sun, pts, blocker)
    assert np.all(lit > 0)
    assert np.all(shadowed[:4] == 0.0)                     # within 0.5 of the axis: the sphere hides the sun
    assert np.array_equal(_u32(shadowed[4:]), _u32(lit[4:]))


# ---- 3. the same paths ----------------------------------------------------------------------------------------------------------------
CORNELL_POINT = PointLight((278.0, 400.0, 278.0), (60000.0, 50000.0, 40000.0))
CORNELL_LIGHTS = [CORNELL_POINT, SpotLight((100.0, 500.0, 100.0), (0.3, -1.0, 0.4), (90000.0, 90000.0, 90000.0), 25.0, 50.0),
                  DirectionalLight((0.2, -1.0, 0.6), (1.0, 0.9, 0.8))]


@pytest.mark.parametrize("which", ["cornell", "mesh_bvh"])
def test_same_paths(which):
    if which == "cornell":
        scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
        lights = CORNELL_LIGHTS
    else:
        scene, r = scenes.config("C3_suzanne", 64, 64, 16)
        r.use_bvh(True)
        lights = [PointLight((2.0, 4.0, 3.0), (40.0, 40.0, 40.0)), DirectionalLight((0.3, -1.0, -0.2), (1.0, 1.0, 1.0))]
    ds = _lib.DeviceScene(scene.to_desc())
    a = ds.render(r)
    ds.set_lights(lights)
    b = ds.render(r)
    assert a.stats["rays"] == b.stats["rays"]
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in b.stats["rays_per_depth"]]
    assert b.linear.astype(np.float64).mean() > 1.05 * a.linear.astype(np.float64).mean()      # (the lights are on)
    c = ds.render(_with(r, light_sampling=True))           # beside §9g's emitters as well
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in c.stats["rays_per_depth"]]


# ---- 4. off means off -----------------------------------------------------------------------------------------------------------------
def test_removed_lights_leave_the_frame_of_a_fresh_scene():
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    fresh = _lib.DeviceScene(scene.to_desc())
    ds = _lib.DeviceScene(scene.to_desc())
    ds.set_lights(CORNELL_LIGHTS)
    lit = ds.render(r)
    ds.set_lights([])
    for rr in (r, _with(r, light_sampling=True)):
        _same(ds.render(rr), fresh.render(rr))
    assert not np.array_equal(lit.linear, fresh.render(r).linear)
    lib = _lib.load()
    ds.set_lights(CORNELL_LIGHTS)
    assert lib.fw_scene_set_lights(ds.handle, None, 0) == A.FW_OK            # NULL, 0 as the header allows
    _same(ds.render(r), fresh.render(r))


def test_no_sampling_material_renders_the_default_frame():
    scene = Scene.new()
    metal = scene.add_material(MetalMat.new((0.8, 0.7, 0.6), 0.1))
    glass = scene.add_material(DielectricMat.new(1.5))
    light = scene.add_material(EmissiveMat.with_color((5.0, 5.0, 5.0)))
    scene.add_object(RenderObject.new(XZRect.new(-20, 20, -20, 20, 0, metal)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, glass)).position(0.0, 1.0, 0.0))
    scene.add_object(RenderObject.new(XZRect.new(-2, 2, -2, 2, 5, light)))
    cam = CameraSettings.default().cam_pos((0.0, 3.0, 8.0)).look_at((0.0, 1.0, 0.0)).field_of_view(50.0)
    r = Renderer.default().width(64).height(64).samples(16).use_bvh(True).camera(cam)
    plain = _lib.DeviceScene(scene.to_desc()).render(r)
    scene.add_light(PointLight((0.0, 4.0, 0.0), (50.0, 50.0, 50.0)))
    scene.add_light(DirectionalLight((0.0, -1.0, 0.0), (1.0, 1.0, 1.0)))
    ds = _lib.DeviceScene(scene.to_desc())
    _same(ds.render(r), plain)
    _same(ds.render(_with(r, env_sampling=True)), plain)           # (the lights are not active: nothing to refuse)


def test_aovs_ignore_lights():
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    before = ds.aovs(r, 4)
    ds.set_lights(CORNELL_LIGHTS)
    assert np.array_equal(_u32(ds.aovs(r, 4)), _u32(before))


# ---- 5. composition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [False, True])
def test_composition(ls):
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    for l in CORNELL_LIGHTS:
        scene.add_light(l)
    r = _with(r, light_sampling=ls)
    ds = _lib.DeviceScene(scene.to_desc())
    full = ds.render(r)
    _same(full, ds.render(r))                                   # a repeated call
    ids = np.random.default_rng(5).choice(64 * 64, 700, replace=False).astype(np.uint32)
    sub = ds.render(r, pixel_ids=ids)                           # a pixel subset
    assert np.array_equal(sub.rgb8, full.rgb8[ids]) and np.array_equal(_u32(sub.linear), _u32(full.linear[ids]))
    accum = np.zeros((64 * 64, 4), np.float32)                 # progressive 4 x 4 = 16
    r4 = _with(r, samples=4)
    for k in range(4):
        res = ds.render_progressive(r4, 4 * k, accum)
    _same(res, full)
    accum16 = np.zeros_like(accum)
    ds.render_progressive(r, 0, accum16)
    assert np.array_equal(_u32(accum), _u32(accum16))
    rays = np.stack([ds.camera_rays(r, s) for s in range(16)])   # caller rays = fw_render
    rr = ds.render_rays(rays, 16, seed=r.settings["seed"], use_bvh=bool(r.settings["use_bvh"]), flags=A.FW_FLAG_LIGHT_SAMPLING if ls else 0)
    assert np.array_equal(rr.rgb8, full.rgb8) and np.array_equal(_u32(rr.linear), _u32(full.linear))


def test_update_keeps_the_lights():
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    for l in CORNELL_LIGHTS:
        scene.add_light(l)
    ds = _lib.DeviceScene(scene.to_desc())
    before = ds.render(r)
    scene.render_objects[6].position(160.0, 0.0, 90.0)          # the short box
    lib = _lib.load()
    desc = ds._desc.placements(scene)
    assert lib.fw_scene_update(ds.handle, desc.ptr()) == A.FW_OK            # the C call alone: no light is set again
    fresh = _lib.DeviceScene(scene.to_desc())                               # create + set
    after = ds.render(r)
    _same(after, fresh.render(r))
    assert not np.array_equal(after.linear, before.linear)
    plain, _ = scenes.config("C2_cornell_box", 64, 64, 16)
    plain.render_objects[6].position(160.0, 0.0, 90.0)
    assert not np.array_equal(after.linear, _lib.DeviceScene(plain.to_desc()).render(r).linear)      # (the lights are still on)


def test_views_adaptive_and_model_frames_honour_the_lights():
    """The other entry points whose frames go through the same path: one view equals fw_render, an adaptive frame whose minimum is its cap
    equals fw_render, and fw_render_model equals fw_render_rays over the model's rays; each differs from the scene without lights."""
    from firework_amd.api import CameraModel
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    dark = _lib.DeviceScene(scene.to_desc())
    for l in CORNELL_LIGHTS:
        scene.add_light(l)
    ds = _lib.DeviceScene(scene.to_desc())
    full = ds.render(r)
    v = ds.render_views(r, [r._camera])
    assert np.array_equal(v.rgb8.reshape(-1, 3), full.rgb8) and np.array_equal(_u32(v.linear_rgb.reshape(-1, 3)), _u32(full.linear))
    ad = ds.render_adaptive(r, 0.05, 16)
    assert np.array_equal(_u32(ad.linear), _u32(full.linear))
    model = CameraModel.panorama((278.0, 278.0, 278.0), 64, 32)
    m = ds.render_model(model, 4, seed=3, use_bvh=False)
    rays = _lib.model_rays(model, 0, 4)
    rr = ds.render_rays(rays, 4, seed=3, use_bvh=False)
    assert np.array_equal(_u32(m.linear), _u32(rr.linear))
    assert not np.array_equal(m.linear, dark.render_model(model, 4, seed=3, use_bvh=False).linear)
    assert not np.array_equal(full.linear, dark.render(r).linear)


# ---- 6. against the validated estimator -----------------------------------------------------------------------------------------------
def _blocks(img, W, H):
    lum = img.reshape(H, W, 3).astype(np.float64).mean(-1)
    return lum.reshape(H // 16, 16, W // 16, 16).mean((1, 3))


def _room(sphere):
    H, T = R.ROOM_HALF, R.ROOM_HEIGHT
    scene = Scene.new()
    white = scene.add_material(LambertianMat.with_color((0.7, 0.7, 0.7)))
    red = scene.add_material(LambertianMat.with_color((0.6, 0.2, 0.2)))
    blue = scene.add_material(LambertianMat.with_color((0.2, 0.3, 0.6)))
    scene.add_object(RenderObject.new(XZRect.new(-H, H, -H, H, 0.0, white)))
    scene.add_object(RenderObject.new(XZRect.new(-H, H, -H, H, T, white)).flip_normals())
    scene.add_object(RenderObject.new(YZRect.new(0.0, T, -H, H, -H, red)))
    scene.add_object(RenderObject.new(YZRect.new(0.0, T, -H, H, H, blue)).flip_normals())
    scene.add_object(RenderObject.new(XYRect.new(-H, H, 0.0, T, -H, white)))
    scene.add_object(RenderObject.new(XYRect.new(-H, H, 0.0, T, H, white)).flip_normals())
    if sphere:
        emit = scene.add_material(EmissiveMat.with_color((R.ROOM_LE,) * 3))
        scene.add_object(RenderObject.new(Sphere.new(R.ROOM_R, emit)).position(*R.ROOM_LIGHT))
    else:
        scene.add_light(PointLight(R.ROOM_LIGHT, (R.ROOM_LE * np.pi * R.ROOM_R ** 2,) * 3))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    cam = CameraSettings.default().cam_pos((0.0, 3.0, 2.8)).look_at((0.0, 3.0, 0.0)).field_of_view(60.0)
    return scene, Renderer.default().width(64).height(64).samples(64).use_bvh(True).camera(cam)


def test_point_light_agrees_with_a_small_emissive_sphere():
    seeds = 8
    s_sphere, r = _room(True)
    s_point, _ = _room(False)
    ds_s, ds_p = _lib.DeviceScene(s_sphere.to_desc()), _lib.DeviceScene(s_point.to_desc())
    rs = _with(r, light_sampling=True)
    a = np.stack([_blocks(ds_s.render(_with(rs, seed=s)).linear, 64, 64) for s in range(seeds)])
    b = np.stack([_blocks(ds_p.render(_with(r, seed=s)).linear, 64, 64) for s in range(seeds)])
    # the one block that holds the sphere's image (Le = 8000 against a room of order 1) is left out
    keep = np.ones((4, 4), bool)
    keep[np.unravel_index(a.mean(0).argmax(), (4, 4))] = False
    ma, mb = a.mean(0), b.mean(0)
    se = np.sqrt((a.var(0, ddof=1) + b.var(0, ddof=1)) / seeds)
    bound = 4.0 * se + 1e-4 * mb                           # the far-field term (r / d)^2 <= 1e-4, relative
    z = np.abs(ma - mb) / bound
    print("sphere blocks", np.array2string(ma, precision=4), "point blocks", np.array2string(mb, precision=4), "|diff| / bound",
          np.array2string(z, precision=2))
    assert mb[keep].min() > 0.01                           # (the room is lit, multi-bounce included: the ceiling block sees no light directly)
    assert np.all(z[keep] <= 1.0), (z, keep)


# ---- 7. linearity with emitters ---------------------------------------------------------------------------------------------------------
def test_linear_beside_the_cornell_light():
    seeds = 8
    scene, r = scenes.config("C2_cornell_box", 64, 64, 64)
    rl = _with(r, light_sampling=True)
    ds_both = _lib.DeviceScene(scene.to_desc())
    ds_both.set_lights([CORNELL_POINT])
    ds_cornell = _lib.DeviceScene(scene.to_desc())
    dark, _ = scenes.config("C2_cornell_box", 64, 64, 64)
    dark.materials[3] = LambertianMat.with_color((0.0, 0.0, 0.0))          # the light's material
    assert isinstance(scene.materials[3], EmissiveMat)
    ds_point = _lib.DeviceScene(dark.to_desc())
    ds_point.set_lights([CORNELL_POINT])
    both = np.stack([_blocks(ds_both.render(_with(rl, seed=s)).linear, 64, 64) for s in range(seeds)])
    corn = np.stack([_blocks(ds_cornell.render(_with(rl, seed=s)).linear, 64, 64) for s in range(seeds)])
    pnt = np.stack([_blocks(ds_point.render(_with(r, seed=s)).linear, 64, 64) for s in range(seeds)])
    sigma = np.sqrt((both.var(0, ddof=1) + corn.var(0, ddof=1) + pnt.var(0, ddof=1)) / seeds)
    z = np.abs(both.mean(0) - corn.mean(0) - pnt.mean(0)) / np.maximum(sigma, 1e-12)
    print("both", np.array2string(both.mean(0), precision=4), "cornell", np.array2string(corn.mean(0), precision=4), "point",
          np.array2string(pnt.mean(0), precision=4), "z", np.array2string(z, precision=2))
    assert pnt.mean() > 0.1 * corn.mean()                  # (the point light matters in the sum)
    assert z.max() <= 4.0, (z.max(), np.unravel_index(z.argmax(), z.shape))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_flags_are_refused():
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    ds.set_lights([CORNELL_POINT])
    good = ds.render(r)
    for rr in (_with(r, env_sampling=True), _with(r, light_sampling=True, all_emitters=True)):
        assert rr.to_params().flags & (A.FW_FLAG_ENV_SAMPLING | A.FW_FLAG_ALL_EMITTERS)
        with pytest.raises(_lib.FireworkError) as e:
            ds.render(rr)
        assert e.value.status == A.FW_ERR_UNSUPPORTED and "lights" in str(e.value)
    rays = np.stack([ds.camera_rays(r, s) for s in range(2)])
    for flags in (A.FW_FLAG_ENV_SAMPLING, A.FW_FLAG_ALL_EMITTERS, A.FW_FLAG_LIGHT_SAMPLING | A.FW_FLAG_ALL_EMITTERS):
        with pytest.raises(_lib.FireworkError) as e:
            ds.render_rays(rays, 2, flags=flags)
        assert e.value.status == A.FW_ERR_UNSUPPORTED
    _same(ds.render(r), good)


def test_invalid_lights_leave_the_scene_as_it_was():
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    ds.set_lights(CORNELL_LIGHTS)
    good = ds.render(r)
    bad = [CORNELL_POINT.to_abi(), A.fw_light(A.FW_LIGHT_SPOT, A.vec3((0, 1, 0)), A.vec3((0, 0, 0)), A.vec3((1, 1, 1)), 0.9, 0.8)]
    with pytest.raises(_lib.FireworkError) as e:
        ds.set_lights(bad)
    assert e.value.status == A.FW_ERR_BAD_ARG and "lights[1]" in str(e.value)
    with pytest.raises(_lib.FireworkError):
        ds.set_lights([PointLight((0, 1, 0), (1.0, float("nan"), 1.0))])
    _same(ds.render(r), good)
