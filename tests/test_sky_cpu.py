"""CPU-side checks of the SunSky environment (fw_check_sky, fw_sky_map, fw_sky_radiance, fw_sky_sun): the exports and
their ctypes signatures against the header, fw_sky's layout against the C compiler's; every argument error of the calls in the header's
order (they come before HIP is called), and the no-device error with the caller's buffers untouched; fw_sky_sun, which is host code,
against api.sky_sun; the properties of the numpy statement — the colours of noon and sunset, linearity in E0, turbidity 0, the symmetry
about the sun's azimuth, the disc's energy at every resolution and through its fallback, the convergence of the default step counts;
and the host plumbing: SunSkyEnv in a Scene, its YAML form, scenes/sun_sky.yml, the CLI's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, yaml_io
from firework_amd.api import DirectionalLight, PointLight, Scene, SunSky, SunSkyEnv

import env_dist_ref as ED
import sky_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- exports and layout ---------------------------------------------------------------------------------------------------------------
def _ctype_of(param):
    param = param.strip()
    if "*" in param:
        for name, t in (("fw_sky", A.fw_sky), ("fw_light", A.fw_light)):
            if re.search(rf"\b{name}\b", param):
                return C.POINTER(t)
        return C.c_void_p
    if param.startswith("uint32_t"):
        return C.c_uint32
    assert param.startswith("int "), param
    return C.c_int


def test_exports_and_signatures_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.SKY_PROTOTYPES) == ["fw_check_sky", "fw_sky_map", "fw_sky_radiance", "fw_sky_sun"]
    for name, argtypes in A.SKY_PROTOTYPES.items():
        assert hasattr(lib, name), name
        found = re.findall(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert len(found) == 1, name
        want = [_ctype_of(p) for p in found[0].replace("\n", " ").split(",")]
        assert argtypes == want, (name, argtypes, want)
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == C.c_int
    assert re.search(r"#define FW_SKY_DISC 1u", text) and A.FW_SKY_DISC == 1


def test_struct_layout(tmp_path):
    """ctypes' fw_sky equals the C compiler's, size and every field offset"""
    names = ["sun_elevation", "sun_azimuth", "turbidity", "sun_irradiance", "sun_radius", "altitude", "ground_albedo", "view_steps", "light_steps",
             "sun_samples", "flags"]
    assert [f for f, _ in A.fw_sky._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 1) + '\\n",sizeof(fw_sky)' +
           "".join(f",offsetof(fw_sky,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_sky)] + [getattr(A.fw_sky, f).offset for f in names]
    a = SunSky(35.0, 60.0).to_abi()
    assert (a.turbidity, a.sun_radius, a.altitude, a.view_steps, a.light_steps, a.sun_samples, a.flags) == (1.0, float(np.float32(0.00465)), 1.0, 32, 16, 8, 0)
    assert (a.sun_irradiance.x, a.sun_irradiance.y, a.sun_irradiance.z) == (5.0, 5.0, 5.0)
    assert a.sun_elevation == float(np.float32(np.radians(35.0))) and a.sun_azimuth == float(np.float32(np.radians(60.0)))
    assert SunSky(35.0, 60.0).to_abi(disc=True).flags == A.FW_SKY_DISC


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def _s(**kw):
    s = SunSky(35.0, 60.0).to_abi()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# the header's order: each entry is broken in its own field and in every later one, and must be reported for its own
BAD_SKIES = [("sun_elevation", dict(sun_elevation=1.6)), ("sun_elevation", dict(sun_elevation=NAN)), ("sun_azimuth", dict(sun_azimuth=INF)),
             ("turbidity", dict(turbidity=-0.5)), ("turbidity", dict(turbidity=65.0)), ("turbidity", dict(turbidity=NAN)),
             ("sun_irradiance", dict(sun_irradiance=A.vec3((1.0, -1.0, 1.0)))), ("sun_irradiance", dict(sun_irradiance=A.vec3((1.0, 1.0, INF)))),
             ("sun_radius", dict(sun_radius=0.0)), ("sun_radius", dict(sun_radius=0.11)), ("sun_radius", dict(sun_radius=NAN)),
             ("altitude", dict(altitude=0.5)), ("altitude", dict(altitude=50001.0)), ("altitude", dict(altitude=NAN)),
             ("ground_albedo", dict(ground_albedo=A.vec3((0.5, 1.5, 0.5)))), ("ground_albedo", dict(ground_albedo=A.vec3((NAN, 0.5, 0.5)))),
             ("view_steps", dict(view_steps=0)), ("view_steps", dict(view_steps=65)), ("light_steps", dict(light_steps=0)),
             ("light_steps", dict(light_steps=33)), ("sun_samples", dict(sun_samples=0)), ("sun_samples", dict(sun_samples=17)),
             ("flags", dict(flags=2))]


def _said(lib, st, word):
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _order_inside_the_description(lib, call):
    for i, (word, kw) in enumerate(BAD_SKIES):
        assert _said(lib, call(_s(**kw)), word) == A.FW_ERR_BAD_ARG, (word, kw)
        later = {}
        for _, k in BAD_SKIES[i + 1:]:
            later.update(k)
        later.update(kw)
        assert _said(lib, call(_s(**later)), word) == A.FW_ERR_BAD_ARG, ("before every later field", word)
    for ok in (dict(sun_elevation=float(np.float32(np.pi / 2))), dict(sun_elevation=-float(np.float32(np.pi / 2))), dict(turbidity=0.0),
               dict(turbidity=64.0), dict(sun_radius=float(np.float32(0.1))), dict(altitude=50000.0), dict(view_steps=64, light_steps=32, sun_samples=16)):
        assert lib.fw_check_sky(C.byref(_s(**ok))) == A.FW_OK, ok


def test_check_sky():
    lib = _lib.load()
    assert _said(lib, lib.fw_check_sky(None), "null") == A.FW_ERR_BAD_ARG
    _order_inside_the_description(lib, lambda s: lib.fw_check_sky(C.byref(s)))
    assert lib.fw_check_sky(C.byref(_s())) == A.FW_OK
    with pytest.raises(_lib.FireworkError, match="turbidity"):
        _lib.check_sky(_s(turbidity=99.0))
    for kw, word in ((dict(elevation_deg=91.0), "elevation"), (dict(turbidity=65.0), "turbidity"), (dict(sun_irradiance=(1, -1, 1)), "sun_irradiance"),
                     (dict(sun_radius=0.2), "sun_radius"), (dict(altitude=0.0), "altitude"), (dict(ground_albedo=(2, 0, 0)), "ground_albedo"),
                     (dict(view_steps=65), "view_steps"), (dict(light_steps=0), "light_steps"), (dict(sun_samples=17), "sun_samples")):
        args = dict(elevation_deg=35.0, azimuth_deg=60.0)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            SunSky(**args).check()


def test_sky_map_argument_checks():
    lib = _lib.load()
    rgb = np.full((4, 8, 3), 7.0, np.float32)

    def call(s=None, w=8, h=4, device=0, on_device=0, null_s=False, out=rgb.ctypes.data):
        return lib.fw_sky_map(None if null_s else C.byref(s if s is not None else _s()), device, w, h, out, on_device, None)

    assert _said(lib, call(null_s=True), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_s(turbidity=99.0), out=None), "null") == A.FW_ERR_BAD_ARG                    # NULL before the description
    _order_inside_the_description(lib, lambda s: call(s, w=1))                                           # the description before the size
    for w, h in ((1, 4), (8, 1), (0, 0)):
        assert _said(lib, call(w=w, h=h), "width and height") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(w=1, on_device=1, out=C.c_void_p(rgb.ctypes.data + 2)), "width and height") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(on_device=1, out=C.c_void_p(rgb.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(w=1 << 16, h=1 << 15, on_device=1, out=C.c_void_p(rgb.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(w=1 << 16, h=1 << 15), "must be below") == A.FW_ERR_UNSUPPORTED               # W H = 2^31
    assert _said(lib, call(w=1 << 16, h=1 << 15, device=-1), "must be below") == A.FW_ERR_UNSUPPORTED    # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(rgb == 7.0)
        with pytest.raises(_lib.FireworkError) as e:
            _lib.sky_map(SunSky(35.0, 60.0), 8, 4)
        assert e.value.status == A.FW_ERR_NO_DEVICE
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG
        assert np.all(rgb == 7.0)


def test_sky_radiance_argument_checks():
    lib = _lib.load()
    dirs, rgb = np.full((4, 6), 7.0, np.float32), np.full((4, 3), 7.0, np.float32)

    def call(s=None, n=4, stride=6, device=0, on_device=0, null_s=False, d=dirs.ctypes.data, out=rgb.ctypes.data):
        return lib.fw_sky_radiance(None if null_s else C.byref(s if s is not None else _s()), device, n, d, stride, out, on_device, None)

    assert _said(lib, call(null_s=True), "null") == A.FW_ERR_BAD_ARG
    for kw in (dict(d=None), dict(out=None)):
        assert _said(lib, call(_s(turbidity=99.0), **kw), "null") == A.FW_ERR_BAD_ARG
    _order_inside_the_description(lib, lambda s: call(s, n=0))
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, on_device=1, d=C.c_void_p(dirs.ctypes.data + 2)), "stride_floats") == A.FW_ERR_BAD_ARG
    for kw in (dict(d=C.c_void_p(dirs.ctypes.data + 2)), dict(out=C.c_void_p(rgb.ctypes.data + 2))):
        assert _said(lib, call(on_device=1, **kw), "aligned") == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(stride=3) == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(rgb == 7.0) and np.all(dirs == 7.0)
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG
        assert np.all(rgb == 7.0)


# ---- fw_sky_sun: host code ------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("elevation", [89.5, 60.0, 35.0, 10.0, 2.0, -3.0])
@pytest.mark.parametrize("altitude", [1.0, 3000.0])
def test_sky_sun(elevation, altitude):
    lib = _lib.load()
    sky = R.sky(elevation, altitude)
    out = A.fw_light()
    out.cos_inner = 7.0
    assert _said(lib, lib.fw_sky_sun(None, C.byref(out)), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, lib.fw_sky_sun(C.byref(_s(turbidity=99.0)), None), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, lib.fw_sky_sun(C.byref(_s(turbidity=99.0)), C.byref(out)), "turbidity") == A.FW_ERR_BAD_ARG and out.cos_inner == 7.0
    light = _lib.sky_sun(sky)
    direction, irradiance = api.sky_sun(sky)
    got_d, got_e = [light.direction.x, light.direction.y, light.direction.z], [light.intensity.x, light.intensity.y, light.intensity.z]
    assert light.kind == A.FW_LIGHT_DIRECTIONAL and (light.cos_inner, light.cos_outer, light.position.x, light.position.y, light.position.z) == (0,) * 5
    assert np.all(_ulps(got_d, direction) <= 1) and np.all(_ulps(got_e, irradiance) <= 1), (got_d, direction, got_e, irradiance)
    assert np.all(_ulps(direction, (-sky.sun_direction()).astype(np.float32)) == 0)
    assert abs(float(np.linalg.norm(sky.sun_direction())) - 1.0) < 1e-15
    if elevation < 0:
        assert got_e == [0.0, 0.0, 0.0] and np.all(irradiance == 0)
    else:
        assert np.all(irradiance > 0) and irradiance[0] > irradiance[1] > irradiance[2]                  # blue is scattered out the most
        assert np.all(irradiance < sky.sun_irradiance)
        assert lib.fw_check_lights(C.byref(light), 1) == A.FW_OK
    sl = sky.sun_light()
    assert isinstance(sl, DirectionalLight) and np.array_equal(sl.direction, direction) and np.array_equal(sl.irradiance, irradiance)


# ---- properties of the statement ------------------------------------------------------------------------------------------------------
def _lum(rgb):
    return float(np.sum(rgb))


def test_noon_is_blue_and_sunset_is_red():
    noon, low = SunSky(60.0, 40.0), SunSky(2.0, 40.0)
    zen_noon, zen_low = api.sky_map(noon, 64, 32)[0, 0], api.sky_map(low, 64, 32)[0, 0]
    assert zen_noon[2] > zen_noon[1] > zen_noon[0] > 0, zen_noon
    t = api.sky_env_texel(low.sun_direction(), 64, 32)
    at_sun = api.sky_map(low, 64, 32).reshape(-1, 3)[t]
    assert at_sun[0] > at_sun[1] > at_sun[2] > 0, at_sun
    assert _lum(zen_low) < _lum(zen_noon)
    print(f"zenith at 60 deg {zen_noon}, at 2 deg {zen_low}; the sun's texel at 2 deg {at_sun}")


def _upward(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.02
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)


def test_linear_in_e0_and_turbidity_zero_has_no_mie_term(monkeypatch):
    d = np.concatenate([_upward(40, 3), -_upward(10, 4)])
    base = SunSky(25.0, 40.0, sun_irradiance=(1.0, 2.0, 4.0))
    twice = SunSky(25.0, 40.0, sun_irradiance=(2.0, 4.0, 8.0))
    a, b = api.sky_radiance(base, d, disc=True), api.sky_radiance(twice, d, disc=True)
    assert np.array_equal(b, np.float32(2.0) * a)                                                   # a power of two: exact in every product
    assert np.array_equal(api.sky_map(twice, 16, 8, disc=True), np.float32(2.0) * api.sky_map(base, 16, 8, disc=True))
    assert np.array_equal(np.float32(2.0) * api.sky_sun(base)[1], api.sky_sun(twice)[1])
    # turbidity 0: beta_M = 0 exactly, so tau has no Mie part and the Mie sum is multiplied by 0 — the Mie phase function, whatever its
    # g, changes no bit — while any haze at all changes the sky
    clear = SunSky(25.0, 40.0, turbidity=0.0)
    k = api._sky_constants(clear)
    assert k["beta_m"] == 0.0 and k["beta_me"] == 0.0
    L = api.sky_radiance(clear, d, disc=True)
    monkeypatch.setattr(api, "SKY_G", 0.3)
    assert np.array_equal(api.sky_radiance(clear, d, disc=True), L)
    assert not np.array_equal(api.sky_radiance(base, d, disc=True), a)
    monkeypatch.undo()
    assert np.all(L[:40] > 0) and np.all(np.isfinite(L))
    assert not np.array_equal(api.sky_radiance(SunSky(25.0, 40.0, turbidity=0.01), d, disc=True), L)


def test_symmetric_about_the_suns_azimuth():
    """azimuth 0 puts the sun at phi = 0, the map's centre column boundary: texel x mirrors texel W - 1 - x"""
    sky = SunSky(20.0, 0.0)
    m = api.sky_map(sky, 32, 16).astype(np.float64)
    assert np.all(np.abs(m - m[:, ::-1]) <= 2.0 ** -22 * np.abs(m))
    # a quarter turn moves the map by W / 4 columns; float32(pi / 2) is 4.4e-8 off, and ln L changes by less than 100 per radian
    rot = api.sky_map(SunSky(20.0, 90.0), 32, 16).astype(np.float64)
    assert np.all(np.abs(np.roll(rot, 8, axis=1) - m) <= 1e-5 * np.abs(m))


@pytest.mark.parametrize("size", [(8, 4), (64, 32), (256, 128), (1024, 512)])
@pytest.mark.parametrize("elevation", [60.0, 2.0])
def test_disc_energy_is_the_suns_at_every_resolution(size, elevation):
    w, h = size
    sky = R.sky(elevation)
    ids, gain, area = api.sky_disc(sky, w, h)
    omega = ED.omega_row(w, h)
    assert np.all(np.abs(api.sky_omega_row(w, h) - omega) <= 4 * R.EPS * np.abs(omega).max())
    k = api._sky_constants(sky)
    et = k["e0"] * api._sky_transmittance(k, k["O"])[0]
    energy = (gain * omega[ids // w][:, None]).sum(0)
    assert np.all(np.abs(energy - et) <= 64 * R.EPS * et), (energy, et)
    cap = 2.0 * np.pi * (1.0 - k["cos_sr"])
    fallback = [int(ED.env_texel(k["s"][None, :], w, h)[0])]
    print(f"{w} x {h} at {elevation} deg: {len(ids)} texels, coverage sum / cap {area / cap:.4f}")
    if (w, h) == (8, 4):                                                                                # no sample of a 45-degree texel falls in the disc
        assert ids.tolist() == fallback and area == omega[ids[0] // w]
    elif (w, h) == (1024, 512):                                                                          # the raw coverage sum misses the cap; the gain does not
        assert len(ids) > 4 and 0.5 < area / cap < 1.5
    else:                                                                                                # one sample of one texel can be all there is
        assert len(ids) >= 1 and area > 0.0
    on, off = api.sky_map(sky, w, h, disc=True, texels=ids).astype(np.float64), api.sky_map(sky, w, h, disc=False, texels=ids).astype(np.float64)
    assert np.all(np.abs((on - off) - gain) <= 2.0 ** -22 * on)
    below = api.sky_disc(R.sky(-3.0), w, h)
    assert below[0].size == 0 and below[2] == 0.0


@pytest.mark.parametrize("elevation", [60.0, 10.0, 2.0])
def test_default_steps_are_within_3_percent_of_converged(elevation):
    """the statement at (32, 16) steps against itself at (512, 128) on 200 seeded upward directions"""
    d = _upward(200, 1)
    coarse = api.sky_radiance(SunSky(elevation, 57.3, view_steps=32, light_steps=16), d).astype(np.float64)
    k = api._sky_constants(SunSky(elevation, 57.3))
    k["nv"], k["nl"] = 512, 128                                                                       # past fw_sky's range: the statement alone
    dd = d.astype(np.float64)
    fine = api._sky_along(k, dd / np.sqrt(api._dot3(dd, dd))[:, None])
    miss = float(np.max(np.abs(coarse - fine) / fine))
    print(f"elevation {elevation}: (32, 16) steps miss (512, 128) by at most {100 * miss:.3f} %")
    assert miss <= 0.03, miss


# ---- host plumbing --------------------------------------------------------------------------------------------------------------------
def test_sun_sky_env_in_a_scene():
    sky = SunSky(35.0, 60.0)
    with pytest.raises(ValueError, match="sun must be"):
        SunSkyEnv(sky, 64, 32, "moon")
    with pytest.raises(ValueError, match="width and height"):
        SunSkyEnv(sky, 1, 32)
    with pytest.raises(ValueError, match="turbidity"):
        SunSkyEnv(SunSky(35.0, 60.0, turbidity=99.0))
    e = SunSkyEnv(sky)
    assert (e.width, e.height, e.sun) == (2048, 1024, "disc")
    scene = Scene()
    lamp = PointLight((0.0, 5.0, 0.0), (1.0, 1.0, 1.0))
    scene.add_light(lamp)
    scene.set_environment(SunSkyEnv(sky, 64, 32, "disc"))
    assert scene.lights == [lamp]
    scene.set_environment(SunSkyEnv(sky, 64, 32, "light"))
    assert len(scene.lights) == 2 and scene.lights[0] is lamp and isinstance(scene.lights[1], DirectionalLight)
    assert np.array_equal(scene.lights[1].irradiance, api.sky_sun(sky)[1])
    scene.set_environment(SunSkyEnv(SunSky(10.0, 60.0), 64, 32, "light"))                                # replaced, not duplicated
    assert len(scene.lights) == 2 and np.array_equal(scene.lights[1].irradiance, api.sky_sun(SunSky(10.0, 60.0))[1])
    scene.set_environment(api.ColorEnv((0.1, 0.1, 0.1)))
    assert scene.lights == [lamp]
    if _lib.device_count() == 0:                                                                         # the bake needs a device, and says so
        scene.add_material(api.LambertianMat(api.ConstantTexture((0.5, 0.5, 0.5))))
        scene.add_object(api.RenderObject(api.Sphere(1.0, 0)))
        scene.set_environment(SunSkyEnv(sky, 64, 32))
        with pytest.raises(_lib.FireworkError) as err:
            scene.to_desc()
        assert err.value.status == A.FW_ERR_NO_DEVICE


def test_yaml_round_trip(tmp_path):
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "sun_sky.yml"))                              # loads without a device
    e = scene.environment
    assert isinstance(e, SunSkyEnv) and (e.width, e.height, e.sun) == (512, 256, "disc") and scene.lights == []
    assert (e.sky.elevation_deg, e.sky.azimuth_deg, e.sky.turbidity, e.sky.view_steps, e.sky.light_steps, e.sky.sun_samples) == (35.0, 60.0, 1.0, 32, 16, 8)
    assert len(scene.render_objects) == 3 and [type(m).__name__ for m in scene.materials] == ["LambertianMat", "LambertianMat", "GgxMat"]
    sky = SunSky(12.5, -70.0, turbidity=2.5, sun_irradiance=(3.0, 2.5, 2.0), sun_radius=0.01, altitude=1200.0, ground_albedo=(0.1, 0.2, 0.3),
                 view_steps=24, light_steps=12, sun_samples=4)
    lamp = PointLight((0.0, 5.0, 0.0), (1.0, 1.0, 1.0))
    for sun, n_lights in (("disc", 1), ("light", 2), ("none", 1)):
        scene.lights = []
        scene.add_light(lamp)
        scene.set_environment(SunSkyEnv(sky, 128, 64, sun))
        assert len(scene.lights) == n_lights
        d = yaml_io.scene_to_dict(scene)
        assert len(d["lights"]) == 1                                                                     # the sky's own sun is not written twice
        yaml_io.save_scene(scene, tmp_path / "s.yml")
        back = yaml_io.load_scene(tmp_path / "s.yml")
        b = back.environment
        assert isinstance(b, SunSkyEnv) and (b.width, b.height, b.sun) == (128, 64, sun) and len(back.lights) == n_lights
        assert bytes(b.sky.to_abi()) == bytes(sky.to_abi())
        assert yaml_io.scene_to_dict(back) == d
    minimal = yaml_io._environment({"environment": "SunSkyEnv", "sky": {"elevation_deg": 5, "azimuth_deg": 10}})
    assert bytes(minimal.sky.to_abi()) == bytes(SunSky(5.0, 10.0).to_abi()) and (minimal.width, minimal.height, minimal.sun) == (2048, 1024, "disc")


@pytest.mark.parametrize("args, word", [
    (["--sun-sky", "35,60", "--sun", "light", "--env-sampling"], "--env-sampling"),
    (["--sun", "disc"], "--sun-sky"),
    (["--sun-sky-size", "64,32"], "--sun-sky"),
    (["--sun-sky", "35"], "EL,AZ"),
    (["--sun-sky", "95,0"], "EL,AZ"),
    (["--sun-sky", "35,x"], "EL,AZ"),
    (["--sun-sky", "35,60,99"], "TURBIDITY"),
    (["--sun-sky", "35,60", "--sun-sky-size", "64"], "W,H"),
    (["--sun-sky", "35,60", "--sun-sky-size", "1,32"], "W,H"),
    (["--sun-sky", "35,60", "--sun", "moon"], "--sun"),
])
def test_cli_refusals_come_before_the_scene_is_read(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args
