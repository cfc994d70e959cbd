"""The SunSky environment on the GPU (fw_sky_map, fw_sky_radiance, SunSkyEnv).

k_sky_map and k_sky_sun against the numpy float64 statement (api.sky_map) within the bound of tests/sky_ref.py — derived from the order of
operations, nothing in it measured — over map sizes below, at and past a wave and a block, every step count's edge, suns from the zenith
to below the horizon, the disc off and on at three sample counts, two altitudes; every decision of the statement on those inputs is
asserted, on the CPU and before the device is asked, to lie outside the margins of tests/sky_ref.py.  Every map is compared texel by
texel (the statement of the largest, 256 x 128 at 64 / 32 steps, takes numpy a good second; each is computed once and shared), and
between the host and the device path bit for bit.  k_sky_dirs over every
count, stride and kind of direction; the disc's energy against fw_sky_sun's light; the map through the renderer's FW_ENV_HDR lookup bit
for bit; the sun as a light through fw_bake_direct; the CLI's round trip; fw_render left as it was."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes, yaml_io
from firework_amd.api import DirectLight, LambertianMat, RenderObject, Scene, Sphere, SunSky, SunSkyEnv

import env_dist_ref as ED
import sky_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SIZES = [(8, 4), (63, 31), (64, 32), (65, 33), (256, 128)]          # below a wave, a wave less one, a wave, a wave plus one, several blocks and rows
STEPS = [(1, 1), (3, 2), (32, 16), (64, 32)]                        # the smallest, odd ones, the defaults, the largest
ELEVATIONS = [89.5, 60.0, 10.0, 2.0, -3.0]
SAMPLES = [1, 4, 8]
ALTITUDES = [1.0, 3000.0]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case_sky(i_size, i_steps, i_el):
    """the sample count and the altitude cycle through the cases: every one meets every size, step count and elevation"""
    k = i_size + i_steps + i_el
    return R.sky(ELEVATIONS[i_el], ALTITUDES[k % 2], STEPS[i_steps], SAMPLES[(i_size + 2 * i_steps + i_el) % 3])


@functools.lru_cache(maxsize=None)
def _reference(i_size, i_steps, i_el):
    """(texel ids, statement without the disc, with it, bound without, with) — computed once, shared, never written to"""
    w, h = SIZES[i_size]
    sky = _case_sky(i_size, i_steps, i_el)
    terms = {}
    covered, gain, _ = api.sky_disc(sky, w, h, terms)
    ids = np.arange(w * h, dtype=np.int64)
    off = api.sky_map(sky, w, h, disc=False, texels=ids, terms=terms)
    what = f"{w}x{h} steps {STEPS[i_steps]} elevation {ELEVATIONS[i_el]}"
    R.assert_margins(terms, what)
    nv, nl = STEPS[i_steps]
    L = terms["radiance"].copy()
    extra = np.zeros_like(L)
    pos = np.searchsorted(ids, covered)
    if covered.size:
        L[pos] = L[pos] + gain
        extra[pos] = R.disc_bound(gain, R.k_common(terms["tau_max"], nv, nl), w, h, covered // w)
    on = L.astype(np.float32)
    for a in (ids, off, on, extra):
        a.setflags(write=False)
    return ids, off, on, terms, extra, what


CASES = [(a, b, c) for a in range(len(SIZES)) for b in range(len(STEPS)) for c in range(len(ELEVATIONS))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{SIZES[c[0]][0]}x{SIZES[c[0]][1]}-{STEPS[c[1]][0]}_{STEPS[c[1]][1]}-{ELEVATIONS[c[2]]}")
def test_map_against_the_statement(case):
    torch, dev = _torch()
    w, h = SIZES[case[0]]
    nv, nl = STEPS[case[1]]
    sky = _case_sky(*case)
    ids, ref_off, ref_on, terms, extra, what = _reference(*case)
    side = torch.cuda.Stream(dev)
    for disc, ref, more in ((False, ref_off, None), (True, ref_on, extra)):
        host = _lib.sky_map(sky.to_abi(disc=disc), w, h)
        out = torch.full((h, w, 3), NAN, dtype=torch.float32, device=dev)
        with torch.cuda.stream(side):
            _lib.sky_map(sky.to_abi(disc=disc), w, h, out=out, stream=side.cuda_stream)
        assert np.array_equal(_u32(host), _u32(out.cpu().numpy())), (what, disc)
        R.assert_close(host.reshape(-1, 3)[ids], ref, terms, nv, nl, f"{what} disc {disc} S {sky.sun_samples} altitude {sky.altitude}", more)
    if ELEVATIONS[case[2]] < 0:
        assert np.array_equal(ref_on, ref_off)                                                      # no disc below the horizon


def test_map_overwrites_and_repeats():
    """NaN-filled host and device outputs are overwritten whole; two runs are bit-equal; the disc's texels are the only ones that differ"""
    torch, dev = _torch()
    lib = _lib.load()
    for (w, h), el in (((65, 33), 10.0), ((256, 128), 60.0)):
        s = R.sky(el).to_abi(disc=True)
        runs = []
        for _ in range(2):
            host = np.full((h, w, 3), NAN, np.float32)
            assert lib.fw_sky_map(C.byref(s), 0, w, h, host.ctypes.data, 0, None) == A.FW_OK
            out = torch.full((h, w, 3), NAN, dtype=torch.float32, device=dev)
            _lib.sky_map(s, w, h, out=out)
            assert np.all(np.isfinite(host)) and np.array_equal(_u32(host), _u32(out.cpu().numpy()))
            runs.append(host)
        assert np.array_equal(_u32(runs[0]), _u32(runs[1]))
        s.flags = 0
        plain = _lib.sky_map(s, w, h)
        differs = np.nonzero(np.any(plain != runs[0], axis=2).reshape(-1))[0]
        assert np.array_equal(differs, np.sort(api.sky_disc(R.sky(el), w, h)[0]))


# ---- fw_sky_radiance ------------------------------------------------------------------------------------------------------------------
def _directions(n, seed):
    """upward, downward, towards the sun and around its edge, of every length; entries 1 and 2 (where they exist) are zero and NaN"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * rng.uniform(0.1, 30.0, size=(n, 1))
    d[::3, 1] = -np.abs(d[::3, 1])                                                                   # a third looks down
    return d.astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("stride", [3, 6])
def test_radiance_along_directions(n, stride):
    torch, dev = _torch()
    sky = R.sky(25.0, 3000.0 if n % 2 else 1.0, (32, 16))
    d = _directions(n, n + stride)
    s = sky.sun_direction()
    if n > 4:
        d[1], d[2] = (0.0, 0.0, 0.0), (1.0, NAN, 0.0)
        d[3], d[4] = (7.0 * s).astype(np.float32), (s + np.array([0.0, 0.02, 0.0])).astype(np.float32)   # inside the disc, and 1 degree outside it
    if stride == 6:                                                                                  # inside a ray buffer, read in place
        rays = np.full((n, 6), NAN, np.float32)
        rays[:, 3:6] = d
        view = rays[:, 3:6]
    else:
        view = d
    for disc in (False, True):
        terms = {}
        ref = api.sky_radiance(sky.to_abi(disc=disc), d, terms=terms)
        R.assert_margins(terms, f"n {n} disc {disc}")
        got = _lib.sky_radiance(sky.to_abi(disc=disc), view)
        full = {k: np.zeros((n,) + terms[k].shape[1:]) for k in ("scatter", "ground_nocos")}
        t_max = np.full(n, np.inf)
        for k in full:
            full[k][terms["ok"]] = terms[k]
        t_max[terms["ok"]] = terms["t_max"]
        t = dict(terms, t_max=t_max, **full)
        kc = R.k_common(terms["tau_max"], 32, 16)
        cos_sr = np.cos(np.float64(np.float32(sky.sun_radius)))
        extra = R.EPS * (kc + 2.0 / (1.0 - cos_sr)) * np.abs(ref.astype(np.float64)) if disc else None
        R.assert_close(got, ref, t, 32, 16, f"n {n} stride {stride} disc {disc}", extra)
        if n > 4:
            assert np.all(got[1:3] == 0.0) and np.all(got[0] > 0)
            if disc:
                assert np.all(got[3] > 100.0 * got[4]) and np.all(got[4] > 0)                           # the disc against the sky one degree beside it
        dv = torch.from_numpy(np.ascontiguousarray(rays if stride == 6 else d)).to(dev)
        out = torch.full((n, 3), NAN, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _lib.sky_radiance(sky.to_abi(disc=disc), dv[:, 3:6] if stride == 6 else dv, out=out, stream=side.cuda_stream)
        assert np.array_equal(_u32(out.cpu().numpy()), _u32(got))
        if stride == 6:
            assert np.all(np.isnan(rays[:, :3]))


def test_map_texel_equals_radiance_along_its_direction():
    """the two kernels share one radiance function: the map's texel is fw_sky_radiance along panorama_rays' float64 direction, to the
    rounding of that direction to float32 (2^-24 relative in d; ln L changes by less than 100 per radian away from the disc)"""
    sky = R.sky(35.0)
    rays = api.panorama_rays((0.0, 0.0, 0.0), 64, 32, 0, jitter=False)
    along = _lib.sky_radiance(sky, rays[:, 3:6]).astype(np.float64)
    m = _lib.sky_map(sky, 64, 32).reshape(-1, 3).astype(np.float64)
    assert np.all(np.abs(along - m) <= 1e-5 * m)


# ---- energy ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size, elevation", [((8, 4), 60.0), ((64, 32), 2.0), ((65, 33), 10.0), ((256, 128), 60.0), ((256, 128), 2.0)])
def test_disc_energy_is_the_sun_lights(size, elevation):
    """sum (map_on - map_off) Omega = fw_sky_sun's irradiance.  Each covered texel is float32(L + g) and float32(L): their difference is
    off g by at most 2^-24 (|L + g| + |L|), the light is float32(E0 T(O)): 2^-24 of itself; the rest is float64 rounding"""
    w, h = size
    sky = R.sky(elevation)
    on = _lib.sky_map(sky.to_abi(disc=True), w, h).astype(np.float64)
    off = _lib.sky_map(sky.to_abi(disc=False), w, h).astype(np.float64)
    omega = ED.omega_row(w, h)[:, None, None]
    energy = ((on - off) * omega).sum((0, 1))
    slack = (2.0 ** -24 * (np.abs(on) + np.abs(off)) * (on != off) * omega).sum((0, 1))
    light = _lib.sky_sun(sky)
    want = np.array([light.intensity.x, light.intensity.y, light.intensity.z], np.float64)
    print(f"{w}x{h} at {elevation}: energy {energy}, the light {want}, allowed {slack + 2.0 ** -24 * want}")
    assert np.all(want > 0) and np.all(np.abs(energy - want) <= slack + 2.0 ** -24 * want + 2.0 ** -40 * want)


# ---- into the renderer and the lights ---------------------------------------------------------------------------------------------------
def _empty_scene(env):
    """one small sphere far below that no ray of these tests meets: a scene needs an object"""
    scene = Scene.new()
    m = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    scene.add_object(RenderObject.new(Sphere.new(0.001, m)).position(0.3, -1000.0, 0.2))
    scene.set_environment(env)
    return scene


@pytest.mark.parametrize("sun", ["disc", "none"])
def test_renderer_reads_the_map_bit_for_bit(sun):
    sky = R.sky(35.0)
    env = SunSkyEnv(sky, 64, 32, sun)
    rays = api.panorama_rays((0.0, 0.0, 0.0), 64, 32, 0, jitter=False)
    ds = _lib.DeviceScene(_empty_scene(env).to_desc())
    try:
        res = ds.render_rays(rays, 1)
    finally:
        ds.close()
    want = _lib.sky_map(sky.to_abi(disc=sun == "disc"), 64, 32)
    assert np.array_equal(_u32(res.linear), _u32(want.reshape(-1, 3)))
    assert np.array_equal(_u32(env.bake()), _u32(want))


def test_sun_as_a_light_through_bake_direct():
    """E = E0 T(O) sin(el) at an upward-facing point: the light's irradiance is one float32 rounding of E0 T(O), its stored direction one
    per component (2^-24 / sin(el) relative in the cosine), the result one more: 2^-24 (2 + 1 / sin(el)) plus float64 rounding"""
    el = 35.0
    sky = R.sky(el)
    scene = _empty_scene(SunSkyEnv(sky, 8, 4, "light"))
    assert len(scene.lights) == 1
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        out, _sums, _stats = ds.bake_direct(DirectLight(0.0, "cosine"), np.zeros((1, 3), np.float32), np.array([[0.0, 1.0, 0.0]], np.float32))
    finally:
        ds.close()
    k = api._sky_constants(sky)
    want = k["e0"] * api._sky_transmittance(k, k["O"])[0] * k["s"][1]
    got = out.reshape(-1, 8)[0]
    assert got[3] == 1.0                                                                             # one light, visible
    assert np.all(np.abs(got[:3].astype(np.float64) - want) <= 2.0 ** -24 * (2.0 + 1.0 / k["s"][1]) * want + 2.0 ** -40 * want), (got, want)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip(tmp_path):
    from firework_amd.__main__ import main
    from PIL import Image
    yml = os.path.join(ROOT, "scenes", "sun_sky.yml")
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(32).height(24).samples(2).use_bvh(True).camera(cam).seed(0)
    base = ["--scene-file", yml, "-s", "2", "--width", "32", "--height", "24"]
    png = str(tmp_path / "a.png")
    assert main(base + ["-o", png]) == 0                                                             # the file's own SunSkyEnv
    img = np.asarray(Image.open(png).convert("RGB"))
    want = r.render(yaml_io.load_scene(yml))
    assert img.shape == (24, 32, 3) and np.array_equal(img.reshape(-1, 3), want.reshape(-1, 3)) and img.max() > 0
    png2 = str(tmp_path / "b.png")
    assert main(base + ["--sun-sky", "10,60,3", "--sun-sky-size", "64,32", "--sun", "none", "-o", png2]) == 0
    scene = yaml_io.load_scene(yml)
    scene.set_environment(SunSkyEnv(SunSky(10.0, 60.0, 3.0), 64, 32, "none"))
    img2 = np.asarray(Image.open(png2).convert("RGB"))
    assert np.array_equal(img2.reshape(-1, 3), r.render(scene).reshape(-1, 3)) and not np.array_equal(img2, img)


def test_fw_render_is_left_as_it_was():
    scene, r = scenes.config("C2_cornell_box", 32, 32, 4)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        before = ds.render(r)
        sky = R.sky(10.0)
        _lib.sky_map(sky.to_abi(disc=True), 65, 33)
        _lib.sky_radiance(sky, _directions(65, 1))
        _lib.sky_sun(sky)
        after = ds.render(r)
    finally:
        ds.close()
    assert np.array_equal(before.rgb8, after.rgb8) and np.array_equal(_u32(before.linear), _u32(after.linear))
