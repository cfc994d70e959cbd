"""Point, spot and directional lights (fw_scene_set_lights) without a GPU: the ctypes fw_light against the header's layout,
fw_check_lights on a valid list and on each invalid case, the YAML `lights:` list (round trip; files without it dump as before), and the
float64 restatement the GPU tests measure the device against (tests/delta_lights_ref.py) on values computed by hand."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from firework_amd import _abi as A
from firework_amd import _lib, scenes, yaml_io
from firework_amd.api import DirectionalLight, PointLight, Scene, SpotLight

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_lights_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_fw_light_matches_header(tmp_path):
    fields = ["kind", "position", "direction", "intensity", "cos_inner", "cos_outer"]
    src = '#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(fw_light));' + \
          "".join(f'printf(" %zu", offsetof(fw_light, {f}));' for f in fields) + \
          'printf(" %d %d %d %u\\n", FW_LIGHT_POINT, FW_LIGHT_SPOT, FW_LIGHT_DIRECTIONAL, FW_MAX_LIGHTS);return 0;}'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert out[0] == C.sizeof(A.fw_light) == 48
    assert out[1:7] == [getattr(A.fw_light, f).offset for f in fields]
    assert out[7:] == [A.FW_LIGHT_POINT, A.FW_LIGHT_SPOT, A.FW_LIGHT_DIRECTIONAL, A.FW_MAX_LIGHTS]
    lib = _lib.load()
    assert hasattr(lib, "fw_scene_set_lights") and hasattr(lib, "fw_check_lights")


def _valid():
    return [PointLight((0, 2, 0), (10, 10, 10)), SpotLight((1, 3, 0), (0, -2, 0), (5, 4, 3), 20.0, 35.0),
            DirectionalLight((0.2, -1, 0.1), (1, 1, 0.5)), SpotLight((1, 3, 0), (0, -1, 0), (5, 4, 3), 30.0, 30.0),
            PointLight((0, 2, 0), (0, 0, 0))]


def test_check_lights_accepts_a_valid_list():
    _lib.check_lights(_valid())
    _lib.check_lights([])
    lib = _lib.load()
    assert lib.fw_check_lights(None, 0) == A.FW_OK
    assert lib.fw_scene_set_lights(None, None, 0) == A.FW_ERR_BAD_ARG            # no scene


def _rec(kind=A.FW_LIGHT_SPOT, position=(0, 1, 0), direction=(0, -1, 0), intensity=(1, 1, 1), ci=0.9, co=0.8):
    return A.fw_light(kind, A.vec3(position), A.vec3(direction), A.vec3(intensity), ci, co)


INVALID = {
    "nan position": _rec(A.FW_LIGHT_POINT, position=(0, math.nan, 0)),
    "inf position": _rec(A.FW_LIGHT_SPOT, position=(math.inf, 0, 0)),
    "nan direction": _rec(A.FW_LIGHT_DIRECTIONAL, direction=(0, -1, math.nan)),
    "inf intensity": _rec(A.FW_LIGHT_POINT, intensity=(1, math.inf, 1)),
    "nan intensity": _rec(A.FW_LIGHT_DIRECTIONAL, intensity=(math.nan, 1, 1)),
    "nan cosine": _rec(ci=math.nan),
    "negative intensity": _rec(A.FW_LIGHT_POINT, intensity=(1, -0.5, 1)),
    "zero spot direction": _rec(A.FW_LIGHT_SPOT, direction=(0, 0, 0)),
    "zero directional direction": _rec(A.FW_LIGHT_DIRECTIONAL, direction=(0, 0, 0)),
    "cosines out of order": _rec(ci=0.5, co=0.6),
    "cos_inner above 1": _rec(ci=1.5, co=0.6),
    "cos_outer below -1": _rec(ci=0.5, co=-1.5),
    "unknown kind": _rec(kind=3),
    "negative kind": _rec(kind=-1),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_check_lights_refuses(case):
    lib = _lib.load()
    good = [l.to_abi() for l in _valid()]
    arr = (A.fw_light * (len(good) + 1))(*good, INVALID[case])            # the bad one last: the whole list is looked at
    assert lib.fw_check_lights(arr, len(good) + 1) == A.FW_ERR_BAD_ARG, case
    assert f"lights[{len(good)}]".encode() in lib.fw_last_error()
    assert lib.fw_check_lights(arr, len(good)) == A.FW_OK
    with pytest.raises(_lib.FireworkError) as e:
        _lib.check_lights(list(arr))
    assert e.value.status == A.FW_ERR_BAD_ARG


def test_check_lights_refuses_too_many_and_null():
    lib = _lib.load()
    n = A.FW_MAX_LIGHTS + 1
    arr = (A.fw_light * n)(*([PointLight((0, 1, 0), (1, 1, 1)).to_abi()] * n))
    assert lib.fw_check_lights(arr, n) == A.FW_ERR_BAD_ARG
    assert lib.fw_check_lights(arr, A.FW_MAX_LIGHTS) == A.FW_OK
    assert lib.fw_check_lights(None, 1) == A.FW_ERR_BAD_ARG


# ---- the Python and YAML layers ---------------------------------------------------------------------------------------------------------
def test_scene_add_light_and_desc():
    s = Scene.new()
    assert s.lights == []
    for i, l in enumerate(_valid()):
        assert s.add_light(l) == i
    with pytest.raises(TypeError):
        s.add_light("sun")
    spot = s.lights[1].to_abi()
    assert spot.kind == A.FW_LIGHT_SPOT and spot.cos_inner == np.float32(math.cos(math.radians(20.0)))
    assert spot.cos_outer == np.float32(math.cos(math.radians(35.0)))
    sun = s.lights[2].to_abi()
    assert sun.kind == A.FW_LIGHT_DIRECTIONAL and (sun.intensity.x, sun.intensity.y, sun.intensity.z) == (1.0, 1.0, 0.5)


def test_yaml_round_trip(tmp_path):
    scene, _ = scenes.cornell_box()
    for l in _valid()[:3]:
        scene.add_light(l)
    p = tmp_path / "lit.yml"
    yaml_io.save_scene(scene, str(p))
    y = yaml.safe_load(p.read_text())
    assert [l["light"] for l in y["lights"]] == ["PointLight", "SpotLight", "DirectionalLight"]
    back = yaml_io.load_scene(str(p))
    assert [type(l) for l in back.lights] == [PointLight, SpotLight, DirectionalLight]
    for a, b in zip(scene.lights, back.lights):
        assert bytes(a.to_abi()) == bytes(b.to_abi())
    assert (back.lights[1].inner_deg, back.lights[1].outer_deg) == (20.0, 35.0)
    p2 = tmp_path / "again.yml"
    yaml_io.save_scene(back, str(p2))
    assert p2.read_bytes() == p.read_bytes()
    with pytest.raises(ValueError):
        yaml_io.scene_from_dict(dict(y, lights=[{"light": "AreaLight"}]))


def test_yaml_without_lights_is_unchanged(tmp_path):
    """A scene without lights is written without the key, byte for byte what the writer produced before it knew lights: the same dict through
    the same dumper, and a file without `lights:` loads to a scene without lights and dumps to the same bytes."""
    scene, _ = scenes.cornell_box()
    d = yaml_io.scene_to_dict(scene)
    assert list(d) == ["render_objects", "materials", "environment"]
    p = tmp_path / "plain.yml"
    yaml_io.save_scene(scene, str(p))
    assert p.read_text() == yaml.safe_dump(d, sort_keys=False, default_flow_style=False)
    assert "lights" not in p.read_text()
    back = yaml_io.load_scene(str(p))
    assert back.lights == []
    p2 = tmp_path / "plain2.yml"
    yaml_io.save_scene(back, str(p2))
    assert p2.read_bytes() == p.read_bytes()
    assert scene.to_desc().content_hash() == back.to_desc().content_hash()


def test_example_scene_loads_and_fits_the_command_line_camera():
    """scenes/three_lights.yml, the README's example: it loads, holds one light of each kind that fw_check_lights accepts, round-trips, and
    lies in front of the CLI's fixed camera at (0, 30, 50) looking at the origin — objects and positional lights within 40 of the origin."""
    path = os.path.join(ROOT, "scenes", "three_lights.yml")
    scene = yaml_io.load_scene(path)
    assert sorted(type(l).__name__ for l in scene.lights) == ["DirectionalLight", "PointLight", "SpotLight"]
    _lib.check_lights(scene.lights)
    assert len(scene.to_desc().lights) == 3
    assert yaml.safe_load(open(path).read()) == yaml_io.scene_to_dict(scene)
    for ro in scene.render_objects[1:]:
        assert np.abs(ro._position).max() <= 40
    for l in scene.lights:
        if not isinstance(l, DirectionalLight):
            assert np.abs(l.position).max() <= 40 and l.position[1] > 0
    assert "scenes/three_lights.yml" in open(os.path.join(ROOT, "README.md")).read()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
UP = (0.0, 1.0, 0.0)


def test_ref_point_light_straight_above():
    a, I, h = 0.5, 12.0, 2.0
    got = R.contribution(PointLight((0.25, h, -1.0), (I, I / 2, 0.0)), (0.25, 0.0, -1.0), UP, (a, a, a))
    want = a * (2 / math.pi) * I / h ** 2                  # cos = 1: p_b = 2 / pi
    assert np.allclose(got, [want, want / 2, 0.0], rtol=1e-12, atol=0)


def test_ref_point_light_oblique_and_below():
    # the light at (3, 4, 0) from the origin: d = 5, cos = 4/5
    got = R.contribution(PointLight((3, 4, 0), (25, 25, 25)), (0, 0, 0), UP, (1, 1, 1))
    assert np.allclose(got, 2 * 0.8 ** 3 / math.pi * 25 / 25, rtol=1e-12)
    assert np.all(R.contribution(PointLight((3, -4, 0), (25, 25, 25)), (0, 0, 0), UP, (1, 1, 1)) == 0)      # below the horizon
    assert np.all(R.contribution(PointLight((1, 1, 1), (1, 1, 1)), (1, 1, 1), UP, (1, 1, 1)) == 0)           # at the light's own point


def test_ref_isotropic_and_pick_probability():
    got = R.contribution(PointLight((0, 0, 2), (8, 8, 8)), (0, 0, 0), (0, 0, 0), (0.5, 0.5, 0.5), beta=(1, 0.5, 0.25), p=0.25)
    want = 0.5 / (4 * math.pi) * 8 / 4 / 0.25
    assert np.allclose(got, [want, want / 2, want / 4], rtol=1e-12)


def test_ref_spot_cone():
    # axis straight down from (0, 2, 0); inner 30 deg, outer 60 deg.  A floor point at radius rho sees c = 2 / sqrt(4 + rho^2)
    spot = SpotLight((0, 2, 0), (0, -3, 0), (10, 10, 10), 30.0, 60.0)
    ci, co = float(np.float32(math.cos(math.radians(30)))), float(np.float32(math.cos(math.radians(60))))
    for rho in (0.0, 1.0, 2.0, 3.0, 4.0):
        d2 = 4 + rho * rho
        c = 2 / math.sqrt(d2)
        t = min(max((c - co) / (ci - co), 0.0), 1.0)
        s = t * t * (3 - 2 * t)
        want = 2 * c ** 3 / math.pi * 10 * s / d2
        got = R.contribution(spot, (rho, 0, 0), UP, (1, 1, 1))
        assert np.allclose(got, want, rtol=1e-12, atol=0), rho
    assert np.all(R.contribution(spot, (4.0, 0, 0), UP, (1, 1, 1)) == 0)                 # c = 0.447 < cos 60
    inside = R.contribution(spot, (0.5, 0, 0), UP, (1, 1, 1))[0]                          # c = 0.970 > cos 30: the point light's value
    assert inside == R.contribution(PointLight((0, 2, 0), (10, 10, 10)), (0.5, 0, 0), UP, (1, 1, 1))[0]
    hard = SpotLight((0, 2, 0), (0, -1, 0), (10, 10, 10), 45.0, 45.0)                     # cos_inner == cos_outer: a hard edge at rho = 2
    assert R.contribution(hard, (1.9, 0, 0), UP, (1, 1, 1))[0] == R.contribution(PointLight((0, 2, 0), (10, 10, 10)), (1.9, 0, 0), UP, (1, 1, 1))[0]
    assert np.all(R.contribution(hard, (2.1, 0, 0), UP, (1, 1, 1)) == 0)


def test_ref_directional():
    sun = DirectionalLight((0, -2, 0), (3, 2, 1))
    assert np.allclose(R.contribution(sun, (5, 0, 7), UP, (0.5, 0.5, 0.5)), 0.5 * 2 / math.pi * np.array([3.0, 2, 1]), rtol=1e-12)
    slant = DirectionalLight((1, -1, 0), (1, 1, 1))               # cos = 1 / sqrt 2, from the float32 direction the library stores
    c = float(np.float32(1 / math.sqrt(2)))
    assert np.allclose(R.contribution(slant, (0, 0, 0), UP, (1, 1, 1)), 2 * c ** 3 / math.pi, rtol=1e-7)
    assert np.all(R.contribution(DirectionalLight((0, 1, 0), (1, 1, 1)), (0, 0, 0), UP, (1, 1, 1)) == 0)     # shining upwards


def test_far_field_room_geometry_stays_inside_the_cap():
    """GPU check 6 compares an emissive sphere of radius r with a point light of I = Le pi r^2.  Their direct terms differ by O((r/d)^2):
    at the room's nearest surface points and at grazing ones the relative difference stays within 1e-4."""
    c, r, le = np.array(R.ROOM_LIGHT), R.ROOM_R, R.ROOM_LE
    point = PointLight(R.ROOM_LIGHT, (le * math.pi * r * r,) * 3)
    H, T = R.ROOM_HALF, R.ROOM_HEIGHT
    nearest = [((c[0], 0.0, c[2]), (0, 1, 0)), ((c[0], T, c[2]), (0, -1, 0)), ((-H, c[1], c[2]), (1, 0, 0)), ((H, c[1], c[2]), (-1, 0, 0)),
               ((c[0], c[1], -H), (0, 0, 1)), ((c[0], c[1], H), (0, 0, -1))]
    others = [((2.5, 0.0, 2.5), (0, 1, 0)), ((-2.9, 0.0, -2.9), (0, 1, 0)), ((H, 0.5, 2.0), (-1, 0, 0)), ((-1.0, T, 1.0), (0, -1, 0))]
    for x, n in nearest + others:
        d = float(np.linalg.norm(c - np.array(x)))
        assert d >= 2.0, (x, d)
        a = R.sphere_direct(c, r, le, x, n)
        b = R.contribution(point, x, n, (1, 1, 1))[0]
        assert a > 0 and abs(a - b) <= 1e-4 * b, (x, a, b, (r / d) ** 2)
