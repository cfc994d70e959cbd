"""CPU-side checks of rendering along caller-supplied rays (fw_render_rays): the export and its struct layout at ABI 8, the argument
errors (checked before the scene is looked at or HIP is called), the no-device error of the Python entry points, the CLI's --camera
checks, and the two camera models: the panorama as the exact inverse of the HDR environment lookup, the orthographic rays against a
float64 statement of their formula, and jitter that does not depend on how samples are chunked."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import CameraSettings, orthographic_rays, panorama_rays, pixel_jitter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_layout(tmp_path, struct, fields):
    src = '#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(fields) + '\\n",sizeof(' + \
          struct + ')' + "".join(f",offsetof({struct},{f})" for f in fields) + ');return 0;}'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    return out[0], out[1:]


def test_render_rays_export_at_abi_8():
    lib = _lib.load()
    assert hasattr(lib, "fw_render_rays")
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    entry_points = text[text.index("/* ---- entry points"):]
    assert re.search(r"\bint fw_render_rays\s*\(fw_scene \*scene, const fw_render_rays_params \*p, const float \*rays, float \*accum,"
                     r"\s*uint8_t \*rgb8, float \*gamma_rgb, float \*linear_rgb, fw_stats \*stats\);", entry_points)


def test_render_rays_params_layout(tmp_path):
    """ctypes' fw_render_rays_params equals the C compiler's, size and every field offset"""
    names = [f for f, _ in A.fw_render_rays_params._fields_]
    size, offs = _c_layout(tmp_path, "fw_render_rays_params", names)
    assert size == C.sizeof(A.fw_render_rays_params)
    assert offs == [getattr(A.fw_render_rays_params, f).offset for f in names]


def _params(**kw):
    p = A.fw_render_rays_params()
    p.n_rays, p.samples, p.per_sample_rays, p.gamma, p.use_bvh = 4, 2, 1, 2.2, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_render_rays_argument_checks():
    """Every argument error comes back before the scene is dereferenced or HIP is called: a 64-byte buffer that is no scene stands in
    for one.  The order is the header's."""
    lib = _lib.load()
    not_a_scene = C.create_string_buffer(64)
    rays = np.zeros((2, 4, 6), np.float32)
    rays[..., 5] = 1.0
    acc = np.zeros((4, 4), np.float32)

    def call(scene, p, r=rays, accum=acc):
        return lib.fw_render_rays(scene, None if p is None else C.byref(p), None if r is None else r.ctypes.data,
                                  None if accum is None else accum.ctypes.data, None, None, None, None)

    assert call(None, _params()) == A.FW_ERR_BAD_ARG                                         # null scene
    assert call(not_a_scene, None) == A.FW_ERR_BAD_ARG                                       # null params
    assert call(not_a_scene, _params(), r=None) == A.FW_ERR_BAD_ARG                          # null rays
    assert call(not_a_scene, _params(n_rays=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _params(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _params(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _params(first_sample=0xFFFFFFFF, samples=1)) == A.FW_ERR_BAD_ARG  # first_sample + samples overflows
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert call(not_a_scene, _params(gamma=g)) == A.FW_ERR_BAD_ARG, g
    assert call(not_a_scene, _params(first_sample=3), accum=None) == A.FW_ERR_BAD_ARG      # resume without the sums
    misaligned = C.c_void_p(acc.ctypes.data + 4)
    assert lib.fw_render_rays(not_a_scene, C.byref(_params(on_device=1)), rays.ctypes.data, misaligned, None, None, None, None) == A.FW_ERR_BAD_ARG
    # the order: an earlier check wins over a later one
    assert call(None, _params(n_rays=0, gamma=0.0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _params(n_rays=0), r=None) == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:                                                             # valid arguments: then the device
        assert call(not_a_scene, _params()) == A.FW_ERR_NO_DEVICE
        assert call(not_a_scene, _params(first_sample=2)) == A.FW_ERR_NO_DEVICE
        assert call(not_a_scene, _params(per_sample_rays=0), accum=None) == A.FW_ERR_NO_DEVICE


def test_render_rays_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    rays = panorama_rays((278.0, 278.0, 278.0), 8, 4, 0)
    for call in (lambda: r.render_rays(scene, rays, 2),
                 lambda: r.render_camera_model(scene, lambda s: panorama_rays((278.0, 278.0, 278.0), 8, 4, s), 4, chunk=2)):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


@pytest.mark.parametrize("w,h", [(256, 128), (1024, 512)])
def test_panorama_inverts_the_hdr_lookup(w, h):
    """Pixel-centre panorama rays are unit vectors that land, through the oracle's sphere_uv and env_sample's index arithmetic, on their
    own texel (x, row j)"""
    from oracle import oracle_binding as ob
    rays = panorama_rays((1.0, -2.0, 3.0), w, h, 0, jitter=False)
    assert rays.dtype == np.float32 and rays.shape == (w * h, 6)
    assert np.array_equal(rays[:, :3], np.broadcast_to(np.float32([1.0, -2.0, 3.0]), (w * h, 3)))
    d = rays[:, 3:]
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    lib = ob.load()
    uv = (C.c_float * 2)()
    fw, fh = np.float32(w), np.float32(h)
    for i in range(w * h):
        lib.fwo_sphere_uv(d[i].ctypes.data_as(C.POINTER(C.c_float)), uv)
        u, v = np.float32(uv[0]), np.float32(uv[1])
        x = int(np.float32(u * fw))                                    # environment.rs: (u * width) as usize
        y = int(np.float32((np.float32(1.0) - v) * fh))               # ((1 - v) * height) as usize
        assert (x, y) == (i % w, i // w), (i, x, y)


def test_orthographic_rays_formula():
    cam = CameraSettings.default().cam_pos((3.0, 30.0, 50.0)).look_at((0.5, -1.0, 2.0))
    w, h, vh, seed, sample = 24, 10, 7.5, 9, 5
    got = orthographic_rays(cam, vh, w, h, sample, seed=seed)
    assert got.dtype == np.float32 and got.shape == (w * h, 6)
    pos, at = np.float64([3.0, 30.0, 50.0]), np.float64([0.5, -1.0, 2.0])
    ww = (pos - at) / np.linalg.norm(pos - at)
    uu = np.cross([0.0, 1.0, 0.0], ww)
    uu /= np.linalg.norm(uu)
    vv = np.cross(ww, uu)
    xi = pixel_jitter(seed, sample, w * h)
    for i in range(w * h):
        x, j = i % w, i // w
        s, t = (x + xi[i, 0]) / w, 1.0 - (j + xi[i, 1]) / h
        o = pos + (s - 0.5) * (vh * w / h) * uu + (t - 0.5) * vh * vv
        assert np.allclose(got[i, :3], o, rtol=0, atol=1e-5 * np.abs(o).max()), i
        assert np.array_equal(got[i, 3:], (at - pos).astype(np.float32)), i
    # pixel centres without jitter; row 0 is the top of the view plane
    c = orthographic_rays(cam, vh, w, h, sample, jitter=False)
    assert np.dot(c[0, :3] - c[(h - 1) * w, :3], vv) > 0 and np.dot(c[w - 1, :3] - c[0, :3], uu) > 0


def test_jitter_does_not_depend_on_chunking():
    """sample s's rays are the same made alone or among others, and differ between samples and seeds"""
    alone = [panorama_rays((0.0, 1.0, 0.0), 16, 8, s, seed=7) for s in range(6)]
    for lo, hi in ((0, 6), (2, 5), (5, 6)):
        together = [panorama_rays((0.0, 1.0, 0.0), 16, 8, s, seed=7) for s in range(lo, hi)]
        for s, r in zip(range(lo, hi), together):
            assert np.array_equal(r, alone[s])
    assert not np.array_equal(alone[0], alone[1])
    assert not np.array_equal(alone[0], panorama_rays((0.0, 1.0, 0.0), 16, 8, 0, seed=8))
    xi = pixel_jitter(7, 3, 4096)
    assert xi.min() >= 0.0 and xi.max() < 1.0 and abs(xi.mean() - 0.5) < 0.02
    cam = CameraSettings.default()
    assert np.array_equal(orthographic_rays(cam, 2.0, 8, 4, 3, seed=1), orthographic_rays(cam, 2.0, 8, 4, 3, seed=1))


def test_cli_camera_refusals(capsys):
    from firework_amd.__main__ import main
    for model in ("panorama", "orthographic"):
        for extra in (["--orbit", "3", "-o", "f_{}.png"], ["--adaptive", "0.05"], ["--denoise"], ["--progressive", "2"]):
            with pytest.raises(SystemExit) as e:
                main(["--scene-file", "s.yml", "-s", "4", "--camera", model, "-o", "x.png"] + extra)
            assert e.value.code == 2
            assert "--camera" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "s.yml", "-s", "4", "--ortho-height", "2", "-o", "x.png"])
    assert e.value.code == 2 and "--ortho-height" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "s.yml", "-s", "4", "--camera", "orthographic", "--ortho-height", "0", "-o", "x.png"])
    assert e.value.code == 2 and "--ortho-height" in capsys.readouterr().err
