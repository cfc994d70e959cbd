"""CPU-side checks of the camera models generated on the device (fw_model_rays, fw_render_model, fw_render_model_aovs): the exports and
fw_camera_model's layout at ABI 8, every argument error in the header's order (before the scene is looked at or HIP is called), the
no-device error with the caller's buffer left as it was, the fisheye's numpy statement against known answers, and the CLI's checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import CameraModel, CameraSettings, fisheye_rays, orthographic_rays, panorama_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = CameraSettings.default().cam_pos((3.0, 30.0, 50.0)).look_at((0.5, -1.0, 2.0))


def _basis(cam):
    pos, at = np.asarray(cam._cam_pos, np.float64), np.asarray(cam._look_at, np.float64)
    w = (pos - at) / np.linalg.norm(pos - at)
    u = np.cross([0.0, 1.0, 0.0], w)
    u /= np.linalg.norm(u)
    return u, np.cross(w, u), w


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    for name, args in (("fw_model_rays", r"const fw_camera_model \*model, int device, uint32_t first_sample, uint32_t n_samples, float \*rays, "
                                         r"int on_device,\s*void \*stream"),
                       ("fw_render_model", r"fw_scene \*scene, const fw_camera_model \*model, const fw_render_rays_params \*rp, float \*accum,"
                                           r"\s*uint8_t \*rgb8, float \*gamma_rgb, float \*linear_rgb, fw_stats \*stats"),
                       ("fw_render_model_aovs", r"fw_scene \*scene, const fw_camera_model \*model, const fw_render_params \*params, float \*aov, "
                                                r"fw_stats \*stats")):
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\s*\({args}\);", text), name


def test_camera_model_layout(tmp_path):
    """ctypes' fw_camera_model equals the C compiler's, size and every field offset; the kinds are the header's"""
    names = [f for f, _ in A.fw_camera_model._fields_]
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(names) +
           ' %d %d %d\\n",sizeof(fw_camera_model)' + "".join(f",offsetof(fw_camera_model,{f})" for f in names) +
           ',FW_MODEL_PANORAMA,FW_MODEL_ORTHOGRAPHIC,FW_MODEL_FISHEYE);return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out[0] == C.sizeof(A.fw_camera_model)
    assert out[1:1 + len(names)] == [getattr(A.fw_camera_model, f).offset for f in names]
    assert out[1 + len(names):] == [A.FW_MODEL_PANORAMA, A.FW_MODEL_ORTHOGRAPHIC, A.FW_MODEL_FISHEYE]


def _model(base=A.FW_MODEL_FISHEYE, **kw):
    """a valid 4 x 2 model of kind `base`, then fields overwritten"""
    m = (CameraModel.panorama(CAM._cam_pos, 4, 2) if base == A.FW_MODEL_PANORAMA else
         CameraModel.orthographic(CAM, 3.0, 4, 2) if base == A.FW_MODEL_ORTHOGRAPHIC else CameraModel.fisheye(CAM, 180.0, 4, 2)).to_abi()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _cam(pos=(3.0, 30.0, 50.0), at=(0.5, -1.0, 2.0), **kw):
    c = CameraSettings.default().cam_pos(pos).look_at(at).to_abi()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _bad_models():
    """(what, model) for every model error of the header, in its order"""
    nan, inf = float("nan"), float("inf")
    out = [("kind", _model(kind=3)), ("kind", _model(kind=-1)), ("width", _model(width=0)), ("height", _model(height=0)),
           ("camera", _model(camera=_cam(pos=(nan, 0.0, 0.0)))), ("camera", _model(camera=_cam(at=(0.0, inf, 0.0)))),
           ("camera", _model(A.FW_MODEL_PANORAMA, camera=_cam(vfov=nan)))]
    for kind in (A.FW_MODEL_ORTHOGRAPHIC, A.FW_MODEL_FISHEYE):
        out += [("basis", _model(kind, camera=_cam(pos=(1.0, 2.0, 3.0), at=(1.0, 2.0, 3.0)))),
                ("basis", _model(kind, camera=_cam(pos=(1.0, 2.0, 3.0), at=(1.0, -5.0, 3.0))))]
    out += [("view_height", _model(A.FW_MODEL_ORTHOGRAPHIC, view_height=v)) for v in (0.0, -1.0, nan, inf)]
    out += [("fov", _model(A.FW_MODEL_FISHEYE, fov=v)) for v in (0.0, -90.0, 360.5, nan, inf)]
    return out


def _rp(**kw):
    p = A.fw_render_rays_params()
    p.n_rays, p.samples, p.per_sample_rays, p.gamma, p.use_bvh = 8, 2, 1, 2.2, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BIG = dict(width=1 << 16, height=1 << 15)       # W x H = 2^31: the jitter counter's limit


def test_model_rays_argument_checks():
    lib = _lib.load()
    rays = np.full((2, 8, 6), 7.0, np.float32)

    def call(m, first=0, n=2, r=rays, on_device=0, ptr=None):
        return lib.fw_model_rays(None if m is None else C.byref(m), 0, first, n, ptr if ptr is not None else (None if r is None else r.ctypes.data),
                                 on_device, None)

    assert call(None) == A.FW_ERR_BAD_ARG
    assert call(_model(), r=None) == A.FW_ERR_BAD_ARG
    for what, m in _bad_models():
        assert call(m) == A.FW_ERR_BAD_ARG, what
    assert call(_model(), n=0) == A.FW_ERR_BAD_ARG
    assert call(_model(), first=0xFFFFFFFF, n=2) == A.FW_ERR_BAD_ARG                          # the sample range overflows
    assert call(_model(), on_device=1, ptr=C.c_void_p(rays.ctypes.data + 2)) == A.FW_ERR_BAD_ARG
    # the order: bad arguments before the size limit, the size limit before the device
    assert call(_model(**BIG), n=0) == A.FW_ERR_BAD_ARG
    assert call(_model(fov=0.0, **BIG)) == A.FW_ERR_BAD_ARG
    assert call(_model(**BIG)) == A.FW_ERR_UNSUPPORTED
    assert call(_model(A.FW_MODEL_PANORAMA, **BIG)) == A.FW_ERR_UNSUPPORTED
    # what a model does not use is not checked: a panorama has no basis, view plane or fov
    ok = [_model(A.FW_MODEL_PANORAMA, camera=_cam(pos=(1.0, 2.0, 3.0), at=(1.0, 2.0, 3.0))), _model(A.FW_MODEL_PANORAMA, fov=-1.0, view_height=-1.0),
          _model(A.FW_MODEL_ORTHOGRAPHIC, fov=-1.0), _model(A.FW_MODEL_FISHEYE, view_height=-1.0), _model(fov=360.0), _model(),
          _model(A.FW_MODEL_ORTHOGRAPHIC)]
    if _lib.device_count() == 0:
        for m in ok:
            assert call(m) == A.FW_ERR_NO_DEVICE
        assert call(_model(), first=0xFFFFFFFE, n=2) == A.FW_ERR_NO_DEVICE                    # [2^32 - 2, 2^32) is a valid range
        assert np.all(rays == 7.0)                                                           # the caller's buffer is as it was


def test_render_model_argument_checks():
    """a 64-byte buffer that is no scene stands in for one: nothing dereferences it before the arguments are valid and a device is found"""
    lib = _lib.load()
    not_a_scene = C.create_string_buffer(64)
    acc = np.full((8, 4), 7.0, np.float32)

    def call(scene, m, p, accum=acc, ptr=None):
        return lib.fw_render_model(scene, None if m is None else C.byref(m), None if p is None else C.byref(p),
                                   ptr if ptr is not None else (None if accum is None else accum.ctypes.data), None, None, None, None)

    assert call(None, _model(), _rp()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, None, _rp()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), None) == A.FW_ERR_BAD_ARG
    for what, m in _bad_models():
        assert call(not_a_scene, m, _rp()) == A.FW_ERR_BAD_ARG, what
    assert call(not_a_scene, _model(), _rp(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), _rp(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), _rp(first_sample=0xFFFFFFFF, samples=1)) == A.FW_ERR_BAD_ARG
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert call(not_a_scene, _model(), _rp(gamma=g)) == A.FW_ERR_BAD_ARG, g
    for n in (0, 7, 9):
        assert call(not_a_scene, _model(), _rp(n_rays=n)) == A.FW_ERR_BAD_ARG, n
    assert call(not_a_scene, _model(), _rp(first_sample=3), accum=None) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), _rp(on_device=1), ptr=C.c_void_p(acc.ctypes.data + 4)) == A.FW_ERR_BAD_ARG
    # the order
    assert call(not_a_scene, _model(**BIG), _rp(n_rays=8)) == A.FW_ERR_BAD_ARG                # n_rays != W x H comes first
    assert call(not_a_scene, _model(**BIG), _rp(n_rays=1 << 31, gamma=0.0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(**BIG), _rp(n_rays=1 << 31)) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(not_a_scene, _model(), _rp()) == A.FW_ERR_NO_DEVICE
        assert call(not_a_scene, _model(chunk_samples=1), _rp(first_sample=2, per_sample_rays=0)) == A.FW_ERR_NO_DEVICE
        assert call(not_a_scene, _model(A.FW_MODEL_PANORAMA), _rp(), accum=None) == A.FW_ERR_NO_DEVICE
        assert np.all(acc == 7.0)


def test_render_model_aovs_argument_checks():
    lib = _lib.load()
    not_a_scene = C.create_string_buffer(64)
    aov = np.full((8, 12), 7.0, np.float32)

    def params(**kw):
        p = A.fw_render_params()
        p.samples, p.use_bvh = 2, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(scene, m, p, a=aov, ptr=None):
        return lib.fw_render_model_aovs(scene, None if m is None else C.byref(m), None if p is None else C.byref(p),
                                        ptr if ptr is not None else (None if a is None else a.ctypes.data), None)

    assert call(None, _model(), params()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, None, params()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), None) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), params(), a=None) == A.FW_ERR_BAD_ARG
    for what, m in _bad_models():
        assert call(not_a_scene, m, params()) == A.FW_ERR_BAD_ARG, what
    assert call(not_a_scene, _model(), params(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), params(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(), params(outputs_on_device=1), ptr=C.c_void_p(aov.ctypes.data + 4)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(**BIG), params(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _model(**BIG), params()) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        # only samples, use_bvh, seed, outputs_on_device and stream are read: a size, pixel ids or an RNG mode of params' own change nothing
        ids = (C.c_uint32 * 2)(0, 1)
        odd = params(width=0, height=0, rng_mode=A.FW_RNG_LCG, pixel_ids=ids, n_pixels=2, gamma=0.0)
        assert call(not_a_scene, _model(), params()) == A.FW_ERR_NO_DEVICE
        assert call(not_a_scene, _model(), odd) == A.FW_ERR_NO_DEVICE
        assert np.all(aov == 7.0)


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    model = CameraModel.fisheye(CAM, 180.0, 8, 4).seed(3)
    for call in (lambda: _lib.model_rays(model, 0, 2), lambda: r.render_model(scene, model, 4, chunk=2),
                 lambda: r.model_aovs(scene, model, 2), lambda: r.render_model_denoised(scene, model, 2)):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


def test_camera_model_builders_state_the_numpy_rays():
    """CameraModel.rays(sample) is panorama_rays / orthographic_rays / fisheye_rays with the model's seed and jitter; to_abi carries them"""
    pano = CameraModel.panorama((1.0, -2.0, 3.0), 16, 8).seed(7)
    assert np.array_equal(pano.rays(5), panorama_rays((1.0, -2.0, 3.0), 16, 8, 5, seed=7))
    ortho = CameraModel.orthographic(CAM, 7.5, 16, 8).seed(0x1234567800000009).jitter(False)
    assert np.array_equal(ortho.rays(2), orthographic_rays(CAM, 7.5, 16, 8, 2, jitter=False))
    fish = CameraModel.fisheye(CAM, 200.0, 16, 8).seed(9)
    assert np.array_equal(fish.rays(3), fisheye_rays(CAM, 200.0, 16, 8, 3, seed=9))
    m = ortho.to_abi()
    assert (m.kind, m.width, m.height, m.view_height, m.jitter, m.seed, m.chunk_samples) == (A.FW_MODEL_ORTHOGRAPHIC, 16, 8, 7.5, 0,
                                                                                             0x1234567800000009, 0)
    assert fish.to_abi().fov == 200.0 and fish.to_abi().jitter == 1
    with pytest.raises(ValueError):
        fisheye_rays(CAM, 0.0, 4, 4, 0)
    with pytest.raises(ValueError):
        fisheye_rays(CAM, 361.0, 4, 4, 0)


def test_fisheye_centre_ray():
    """the centre of an even-sized image without jitter lies between four pixels whose directions average to -w's direction; the one
    pixel of a 1 x 1 image is the centre itself"""
    u, v, w = _basis(CAM)
    one = fisheye_rays(CAM, 180.0, 1, 1, 0, jitter=False)
    assert one.shape == (1, 6) and np.array_equal(one[0, :3], CAM._cam_pos)
    assert np.array_equal(one[0, 3:], (-w).astype(np.float32))
    for W, H in ((8, 6), (64, 64)):
        d = fisheye_rays(CAM, 120.0, W, H, 0, jitter=False)[:, 3:].astype(np.float64).reshape(H, W, 3)
        mid = d[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].reshape(4, 3).mean(axis=0)
        assert np.allclose(mid / np.linalg.norm(mid), -w, rtol=0, atol=1e-6)


@pytest.mark.parametrize("fov", [90.0, 180.0, 360.0])
def test_fisheye_angles(fov):
    """unit directions whose angle to -w is r * fov / 2 (equidistant), r the pixel's distance from the centre over the half diagonal;
    the azimuth is the pixel's; the origin is the position"""
    W, H, sample, seed = 24, 10, 5, 9
    u, v, w = _basis(CAM)
    rays = fisheye_rays(CAM, fov, W, H, sample, seed=seed)
    assert rays.dtype == np.float32 and rays.shape == (W * H, 6)
    assert np.array_equal(rays[:, :3], np.broadcast_to(np.asarray(CAM._cam_pos, np.float32), (W * H, 3)))
    d = rays[:, 3:].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-6
    from firework_amd.api import pixel_jitter
    xi = pixel_jitter(seed, sample, W * H)
    j, x = np.divmod(np.arange(W * H), W)
    a, b = 2.0 * (x + xi[:, 0]) - W, H - 2.0 * (j + xi[:, 1])
    r = np.hypot(a, b) / np.hypot(W, H)
    assert 0.0 < r.min() and r.max() < 1.0
    theta = np.arctan2(np.linalg.norm(np.cross(d, -w), axis=1), d @ -w)
    assert np.abs(theta - r * np.radians(fov) / 2.0).max() <= 1e-6
    away = r * fov > 1.0                                               # (the azimuth of a ray almost along -w is ill-conditioned)
    assert np.abs(np.angle(np.exp(1j * (np.arctan2(d @ v, d @ u) - np.arctan2(b, a))))[away]).max() <= 1e-5
    if fov <= 180.0:
        assert np.all(d @ -w > 0.0)                                    # the front half-space
    else:
        assert np.any(d @ -w < 0.0)
    # row 0 is the top, column 0 the left
    c = fisheye_rays(CAM, fov, W, H, 0, jitter=False)[:, 3:].astype(np.float64).reshape(H, W, 3)
    assert (c[0, W // 2] - c[H - 1, W // 2]) @ v > 0 and (c[H // 2, W - 1] - c[H // 2, 0]) @ u > 0


def test_cli_fisheye_checks(capsys):
    from firework_amd.__main__ import main
    for extra in (["--orbit", "3", "-o", "f_{}.png"], ["--adaptive", "0.05"], ["--denoise"], ["--progressive", "2"], ["--checkpoint", "c.npz"]):
        with pytest.raises(SystemExit) as e:
            main(["--scene-file", "s.yml", "-s", "4", "--camera", "fisheye", "-o", "x.png"] + extra)
        assert e.value.code == 2
        assert "--camera fisheye" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "s.yml", "-s", "4", "--camera", "fisheye", "--orbit", "3", "--temporal", "-o", "f_{}.png"])
    assert e.value.code == 2 and "--temporal" in capsys.readouterr().err
    for cam in ([], ["--camera", "panorama"], ["--camera", "orthographic"]):
        with pytest.raises(SystemExit) as e:
            main(["--scene-file", "s.yml", "-s", "4", "--fisheye-fov", "120", "-o", "x.png"] + cam)
        assert e.value.code == 2 and "--fisheye-fov" in capsys.readouterr().err
    for bad in ("0", "-10", "361", "nan"):
        with pytest.raises(SystemExit) as e:
            main(["--scene-file", "s.yml", "-s", "4", "--camera", "fisheye", "--fisheye-fov", bad, "-o", "x.png"])
        assert e.value.code == 2 and "--fisheye-fov" in capsys.readouterr().err


# A host against include/firework.hpp: firework::CameraModel and Renderer::render_model.  First a model of 2^31 pixels (refused), then
# the three models over cornell's walls at 24 x 10, 4 spp; prints one FNV-1a hash per image.  tests/test_gpu_camera_models.py compares
# the hashes with the Python path's.
CPP_HOST = r"""
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
    CameraSettings camera = CameraSettings::default_().cam_pos({278.f, 278.f, -800.f}).look_at({278.f, 270.f, 0.f});
    Renderer r = Renderer::default_().samples(4).use_bvh(true).seed(5);
    try { r.render_model(world, CameraModel::fisheye(camera, 180.0, 65536, 32768)); std::printf("large: rendered\n"); }
    catch (const std::exception &e) { std::printf("large: %s\n", e.what()); }
    const CameraModel models[3] = {CameraModel::panorama({278.f, 278.f, 278.f}, 24, 10).seed(3),
                                   CameraModel::orthographic(camera, 500.0, 24, 10).seed(3).chunk_samples(3),
                                   CameraModel::fisheye(camera, 150.0, 24, 10).seed(3).jitter(false)};
    for (const CameraModel &m : models) {
        try {
            const std::vector<Color> img = r.render_model(world, m);
            unsigned long long h = 1469598103934665603ull;
            for (const Color &c : img) for (uint8_t b : {c.r, c.g, c.b}) { h ^= b; h *= 1099511628211ull; }
            std::printf("model %d: %zu pixels %016llx\n", (int)m.m.kind, img.size(), h);
        } catch (const std::exception &e) { std::printf("error: %s\n", e.what()); return 3; }
    }
    return 0;
}
"""


def build_cpp_host(tmp_path):
    src, exe = tmp_path / "models.cpp", tmp_path / "models"
    src.write_text(CPP_HOST)
    libdir = os.path.join(ROOT, "firework_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", libdir,
                           "-lfirework_hip", f"-Wl,-rpath,{libdir}"])
    return exe


def test_cpp_host_compiles_and_checks_its_arguments(tmp_path):
    """firework::CameraModel and Renderer::render_model compile against the C ABI; 2^31 pixels are refused as unsupported (the 32-bit
    ray count never wraps), and without a GPU the first real render reports the missing device"""
    lib = _lib.load()
    out = subprocess.run([str(build_cpp_host(tmp_path))], capture_output=True, text=True, timeout=300)
    lines = out.stdout.splitlines()
    assert lines[0].startswith("large: " + lib.fw_strerror(A.FW_ERR_UNSUPPORTED).decode()), out.stdout
    if _lib.device_count() == 0:
        assert out.returncode == 3 and lines[1].startswith("error: " + lib.fw_strerror(A.FW_ERR_NO_DEVICE).decode()), out.stdout
    else:
        assert out.returncode == 0 and len(lines) == 4 and all("240 pixels" in x for x in lines[1:]), out.stdout
