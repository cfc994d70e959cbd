"""CPU-side checks of the guide buffers and the denoiser (fw_render_aovs, fw_denoise): the exports at ABI 8, the parameter struct's layout,
the argument and no-device errors, the CLI's --denoise refusals, and the numpy restatement of the filter (tests/denoise_ref.py): its
identities, and its quality on oracle renders of cornell_box."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes

import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_denoise_exports_at_abi_8():
    lib = _lib.load()
    assert hasattr(lib, "fw_render_aovs") and hasattr(lib, "fw_denoise")
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    entry_points = text[text.index("/* ---- entry points"):]
    assert re.search(r"\bint fw_render_aovs\s*\(fw_scene \*scene, const fw_render_params \*params, float \*aov, fw_stats \*stats\);", entry_points)
    assert re.search(r"\bint fw_denoise\s*\(const fw_denoise_params \*p, const float \*color, const float \*aov, const float \*moments,\s*"
                     r"float \*linear_rgb, float \*gamma_rgb, uint8_t \*rgb8\);", entry_points)


def test_denoise_params_layout(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(fw_denoise_params), offsetof(fw_denoise_params, device), '
                   'offsetof(fw_denoise_params, stream)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, o_dev, o_stream = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(A.fw_denoise_params)
    assert o_dev == A.fw_denoise_params.device.offset and o_stream == A.fw_denoise_params.stream.offset


def test_constants_agree():
    """the header, the Python ABI and the restatement state the same constants"""
    h = R.header_constants()
    assert h == dict(EPS=R.EPS, NORMAL_POW=R.NORMAL_POW, PLANE=R.PLANE, LUM=R.LUM, ITERATIONS=R.ITERATIONS, MAX_ITERATIONS=10)
    assert (A.FW_DENOISE_EPS, A.FW_DENOISE_NORMAL_POW, A.FW_DENOISE_PLANE, A.FW_DENOISE_LUM, A.FW_DENOISE_ITERATIONS,
            A.FW_DENOISE_MAX_ITERATIONS) == (R.EPS, R.NORMAL_POW, R.PLANE, R.LUM, R.ITERATIONS, 10)
    kernels = open(os.path.join(ROOT, "firework_amd", "csrc", "fw_kernels.hip")).read()
    assert "FW_DENOISE_EPS" in kernels and "FW_DENOISE_PLANE" in kernels and "FW_DENOISE_LUM" in kernels


def test_aovs_argument_checks():
    """Every argument error comes back before the scene is dereferenced: 64 bytes that are no scene stand in for one."""
    lib = _lib.load()
    not_a_scene = C.addressof(C.create_string_buffer(64))
    _s, r = scenes.cornell_box()
    buf = np.zeros(8 * 8 * 12 + 4, F)
    aov = buf.ctypes.data

    def params(**kw):
        p = r.width(8).height(8).samples(4).to_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(scene, p, out=aov):
        return lib.fw_render_aovs(scene, None if p is None else C.byref(p), out, None)

    assert call(None, params()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, None) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, params(), None) == A.FW_ERR_BAD_ARG
    ids = np.array([0, 1], np.uint32)
    with_ids = params(n_pixels=2)
    with_ids.pixel_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    assert call(not_a_scene, with_ids) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, params(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, params(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, params(width=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, params(height=0)) == A.FW_ERR_BAD_ARG
    off = aov + (16 - aov % 16) + 4                                      # 4 bytes past a 16-byte boundary
    assert call(not_a_scene, params(outputs_on_device=1), off) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, params(rng_mode=A.FW_RNG_LCG, samples=0)) == A.FW_ERR_BAD_ARG     # BAD_ARG before UNSUPPORTED
    assert call(not_a_scene, params(rng_mode=A.FW_RNG_LCG)) == A.FW_ERR_UNSUPPORTED
    assert call(not_a_scene, params(width=1 << 16, height=1 << 16)) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(not_a_scene, params()) == A.FW_ERR_NO_DEVICE


def _dn_call(p, color, aov, moments=None):
    lib = _lib.load()
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    return lib.fw_denoise(None if p is None else C.byref(p), ptr(color), ptr(aov), ptr(moments), None, None, None)


def test_denoise_argument_checks():
    n = 8 * 8
    color, aov, mom = np.zeros((n, 3), F), np.zeros((n + 1, 12), F), np.zeros((n + 1, 4), F)

    def params(**kw):
        p = A.fw_denoise_params()
        p.width, p.height, p.iterations, p.gamma, p.device = 8, 8, 5, 2.2, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert _dn_call(None, color, aov) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(), None, aov) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(), color, None) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(width=0), color, aov) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(height=0), color, aov) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(iterations=11), color, aov) == A.FW_ERR_BAD_ARG
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert _dn_call(params(gamma=g), color, aov) == A.FW_ERR_BAD_ARG, g
    assert _dn_call(params(device=-1), color, aov) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(device=1 << 20), color, aov) == A.FW_ERR_BAD_ARG
    a_off = aov.ctypes.data + (16 - aov.ctypes.data % 16) + 4
    m_off = mom.ctypes.data + (16 - mom.ctypes.data % 16) + 8
    a_ok = aov.ctypes.data + (16 - aov.ctypes.data % 16) % 16
    assert _dn_call(params(on_device=1), color, a_off) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(on_device=1), color, a_ok, m_off) == A.FW_ERR_BAD_ARG
    assert _dn_call(params(width=1 << 16, height=1 << 16), color, aov) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        for L in (0, 5, 10):
            assert _dn_call(params(iterations=L), color, aov) == A.FW_ERR_NO_DEVICE
            assert _dn_call(params(iterations=L), color, aov, mom) == A.FW_ERR_NO_DEVICE


def test_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    r.width(8).height(8).samples(4)
    for call in (lambda: r.aovs(scene, 2), lambda: r.render_denoised(scene),
                 lambda: _lib.denoise(np.zeros((64, 3), F), np.zeros((64, 12), F), None, 8, 8)):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


def test_cli_denoise_refusals(tmp_path, capsys):
    from firework_amd.__main__ import main
    out = str(tmp_path / "o.png")
    for extra in (["--progressive", "2"], ["--checkpoint", str(tmp_path / "ck.npz")], ["--orbit", "3", "-o", str(tmp_path / "f{}.png")]):
        for dn in (["--denoise"], ["--denoise", "3"]):
            with pytest.raises(SystemExit) as e:
                main(["--scene-file", "s.yml", "-s", "16", "-o", out] + dn + extra)
            assert e.value.code == 2
            assert "--denoise" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "s.yml", "-s", "16", "-o", out, "--denoise", "11"])
    assert e.value.code == 2


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _synthetic(h, w, seed=0):
    rng = np.random.default_rng(seed)
    n = h * w
    color = rng.uniform(0, 1, (n, 3)).astype(F)
    aov = np.zeros((n, 12), F)
    aov[:, 0:3] = rng.uniform(0.2, 1, (n, 3))
    aov[:, 3] = 1
    nrm = rng.normal(size=(n, 3)) * 0.1 + np.array([0, 0, 1])
    aov[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    aov[:, 7] = rng.uniform(4, 6, n)
    yy, xx = np.mgrid[0:h, 0:w]
    aov[:, 8] = xx.ravel() * 0.01
    aov[:, 9] = yy.ravel() * 0.01
    aov[:, 10] = 5 + rng.normal(size=n) * 0.001
    mom = np.zeros((n, 4), F)
    mom[:, 3] = 16
    mom[:, 0:3] = 16 * color * color + rng.uniform(0, 1, (n, 3))
    return color, aov, mom


def test_restatement_identities():
    h, w = 23, 17
    color, aov, mom = _synthetic(h, w)
    for m in (None, mom):
        assert np.array_equal(R.filtered_linear(color, aov, m, w, h, 0), color.astype(np.float64))        # L = 0: the identity
    # constant image, constant guides: unchanged
    c = np.full((h * w, 3), [0.3, 0.5, 0.7], F)
    a = np.zeros((h * w, 12), F)
    a[:, 0:3] = [0.5, 0.6, 0.7]; a[:, 3] = 1; a[:, 6] = 1; a[:, 7] = 5
    yy, xx = np.mgrid[0:h, 0:w]
    a[:, 8] = xx.ravel(); a[:, 9] = yy.ravel(); a[:, 10] = 5
    mc = np.zeros((h * w, 4), F); mc[:, 3] = 8; mc[:, 0:3] = 8 * c * c + 0.01
    for m in (None, mc):
        for L in (1, 5, 10):
            out = R.filtered_linear(c, a, m, w, h, L)
            assert np.all(np.abs(out - c) <= 1e-6 * np.abs(c)), (L, m is None)
    # coverage 0 and non-finite inputs pass through
    cov0 = aov.copy()
    cov0[::7, 3] = 0
    cc = color.copy()
    cc[5] = np.nan; cc[9, 1] = np.inf
    for m in (None, mom):
        out = R.filtered_linear(cc, cov0, m, w, h, 5)
        assert np.array_equal(out[::7], cc[::7].astype(np.float64))
        assert np.array_equal(out[[5, 9]], cc[[5, 9]].astype(np.float64), equal_nan=True)
        assert np.all(np.isfinite(np.delete(out, [5, 9], axis=0)))


def _oracle_aovs(oracle, scene, r, samples):
    """AOVs of a cornell-like scene (constant textures) from oracle.trace of pixel rays built from oracle.camera's basis, at 2 x 2
    stratified offsets inside each pixel (pixel centres for one sample)."""
    s = r.settings
    w, h = s["width"], s["height"]
    cam = oracle.camera(r._camera, w, h)
    sd = scene.to_desc()
    idx = np.arange(w * h)
    px = (idx % w).astype(F)
    py = (h - idx // w).astype(F)
    per = []
    for k in range(samples):
        ox, oy = ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75))[k % 4] if samples > 1 else (0.5, 0.5)   # stratified offsets
        u = (px + F(ox)) / F(w)
        v = (py + F(oy)) / F(h)
        d = (cam["lower_left"][None] + u[:, None] * cam["horizontal"][None] + v[:, None] * cam["vertical"][None] - cam["position"][None]).astype(F)
        rays = np.concatenate([np.tile(cam["position"], (w * h, 1)), d], axis=1).astype(F)
        tr = oracle.trace(sd, rays, use_bvh=s["use_bvh"])
        hit = np.zeros(w * h, _lib.HIT_DTYPE)
        ok = tr[:, 0] > 0
        hit["object"] = np.where(ok, 0, A.FW_NO_HIT)
        hit["t"] = np.where(ok, tr[:, 1], 0)
        hit["point"] = np.where(ok[:, None], tr[:, 2:5], 0)
        hit["normal"] = np.where(ok[:, None], tr[:, 5:8], 0)
        hit["material"] = np.where(ok, tr[:, 8], 0).astype(np.uint32)
        hit["u"] = np.where(ok, tr[:, 9], 0)
        per.append((rays, hit))
    return R.aovs_from_hits(sd, per, oracle)


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def _frame_with_moments(oracle, scene, r, n):
    """an n-sample frame as the mean of n one-sample oracle renders under different seeds, with fw_render_adaptive's moments layout"""
    s_sum = q_sum = None
    for k in range(n):
        x = oracle.render(scene, r.samples(1).seed(100 + k)).linear.astype(F)
        s_sum = x if s_sum is None else (s_sum + x).astype(F)
        q_sum = x * x if q_sum is None else (q_sum + x * x).astype(F)
    r.seed(0)
    return (s_sum / F(n)).astype(F), np.concatenate([q_sum, np.full((len(q_sum), 1), n, F)], axis=1)


# Measured on this test's inputs (cornell_box 128 x 128, 16 spp with moments, AOVs of 4 stratified samples, L = 5): denoised / raw
# RMSE 0.294, mean brightness -0.15 %.  The bounds keep a margin.
QUALITY_RATIO = 0.4
BRIGHTNESS_SHIFT = 0.02


@pytest.mark.slow
def test_quality_on_oracle_renders(oracle):
    scene, r = scenes.cornell_box()
    r.width(128).height(128)
    color, moments = _frame_with_moments(oracle, scene, r, 16)
    hi = oracle.render(scene, r.samples(1024))
    aov = _oracle_aovs(oracle, scene, r, 4)
    _, raw_gamma, _ = R.resolve(color)
    lin, gam, _ = R.denoise(color, aov, moments, 128, 128, R.ITERATIONS, 2.2)
    raw_err, dn_err = _rmse(raw_gamma, hi.gamma), _rmse(gam, hi.gamma)
    assert dn_err <= QUALITY_RATIO * raw_err, (dn_err, raw_err)
    m_raw, m_dn = float(color.astype(np.float64).mean()), float(lin.astype(np.float64).mean())
    assert abs(m_dn - m_raw) <= BRIGHTNESS_SHIFT * m_raw, (m_dn, m_raw)
