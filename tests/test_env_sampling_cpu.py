"""Environment sampling (FW_FLAG_ENV_SAMPLING) without a GPU: the public switch (the flag's value in the header and in _abi,
Renderer.env_sampling, the CLI) and the float64 restatement the GPU tests measure the device against — env_sample's texel lookup, the rows'
solid angles, the texel densities and the floor quadrature of the known-answer probes."""
import os
import re
import subprocess
import sys

import numpy as np

from firework_amd import _abi as A
from firework_amd.api import Renderer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import env_dist_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def test_flag_matches_header():
    hdr = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    m = re.search(r"#define FW_FLAG_ENV_SAMPLING (\d+)u", hdr)
    assert m and int(m.group(1)) == A.FW_FLAG_ENV_SAMPLING == 8
    assert int(re.search(r"#define FW_ENV_SAMPLE_FLOATS (\d+)", hdr).group(1)) == A.FW_ENV_SAMPLE_FLOATS
    assert int(re.search(r"#define FW_ABI_VERSION (\d+)", hdr).group(1)) == A.FW_ABI_VERSION == 8
    for name in ("fw_selftest_env_dist", "fw_selftest_env_sample"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_renderer_switch():
    r = Renderer.default().light_sampling()
    r.env_sampling()
    assert r.to_params().flags == A.FW_FLAG_LIGHT_SAMPLING | A.FW_FLAG_ENV_SAMPLING
    r.env_sampling(False)
    assert r.to_params().flags == A.FW_FLAG_LIGHT_SAMPLING
    r.light_sampling(False).env_sampling(True)
    assert r.to_params().flags == A.FW_FLAG_ENV_SAMPLING


def test_cli_accepts_flag():
    out = subprocess.run([sys.executable, "-m", "firework_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--env-sampling" in out.stdout and "--light-sampling" in out.stdout
    src = open(os.path.join(ROOT, "firework_amd", "__main__.py")).read()
    assert ".env_sampling(opt.env_sampling)" in src


def test_cpp_header_switch():
    src = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "Renderer env_sampling(bool on = true)" in src and "FW_FLAG_ENV_SAMPLING" in src


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_omega_sums_to_4pi():
    for w, h in ((1, 1), (3, 5), (64, 32), (4096, 2048)):
        om = R.omega_row(w, h)
        assert (om > 0).all()
        assert abs(om.sum() * w - 4 * np.pi) <= 1e-12 * 4 * np.pi


def _texel64(d, w, h):
    """the texel in exact arithmetic: u = 1 - (phi + pi) / 2 pi, 1 - v = (pi / 2 - theta) / pi"""
    d = np.asarray(d, np.float64)
    phi, theta = np.arctan2(d[:, 2], d[:, 0]), np.arcsin(np.clip(d[:, 1], -1, 1))
    u, omv = 1 - (phi + np.pi) / (2 * np.pi), (np.pi / 2 - theta) / np.pi
    return np.floor(omv * h).astype(np.int64), np.floor(u * w).astype(np.int64)


def test_lookup_matches_sphere_uv_on_random_directions():
    rng = np.random.default_rng(7)
    d = rng.normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    for w, h in ((4096, 2048), (3, 5), (1, 1)):
        y, x = _texel64(d, w, h)
        want = np.minimum(y * w + x, w * h - 1)
        got = R.env_texel(d, w, h)
        bad = got != want
        assert bad.mean() <= 1e-3, (w, h, bad.mean())                  # (float32 atan2 / asin near an edge: 2e-4 of them at 4096 x 2048)
        dy, dx = np.abs(got[bad] // w - want[bad] // w), np.abs(got[bad] % w - want[bad] % w)
        assert ((dy <= 1) & ((dx <= 1) | (dx == w - 1))).all()      # float32 rounding at an edge: a neighbour (or across the seam)
        # the region of a texel is where its index comes back: directions drawn inside texels far from their edges find them
        yy, xx = rng.integers(0, h, 1000), rng.integers(0, w, 1000)
        hi, lo = R.row_bounds(h)
        s = lo[yy] + (0.25 + 0.5 * rng.random(1000)) * (hi[yy] - lo[yy])
        ph = np.pi * (1 - 2 * (xx + 0.25 + 0.5 * rng.random(1000)) / w)
        c = np.sqrt(1 - s * s)
        dd = np.stack([c * np.cos(ph), s, c * np.sin(ph)], 1)
        assert np.array_equal(R.env_texel(dd, w, h), yy * w + xx)


def test_lookup_at_poles_and_seam():
    w, h = 64, 32
    assert R.env_texel([[0, 1, 0]], w, h)[0] == w // 2                 # atan2(0, 0) = 0: u = 1/2 in row 0
    assert R.env_texel([[0, -1, 0]], w, h)[0] == w * h - 1             # v = 0: row h, clamped to the last texel
    seam = np.array([[-1, 0, -0.0]], np.float32)                       # atan2(-0, -1) = -pi: u = 1, x = w, the next row's first texel
    assert R.env_texel(seam, w, h)[0] == (h // 2 + 1) * w
    assert R.env_texel(np.array([[-1, 0, 0.0]], np.float32), w, h)[0] == (h // 2) * w      # atan2(+0, -1) = pi: u = 0


def test_table_density():
    rng = np.random.default_rng(3)
    m = rng.random((5, 3, 3)).astype(np.float32)
    m[1, 2] = [-1.0, np.nan, np.inf]                                   # counts as 0
    m[4, 0] = [-2.0, 0.5, -1.0]                                        # counts as 0.5
    p, dens, tot = R.table(m)
    assert p[1, 2] == 0 and dens[1, 2] == 0
    assert abs(p.sum() - 1) <= 1e-12
    om = R.omega_row(3, 5)
    assert np.allclose(dens * om[:, None], p)
    assert abs(p[4, 0] - 0.5 * om[4] / tot) <= 1e-15
    assert abs((dens * om[:, None]).sum() - 1) <= 1e-12                # the density integrates to 1 over the sphere


# ---- the quadrature ---------------------------------------------------------------------------------------------------------------------
def test_uniform_map_integrates_bsdf_density_to_one():
    for w, h in ((1, 1), (3, 5), (64, 32), (4096, 2048)):
        assert abs(R.texel_cos3(w, h).sum() * w - 1) <= 1e-12         # int over the upper hemisphere of 2 cos^3 / pi = 1
        mean, var = R.floor_answer(np.ones((h, w, 3), np.float32), 0.5)
        assert np.allclose(mean, 0.5) and np.allclose(var, 0.0, atol=1e-12)


def test_quadrature_against_a_fine_grid():
    w, h = 8, 6
    hi, lo = R.row_bounds(h)
    n = 400
    for y in range(h):
        s = lo[y] + (np.arange(n) + 0.5) / n * (hi[y] - lo[y])
        brute = (2 * np.pi / w) * np.mean(2 * np.maximum(s, 0) ** 3 / np.pi) * (hi[y] - lo[y])
        assert abs(brute - R.texel_cos3(w, h)[y]) <= 1e-5 * max(R.texel_cos3(w, h).max(), 1e-30)
    m = np.zeros((h, w, 3), np.float32)
    m[1, 3] = [2.0, 4.0, 6.0]
    mean, var = R.floor_answer(m, 0.5)
    I = R.texel_cos3(w, h)[1]
    assert np.allclose(mean, 0.5 * np.array([2, 4, 6]) * I)
    assert np.allclose(var, 0.25 * np.array([4, 16, 36]) * I * (1 - I))    # a Bernoulli draw of the texel
