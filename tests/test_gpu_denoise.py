"""GPU checks of fw_render_aovs and fw_denoise on the MI355X: the guide buffers equal their composition from the library's own ray queries
(tests/denoise_ref.py) bit for bit, the filter equals the numpy restatement to float32 accuracy, L = 0 is fw_render's frame bit for bit,
calls are deterministic and the device path equals the host path, the denoised frame's quality, and renders left unchanged."""
import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes

import denoise_ref as R
from test_denoise_cpu import _synthetic

pytestmark = pytest.mark.gpu

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _scene(name, w, h):
    if name == "conics":
        return scenes.config("conics", w, h, 1)
    if name == "C4a_hdri_test":                       # a small HDR keeps the oracle's per-miss env_sample cheap; the misses are the point
        scene, r = scenes.config(name, w, h, 1)
        return scenes.hdri_test(scenes.synthetic_hdr(64, 32))[0], r
    return scenes.config(name, w, h, 1)


AOV_CASES = [("C1_random_spheres", 8, None), ("C2_cornell_box", 8, None), ("C3_suzanne", 8, None), ("conics", 8, None),
             ("C4a_hdri_test", 8, None), ("C4b_volume_test", 1, False), ("C4b_volume_test", 1, True), ("C5_part2_all", 1, False),
             ("C5_part2_all", 1, True)]


@pytest.mark.parametrize("name,samples,use_bvh", AOV_CASES, ids=[f"{n}-S{s}-bvh{b}" for n, s, b in AOV_CASES])
def test_aovs_equal_their_composition(oracle, name, samples, use_bvh):
    w, h = 24, 20
    scene, r = _scene(name, w, h)
    if use_bvh is not None:
        r.use_bvh(use_bvh)
    r.seed(7)
    sd = scene.to_desc()
    ds = _lib.DeviceScene(sd, 0)
    try:
        got = ds.aovs(r, samples)
        st = ds.aovs_stats
        want = R.aovs_composed(ds, sd, r, samples, oracle)
    finally:
        ds.close()
    assert got.shape == (w * h, 12)
    bad = np.nonzero(np.any(_u32(got) != _u32(want), axis=1))[0]
    assert bad.size == 0, (name, bad[:8], got[bad[:2]], want[bad[:2]])
    assert st["rays"] > 0 and st["n_batches"] >= samples
    assert float(got[:, 3].max()) > 0                             # something was hit


def _check_close(gpu, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(gpu))
    err = np.abs(gpu.astype(np.float64) - ref)
    tol = 1e-4 * np.abs(ref) + 1e-6
    worst = np.max(np.where(fin, err - tol, -1.0))
    assert worst <= 0, float(worst)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 300), (257, 129), (256, 256)])
def test_denoise_matches_restatement_synthetic(w, h):
    color, aov, mom = _synthetic(h, w, seed=w * 1000 + h)
    if w * h > 16:
        color[3] = np.nan
        color[11, 2] = np.inf
        color[w * h // 2, 0] = -np.inf
        aov[::13, 3] = 0
    for L in (1, 2, 5, 10):
        for m in (None, mom):
            _, _, lin = _lib.denoise(color, aov, m, w, h, L, 2.2)
            ref = R.filtered_linear(color, aov, m, w, h, L)
            _check_close(lin, ref)


def test_denoise_matches_restatement_on_renders():
    scene, r = scenes.config("C2_cornell_box", 96, 80, 16)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        res = ds.render_adaptive(r, 1.0, 16)
        aov = ds.aovs(r, 4)
    finally:
        ds.close()
    for L in (1, 5, 10):
        for m in (None, res.moments):
            _, _, lin = _lib.denoise(res.linear, aov, m, 96, 80, L, 2.2)
            _check_close(lin, R.filtered_linear(res.linear, aov, m, 96, 80, L))


@pytest.mark.parametrize("name", ["C2_cornell_box", "C4a_hdri_test"])
def test_zero_iterations_is_the_render(name):
    scene, r = scenes.config(name, 64, 48, 8)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        ref = ds.render(r)
        aov = ds.aovs(r, 2)
    finally:
        ds.close()
    rgb8, gam, lin = _lib.denoise(ref.linear, aov, None, 64, 48, 0, r.settings["gamma"])
    assert np.array_equal(_u32(lin), _u32(ref.linear))
    assert np.array_equal(_u32(gam), _u32(ref.gamma))
    assert np.array_equal(rgb8, ref.rgb8)


def test_deterministic_and_device_path():
    import torch
    w, h = 257, 129
    color, aov, mom = _synthetic(h, w, seed=3)
    a = _lib.denoise(color, aov, mom, w, h, 5, 2.2)
    b = _lib.denoise(color, aov, mom, w, h, 5, 2.2)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        tc, ta, tm = (torch.from_numpy(x).to(dev) for x in (color, aov, mom))
        d8, dg, dl = _lib.denoise(tc, ta, tm, w, h, 5, 2.2)
    side.synchronize()
    assert np.array_equal(d8.cpu().numpy(), a[0])
    assert np.array_equal(_u32(dg.cpu().numpy()), _u32(a[1]))
    assert np.array_equal(_u32(dl.cpu().numpy()), _u32(a[2]))
    # device AOVs equal the host ones
    scene, r = scenes.config("C2_cornell_box", 40, 30, 4)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        host = ds.aovs(r, 3)
        out = torch.empty((40 * 30, 12), dtype=torch.float32, device=dev)
        with torch.cuda.stream(side):
            ds.aovs(r, 3, out=out, stream=side.cuda_stream)
        assert np.array_equal(_u32(out.cpu().numpy()), _u32(host))
    finally:
        ds.close()


def test_denoised_quality():
    scene, r = scenes.config("C2_cornell_box", 256, 256, 16)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        dn = r.render_denoised(ds, iterations=5, aov_samples=8)
        ref = ds.render(scenes.config("C2_cornell_box", 256, 256, 4096)[1])
    finally:
        ds.close()
    from test_denoise_cpu import BRIGHTNESS_SHIFT, QUALITY_RATIO, _rmse
    raw_err, dn_err = _rmse(dn.raw.gamma, ref.gamma), _rmse(dn.gamma, ref.gamma)
    print(f"C2 256x256 @16: raw RMSE {raw_err:.4f}, denoised {dn_err:.4f} (ratio {dn_err / raw_err:.3f})")
    assert dn_err <= QUALITY_RATIO * raw_err, (dn_err, raw_err)
    m_raw, m_dn = float(dn.raw.linear.astype(np.float64).mean()), float(dn.linear.astype(np.float64).mean())
    assert abs(m_dn - m_raw) <= BRIGHTNESS_SHIFT * m_raw, (m_dn, m_raw)
    # the raw frame is fw_render's at 16 samples
    plain = _lib.render_scene(scene.to_desc(), r)
    assert np.array_equal(dn.raw.rgb8, plain.rgb8) and np.array_equal(_u32(dn.raw.linear), _u32(plain.linear))


def test_renders_unchanged_by_aovs_and_denoise():
    for name in ("C2_cornell_box", "C4b_volume_test"):
        scene, r = scenes.config(name, 64, 64, 8)
        ds = _lib.DeviceScene(scene.to_desc(), 0)
        try:
            before = ds.render(r)
            aov = ds.aovs(r, 4)
            _lib.denoise(before.linear, aov, None, 64, 64, 5, 2.2)
            after = ds.render(r)
        finally:
            ds.close()
        assert np.array_equal(before.rgb8, after.rgb8)
        assert np.array_equal(_u32(before.linear), _u32(after.linear)) and np.array_equal(_u32(before.gamma), _u32(after.gamma))
