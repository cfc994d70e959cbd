"""GPU checks of temporal accumulation (fw_temporal): k_tp_reproject against the numpy restatement (tests/temporal_ref.py)
on synthetic and rendered frame pairs, the projection convention against fw_camera_rays, the static identity against a render of all the
samples, the first frame, determinism and the device path, motion and disocclusion, renders left unchanged, and render_sequence's
quality against per-view denoising."""
import copy

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes

import temporal_ref as R
from test_denoise_cpu import BRIGHTNESS_SHIFT, _rmse
from test_temporal_cpu import GPU_SYNTHETIC_CASES, MAX_EXCLUDED_SHARE

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _check_close(gpu, ref, keep):
    """test_gpu_denoise's tolerance (1e-4 relative + 1e-6) on the pixels in `keep`"""
    gpu, ref = np.asarray(gpu)[keep], np.asarray(ref)[keep]
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(gpu))
    err = np.abs(gpu.astype(np.float64) - ref)
    tol = 1e-4 * np.abs(ref) + 1e-6
    worst = np.max(np.where(fin, err - tol, -1.0)) if ref.size else -1.0
    assert worst <= 0, float(worst)


def _against_restatement(color, moments, aov, history, prev_pos, w, h, cam, prev_cam, samples, max_history):
    oc, om, oh = _lib.temporal(color, aov, moments, history, prev_pos, w, h, cam, prev_cam, samples, max_history)
    rc, rm, rh, near = R.temporal(color, moments, aov, history, prev_pos, w, h, prev_cam, samples, max_history)
    share = float(near.mean())
    print(f"{w}x{h}: {share:.4%} of the pixels within {R.NEAR} of a threshold in the restatement, carried over on {(rh > 0).mean():.1%}")
    assert share <= MAX_EXCLUDED_SHARE, share
    keep = ~near
    _check_close(oc, rc, keep); _check_close(om, rm, keep); _check_close(oh, rh, keep)
    return oc, om, oh


@pytest.mark.parametrize("w,h,seed", GPU_SYNTHETIC_CASES)
def test_temporal_matches_restatement_synthetic(w, h, seed):
    c = R.synthetic_case(w, h, seed=seed)
    for mom, cap in ((c["moments"], 40.0), (c["moments"], INF), (None, 40.0)):
        _against_restatement(c["color"], mom, c["aov"], c["history"], None, w, h, c["camera"], c["prev_camera"], 16, cap)
    # a prev_position of the caller's: the surface points moved by a fraction of a pixel between the frames
    moved = (c["aov"][:, 8:11] + F(0.004)).astype(F)
    _against_restatement(c["color"], c["moments"], c["aov"], c["history"], moved, w, h, c["camera"], c["prev_camera"], 16, 40.0)


def _orbit_pair(name, w, h, spp, use_bvh, step):
    """two consecutive frames of an orbit of `step` views per turn: (cams, per-frame (linear, moments, aov))"""
    scene, r = scenes.config(name, w, h, spp)
    if use_bvh is not None:
        r.use_bvh(use_bvh)
    cams = api.orbit_cameras(r._camera, step)[:2]
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    frames = []
    try:
        for k, cam in enumerate(cams):
            rk = copy.copy(r); rk.settings = dict(r.settings); rk.settings["seed"] = 5 + k; rk._camera = cam
            res = ds.render_adaptive(rk, 1.0, spp)
            frames.append((res.linear, res.moments, ds.aovs(rk, 4)))
    finally:
        ds.close()
    return cams, frames


@pytest.mark.parametrize("name,use_bvh", [("C2_cornell_box", None), ("C3_suzanne", True)])
def test_temporal_matches_restatement_on_renders(name, use_bvh):
    w, h = 96, 80
    cams, frames = _orbit_pair(name, w, h, 16, use_bvh, 360)                      # one degree per frame
    (c0, m0, a0), (c1, m1, a1) = frames
    first = _lib.temporal(c0, a0, m0, None, None, w, h, cams[0], None, 16, INF)
    oc, om, oh = _against_restatement(c1, m1, a1, (first[0], first[1], a0), None, w, h, cams[1], cams[0], 16, INF)
    assert (oh > 0).mean() > 0.5                                                   # most of the frame found its history


def test_projection_convention():
    """Every ray of fw_camera_rays, at any distance, projects back to within half a pixel of its own pixel — through the kernel: a history
    whose colour is the pixel's own column and row comes back at its own pixel."""
    for name in ("C2_cornell_box", "C3_suzanne"):
        w, h = 52, 36
        _scene, r = scenes.config(name, w, h, 1)
        cam = r._camera
        n = w * h
        idx = np.arange(n)
        col, row = (idx % w).astype(F), (idx // w).astype(F)
        hist_aov = np.zeros((n, 12), F)
        basis = R.camera_basis(cam, w, h)
        # unit coverage; the points at one t lie in a plane across the view direction, so that is the normal; positions: see below
        hist_aov[:, 0:3], hist_aov[:, 3], hist_aov[:, 4:7] = 0.5, 1, basis["w"]
        hist_c = np.stack([col, row, np.zeros(n, F)], axis=1)
        hist_m = np.concatenate([hist_c * hist_c, np.ones((n, 1), F)], axis=1)
        ts = (1.0,) if cam.to_abi().aperture > 0 else (0.25, 1.0, 40.0)            # a lens: only the focus plane (t = 1) is sharp
        for s in (0, 1, 7):
            rays = _lib.camera_rays(r, s)
            for t in ts:
                X = (rays[:, 0:3].astype(np.float64) + t * rays[:, 3:6].astype(np.float64)).astype(F)
                x, y, depth = R.project(basis, X, w, h)                             # the restatement's projection ...
                assert np.all(depth > 0)
                assert np.abs(x - col).max() <= 0.5 + 1e-3 and np.abs(y - row).max() <= 0.5 + 1e-3, (name, s, t)
                aov = hist_aov.copy()
                aov[:, 8:11] = X
                ha = hist_aov.copy()
                ha[:, 8:11] = X                                                     # the same surface, so the plane test passes everywhere
                cur = np.zeros((n, 3), F)
                oc, om, oh = _lib.temporal(cur, aov, None, (hist_c, hist_m, ha), None, w, h, cam, cam, 1, INF)
                inner = (col >= 1) & (col <= w - 2) & (row >= 1) & (row <= h - 2)   # all four taps inside the image
                assert np.abs(oh[inner] - 1).max() <= 1e-6
                got = 2.0 * oc.astype(np.float64)                                   # n_h = n_c = 1 and a current colour of 0: the mean history
                assert np.abs(got[inner, 0] - col[inner]).max() <= 0.5 + 1e-3 and np.abs(got[inner, 1] - row[inner]).max() <= 0.5 + 1e-3
                assert np.allclose(got[inner, 0], x[inner], atol=5e-3) and np.allclose(got[inner, 1], y[inner], atol=5e-3)


def _centre_guides(ds, r, aov):
    """`aov` with normal, distance and position from the ray through each pixel's centre (coverage 0 where it misses): guides under which
    an unmoved camera projects every pixel onto itself"""
    w, h = r.settings["width"], r.settings["height"]
    b = R.camera_basis(r._camera, w, h)
    idx = np.arange(w * h)
    u, v = (idx % w + 0.5) / w, (h - idx // w + 0.5) / h
    d = -b["w"][None] + ((2 * u - 1) * b["half_width"])[:, None] * b["u"][None] + ((2 * v - 1) * b["half_height"])[:, None] * b["v"][None]
    rays = np.concatenate([np.tile(b["pos"], (w * h, 1)), d], axis=1).astype(F)
    hits = ds.trace(rays, r.settings["use_bvh"], seed=r.settings["seed"])
    ok = hits["object"] != A.FW_NO_HIT
    out = aov.copy()
    nl = np.linalg.norm(hits["normal"], axis=1)
    out[:, 3] = np.where(ok & (nl > 0), 1.0, 0.0)
    out[:, 4:7] = np.where(ok[:, None], hits["normal"] / np.where(nl > 0, nl, 1)[:, None], 0)
    out[:, 7] = np.where(ok, hits["t"] * np.linalg.norm(rays[:, 3:6], axis=1), 0)
    out[:, 8:11] = np.where(ok[:, None], hits["point"], 0)
    return out


@pytest.mark.parametrize("S,with_moments", [(16, True), (1, False)])
def test_static_identity(S, with_moments):
    """K slices of S samples of one seed, merged under an unmoved camera, are the render of all K S samples."""
    K, w, h = 4, 64, 48
    scene, r = scenes.config("C2_cornell_box", w, h, K * S)
    r.seed(3)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        full = ds.render(r)
        aov = _centre_guides(ds, r, ds.aovs(r, 4))
        rs = copy.copy(r); rs.settings = dict(r.settings); rs.settings["samples"] = S
        hist = None
        for k in range(K):
            acc = np.zeros((w * h, 4), F)
            ds.render_progressive(rs, k * S, acc)                                   # samples [k S, (k + 1) S) alone
            lin = (acc[:, 0:3] / F(S)).astype(F)
            mom = None
            if with_moments:      # (fw_render_adaptive has no first sample to match a later slice: the statement's substitute, as an array)
                mom = np.concatenate([F(S) * (lin * lin), np.full((w * h, 1), S, F)], axis=1).astype(F)
            oc, om, oh = _lib.temporal(lin, aov, mom, hist, None, w, h, r._camera, r._camera, S, INF)
            hist = (oc, om, aov)
    finally:
        ds.close()
    covered = aov[:, 3] != 0
    assert covered.mean() > 0.5
    assert np.all(om[covered, 3] == K * S) and np.all(oh[covered] == (K - 1) * S)
    err = np.abs(oc[covered].astype(np.float64) - full.linear[covered]) - (1e-5 * np.abs(full.linear[covered]) + 1e-7)
    assert err.max() <= 0, float(err.max())


def test_first_frame_bit_for_bit():
    c = R.synthetic_case(257, 129, seed=21)
    oc, om, oh = _lib.temporal(c["color"], c["aov"], c["moments"], None, None, 257, 129, c["camera"], None, 16, 8.0)
    assert np.array_equal(_u32(oc), _u32(c["color"])) and np.array_equal(_u32(om), _u32(c["moments"])) and not oh.any()
    oc, om, oh = _lib.temporal(c["color"], c["aov"], None, None, None, 257, 129, c["camera"], None, 3, 8.0)
    col = c["color"]
    with np.errstate(all="ignore"):
        want = np.concatenate([F(3) * (col * col), np.full((len(col), 1), 3, F)], axis=1).astype(F)
    assert np.array_equal(_u32(oc), _u32(col)) and np.array_equal(_u32(om), _u32(want)) and not oh.any()


def test_deterministic_and_device_path():
    import torch
    w, h = 257, 129
    c = R.synthetic_case(w, h, seed=22)
    args = (c["color"], c["aov"], c["moments"], c["history"], None, w, h, c["camera"], c["prev_camera"], 16, 40.0)
    a, b = _lib.temporal(*args), _lib.temporal(*args)
    for x, y in zip(a, b):
        assert np.array_equal(_u32(x), _u32(y))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        up = lambda x: torch.from_numpy(x).to(dev)
        d = _lib.temporal(up(c["color"]), up(c["aov"]), up(c["moments"]), tuple(up(x) for x in c["history"]), None, w, h, c["camera"],
                          c["prev_camera"], 16, 40.0)
    side.synchronize()
    for x, y in zip(d, a):
        assert np.array_equal(_u32(x.cpu().numpy()), _u32(y))


def _cornell_with_sphere(x):
    scene, r = scenes.cornell_box()
    m = scene.add_material(api.LambertianMat.with_color((0.7, 0.3, 0.3)))
    scene.add_object(api.RenderObject.new(api.Sphere.new(60.0, m)).position(x, 330.0, 150.0))
    return scene, r


def _erode(mask, times):
    """`mask` (H, W) without the pixels within `times` pixels of its complement or of the image border"""
    m = mask.copy()
    for _ in range(times):
        e = m.copy()
        e[1:] &= m[:-1]; e[:-1] &= m[1:]; e[:, 1:] &= m[:, :-1]; e[:, :-1] &= m[:, 1:]
        e[0] = e[-1] = False; e[:, 0] = e[:, -1] = False
        m = e
    return m


def test_disocclusion_and_motion():
    w, h, S = 96, 96, 8
    scene, r = _cornell_with_sphere(200.0)
    r.width(w).height(h).samples(S)
    sphere = len(scene.render_objects) - 1
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        f0 = ds.render_adaptive(r, 1.0, S)
        a0 = ds.aovs(r, 4)
        g0 = r.gbuffer(ds)
        before = ds._desc
        scene.render_objects[sphere].position(330.0, 330.0, 150.0)                  # sideways by about two diameters
        ds.update(scene)
        r1 = copy.copy(r); r1.settings = dict(r.settings); r1.settings["seed"] = 1
        f1 = ds.render_adaptive(r1, 1.0, S)
        a1 = ds.aovs(r1, 4)
        g1 = r1.gbuffer(ds)
        after = ds._desc
    finally:
        ds.close()
    first = _lib.temporal(f0.linear, a0, f0.moments, None, None, w, h, r._camera, None, S, INF)
    hist = (first[0], first[1], a0)
    prev = api.previous_positions(a1[:, 8:11], g1["object"].reshape(-1), before, after)
    _, _, oh_moved = _lib.temporal(f1.linear, a1, f1.moments, hist, prev, w, h, r._camera, r._camera, S, INF)
    _, _, oh_static = _lib.temporal(f1.linear, a1, f1.moments, hist, None, w, h, r._camera, r._camera, S, INF)
    on0, on1 = g0["object"] == sphere, g1["object"] == sphere
    inner = _erode(on1, 2).reshape(-1) & (a1[:, 3] == 1)                               # the sphere's interior in frame 1
    assert inner.sum() >= 20
    assert (oh_moved[inner] > 0).mean() >= 0.9, float((oh_moved[inner] > 0).mean())     # with its motion the sphere keeps its history
    assert not oh_static[inner].any()                                                  # without, it loses it (or finds the wall's: rejected)
    # the wall the sphere uncovered: pixels that showed the sphere in frame 0 and do not in frame 1
    # (two pixels inside frame 0's silhouette: no bilinear tap reaches the wall beside it)
    uncovered = (_erode(on0, 2) & ~on1).reshape(-1) & (a1[:, 3] == 1)
    assert uncovered.sum() >= 20
    assert not oh_moved[uncovered].any() and not oh_static[uncovered].any()


def test_renders_unchanged_by_temporal():
    scene, r = scenes.config("C2_cornell_box", 64, 64, 8)
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        before = ds.render(r)
        again = ds.render(r)                                                          # asked for twice in a row: the frame graph from here on
        aov = ds.aovs(r, 4)
        first = _lib.temporal(before.linear, aov, None, None, None, 64, 64, r._camera, None, 8, INF)
        _lib.temporal(before.linear, aov, None, (first[0], first[1], aov), None, 64, 64, r._camera, r._camera, 8, INF)
        after = [ds.render(r) for _ in range(3)]
    finally:
        ds.close()
    for x in [again] + after:
        assert np.array_equal(before.rgb8, x.rgb8)
        assert np.array_equal(_u32(before.linear), _u32(x.linear)) and np.array_equal(_u32(before.gamma), _u32(x.gamma))


# Measured (profiles/temporal.txt): render_sequence / render_denoised RMSE of the last of 8 views of a 36-per-turn cornell
# orbit, 256 x 256 at 16 spp, against 4096 spp = MEASURED_RATIO.  The bound is the geometric mean of the measured ratio and 1.
MEASURED_RATIO = 0.8022
QUALITY_RATIO = float(np.sqrt(MEASURED_RATIO * 1.0))


def test_sequence_quality_and_plain_sequence():
    w = h = 256
    scene, r = scenes.config("C2_cornell_box", w, h, 16)
    cams = api.orbit_cameras(r._camera, 36)[:8]
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        seq = list(r.render_sequence(ds, cams))
        plain = list(r.render_sequence(ds, cams, temporal=False))
        per_view = []
        for k, cam in enumerate(cams):
            rk = copy.copy(r); rk.settings = dict(r.settings); rk.settings["seed"] = r.settings["seed"] + k; rk._camera = cam
            per_view.append(rk.render_denoised(ds))
        rr = scenes.config("C2_cornell_box", w, h, 4096)[1]
        rr._camera = cams[-1]
        ref = ds.render(rr)
    finally:
        ds.close()
    for a, b in zip(plain, per_view):                                                 # temporal=False: render_denoised of each view, bit for bit
        assert np.array_equal(a.rgb8, b.rgb8) and np.array_equal(_u32(a.linear), _u32(b.linear)) and np.array_equal(_u32(a.gamma), _u32(b.gamma))
        assert np.array_equal(_u32(a.raw.linear), _u32(b.raw.linear))
    assert np.array_equal(_u32(seq[0].linear), _u32(per_view[0].linear))              # a first frame has no history
    tp_err, dn_err = _rmse(seq[-1].gamma, ref.gamma), _rmse(per_view[-1].gamma, ref.gamma)
    print(f"C2 orbit 256x256 @16, view 7: render_sequence RMSE {tp_err:.5f}, render_denoised {dn_err:.5f} (ratio {tp_err / dn_err:.3f}), "
          f"mean history {seq[-1].stats['history_mean']:.1f}")
    assert tp_err <= QUALITY_RATIO * dn_err, (tp_err, dn_err)
    m_raw, m_tp = float(seq[-1].raw.linear.astype(np.float64).mean()), float(seq[-1].linear.astype(np.float64).mean())
    assert abs(m_tp - m_raw) <= BRIGHTNESS_SHIFT * m_raw, (m_tp, m_raw)
