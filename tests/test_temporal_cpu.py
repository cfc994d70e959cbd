"""CPU-side checks of temporal accumulation (fw_temporal): the export at ABI 8, the parameter struct's layout, the
constants, every argument error in its stated order, the no-device error, the CLI's --temporal refusals, api.previous_positions, and
the numpy restatement (tests/temporal_ref.py): its identities, the share of near-threshold pixels of the GPU test's synthetic cases,
and its quality on oracle renders of a cornell_box orbit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes

import denoise_ref as D
import temporal_ref as R
from test_denoise_cpu import BRIGHTNESS_SHIFT, _oracle_aovs, _rmse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")


# ---- surface ----------------------------------------------------------------------------------------------------------------------
def test_temporal_export_at_abi_8():
    lib = _lib.load()
    assert hasattr(lib, "fw_temporal")
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    entry_points = text[text.index("/* ---- entry points"):]
    assert re.search(r"\bint fw_temporal\s*\(const fw_temporal_params \*p, const float \*color, const float \*moments, const float \*aov,\s*"
                     r"const float \*hist_color, const float \*hist_moments, const float \*hist_aov, const float \*prev_position,\s*"
                     r"float \*out_color, float \*out_moments, float \*out_history\);", entry_points)


def test_temporal_params_layout(tmp_path):
    fields = [name for name, _ in A.fw_temporal_params._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu", sizeof(fw_temporal_params));\n'
                   + "".join(f'printf(" %zu", offsetof(fw_temporal_params, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(A.fw_temporal_params)
    assert got[1:] == [getattr(A.fw_temporal_params, f).offset for f in fields]


def test_constants_agree():
    """the header, the Python ABI, the restatement and the kernel state the same constants"""
    assert R.header_constants() == dict(NORMAL_COS=R.NORMAL_COS, PLANE=R.PLANE, MIN_TAP=R.MIN_TAP)
    assert (A.FW_TEMPORAL_NORMAL_COS, A.FW_TEMPORAL_PLANE, A.FW_TEMPORAL_MIN_TAP) == (R.NORMAL_COS, R.PLANE, R.MIN_TAP)
    assert R.EPS == D.EPS == A.FW_DENOISE_EPS
    kernel = open(os.path.join(ROOT, "firework_amd", "csrc", "fw_temporal.hip")).read()
    for name in ("FW_DENOISE_EPS", "FW_TEMPORAL_NORMAL_COS", "FW_TEMPORAL_PLANE", "FW_TEMPORAL_MIN_TAP"):
        assert name in kernel
    assert "asm" not in kernel
    assert api.DEFAULT_MAX_HISTORY == __import__("firework_amd.__main__", fromlist=["x"]).TEMPORAL_DEFAULT


def _camera(pos=(0.0, 0.0, 0.0), at=(0.0, 0.0, -1.0)):
    return R._settings(pos, at)


def _params(**kw):
    p = A.fw_temporal_params()
    p.width, p.height, p.samples, p.max_history, p.device = 8, 8, 4, 64.0, 0
    p.camera, p.prev_camera = _camera(), _camera()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _call(p, color, moments, aov, hist=(None, None, None), prev=None, outs=(None, None, None)):
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    return _lib.load().fw_temporal(None if p is None else C.byref(p), ptr(color), ptr(moments), ptr(aov), ptr(hist[0]), ptr(hist[1]), ptr(hist[2]),
                                   ptr(prev), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]))


def test_temporal_argument_checks():
    n = 64
    color, mom, aov = np.zeros((n, 3), F), np.zeros((n + 1, 4), F), np.zeros((n + 1, 12), F)
    hc, hm, ha = np.zeros((n + 1, 3), F), np.zeros((n + 1, 4), F), np.zeros((n + 1, 12), F)
    hist = (hc, hm, ha)
    bad = A.FW_ERR_BAD_ARG
    assert _call(None, color, mom, aov) == bad
    assert _call(_params(), None, mom, aov) == bad
    assert _call(_params(), color, mom, None) == bad
    assert _call(_params(width=0), color, mom, aov) == bad
    assert _call(_params(height=0), color, mom, aov) == bad
    for part in ((hc, None, None), (None, hm, None), (None, None, ha), (hc, hm, None), (hc, None, ha), (None, hm, ha)):
        assert _call(_params(), color, mom, aov, part) == bad
    out_m = np.zeros((n, 4), F)
    assert _call(_params(), color, mom, aov, hist, outs=(hc, None, None)) == bad                   # an output that is a history array
    assert _call(_params(), color, mom, aov, hist, outs=(None, hm, None)) == bad
    assert _call(_params(), color, mom, aov, hist, outs=(None, None, ha.ctypes.data + 48 * (n - 1))) == bad      # ... or overlaps its end
    for mh in (0.0, -1.0, float("nan")):
        assert _call(_params(max_history=mh), color, mom, aov) == bad, mh
    for which in ("camera", "prev_camera"):
        for v in (float("nan"), INF):
            assert _call(_params(**{which: _camera(pos=(v, 0.0, 0.0))}), color, mom, aov) == bad
            c = _camera(); c.vfov = v
            assert _call(_params(**{which: c}), color, mom, aov) == bad
    assert _call(_params(device=-1), color, mom, aov) == bad
    al = lambda a: a.ctypes.data + (16 - a.ctypes.data % 16) % 16
    off = lambda a: al(a) + 4
    assert _call(_params(on_device=1), color, al(mom), off(aov)) == bad
    assert _call(_params(on_device=1), color, off(mom), al(aov)) == bad
    assert _call(_params(on_device=1), color, al(mom), al(aov), (al(hc), off(hm), al(ha))) == bad
    assert _call(_params(on_device=1), color, al(mom), al(aov), (al(hc), al(hm), off(ha))) == bad
    assert _call(_params(on_device=1), color, al(mom), al(aov), (off(hc), al(hm), al(ha))) == bad
    assert _call(_params(samples=0), color, None, aov) == bad
    # the order: every BAD_ARG above comes before UNSUPPORTED, and that before NO_DEVICE
    big = dict(width=1 << 16, height=1 << 16)
    assert _call(_params(max_history=0.0, **big), color, mom, aov) == bad
    assert _call(_params(samples=0, **big), color, None, aov) == bad
    assert _call(_params(**big), color, mom, aov) == A.FW_ERR_UNSUPPORTED
    assert _call(_params(max_history=INF, **big), color, mom, aov) == A.FW_ERR_UNSUPPORTED         # INFINITY is allowed
    assert _call(_params(device=1 << 20), color, mom, aov) == bad
    if _lib.device_count() == 0:
        assert _call(_params(), color, mom, aov) == A.FW_ERR_NO_DEVICE
        assert _call(_params(max_history=INF), color, None, aov, hist, outs=(None, out_m, None)) == A.FW_ERR_NO_DEVICE


def test_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    r.width(8).height(8).samples(4)
    z = lambda c: np.zeros((64, c), F)
    for call in (lambda: _lib.temporal(z(3), z(12), z(4), None, None, 8, 8, r._camera),
                 lambda: next(r.render_sequence(scene, api.orbit_cameras(r._camera, 2)))):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


def test_cli_temporal_refusals(tmp_path, capsys):
    from firework_amd.__main__ import main
    base = ["--scene-file", "s.yml", "-s", "16"]
    frames = ["-o", str(tmp_path / "f{}.png")]
    for extra in (["--progressive", "2"], ["--checkpoint", str(tmp_path / "ck.npz")], ["--adaptive", "0.05"], ["--camera", "panorama"]):
        for tp in (["--temporal"], ["--temporal", "32"]):
            with pytest.raises(SystemExit) as e:
                main(base + frames + ["--orbit", "3"] + tp + extra)
            assert e.value.code == 2
            assert "--temporal" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                    # only with --orbit
        main(base + ["-o", str(tmp_path / "o.png"), "--temporal"])
    assert e.value.code == 2 and "--orbit" in capsys.readouterr().err
    for mh in ("0", "-4", "nan"):
        with pytest.raises(SystemExit) as e:
            main(base + frames + ["--orbit", "3", "--temporal", mh])
        assert e.value.code == 2


# ---- previous_positions -----------------------------------------------------------------------------------------------------------
def test_previous_positions_against_direct_evaluation(oracle):
    def build(pos_a, rot_a):
        s = api.Scene.new()
        m = s.add_material(api.LambertianMat.with_color((0.5, 0.5, 0.5)))
        s.add_object(api.RenderObject.new(api.Sphere.new(1.0, m)).position(0.0, 0.0, 0.0))
        s.add_object(api.RenderObject.new(api.Rect3d.with_size((1.0, 2.0, 3.0), m)).position(*pos_a).rotate(rot_a))
        s.add_object(api.RenderObject.new(api.Sphere.new(0.5, m)).position(4.0, 0.0, 0.0))
        return s
    rot_b, rot_a = api.Rotor3.from_rotation_xz(0.3), api.Rotor3.from_euler_angles(0.2, -0.4, 0.9)
    before = build((1.0, 2.0, 3.0), rot_b).to_desc()
    after_scene = build((1.5, 2.0, 2.0), rot_a)
    after_scene.render_objects[2].position(4.0, 1.0, 0.0)                    # a pure translation
    after = after_scene.to_desc()
    rng = np.random.default_rng(1)
    local = rng.uniform(-1, 1, (40, 3))
    obj = rng.integers(0, 3, 40).astype(np.uint32)
    obj[::9] = A.FW_NO_HIT

    def mat(rotor):                                                            # the oracle's Rotor3::into_matrix: v' = M @ v
        return np.asarray(oracle.rotor_into_matrix(api.Rotor3(rotor.s, rotor.xy, rotor.xz, rotor.yz)), np.float64)

    def place(desc, i, x):
        o = desc.objects[i]
        m = mat(o.rotation)
        m = m if 0.5 * (np.trace(m) - 1) < 0.999 else np.eye(3)
        return m @ x + np.array([o.position.x, o.position.y, o.position.z])
    world_after = np.array([place(after, int(o), x) if o != A.FW_NO_HIT else x for o, x in zip(obj, local)], F)
    # the direct evaluation: invert the current placement (float32 positions in, so in float64 from those), apply the previous one
    want = []
    for o, xw in zip(obj, world_after.astype(np.float64)):
        if o == A.FW_NO_HIT:
            want.append(xw); continue
        oa = after.objects[int(o)]
        ma = mat(oa.rotation)
        ma = ma if 0.5 * (np.trace(ma) - 1) < 0.999 else np.eye(3)
        loc = np.linalg.solve(ma, xw - np.array([oa.position.x, oa.position.y, oa.position.z]))
        want.append(place(before, int(o), loc))
    want = np.array(want)
    got = api.previous_positions(world_after, obj, before, after)
    assert got.dtype == F and got.shape == (40, 3)
    assert np.allclose(got, want, rtol=0, atol=2e-5), float(np.abs(got - want).max())
    still = (obj == 0) | (obj == A.FW_NO_HIT)                                   # the unmoved object and the misses: bit for bit
    assert np.array_equal(got[still], world_after[still])
    moved = obj == 2
    assert np.allclose(got[moved] - world_after[moved], [0.0, -1.0, 0.0], atol=1e-5)
    assert np.array_equal(api.previous_positions(world_after, obj.view(np.int32), before, after), got)      # FW_NO_HIT as -1


# ---- the restatement's identities -------------------------------------------------------------------------------------------------
def _plane_frame(cam, W, H, rng, count=16.0, albedo=None):
    """a fronto-parallel plane z = -5 seen through pixel centres; albedo: a function of the world position"""
    n = W * H
    b = R.camera_basis(cam, W, H)
    idx = np.arange(n)
    u, v = (idx % W + 0.5) / W, (H - idx // W + 0.5) / H
    d = -b["w"][None] + ((2 * u - 1) * b["half_width"])[:, None] * b["u"][None] + ((2 * v - 1) * b["half_height"])[:, None] * b["v"][None]
    X = b["pos"][None] + (-5.0 - b["pos"][2]) / d[:, 2:3] * d
    aov = np.zeros((n, 12), F)
    aov[:, 0:3] = 0.5 if albedo is None else albedo(X)
    aov[:, 3], aov[:, 6], aov[:, 7], aov[:, 8:11] = 1, 1, np.linalg.norm(X - b["pos"], axis=1), X
    color = (aov[:, 0:3] * rng.uniform(0.5, 1.0, (n, 3))).astype(F)
    mom = np.concatenate([count * color.astype(np.float64) ** 2 + rng.uniform(0, 0.1, (n, 3)), np.full((n, 1), count)], axis=1).astype(F)
    return color, mom, aov, X


def test_identity_first_frame():
    c = R.synthetic_case(17, 23, seed=2)
    oc, om, oh, _ = R.temporal(c["color"], c["moments"], c["aov"], None, None, 17, 23, c["prev_camera"])
    assert np.array_equal(oc, c["color"].astype(np.float64), equal_nan=True) and np.array_equal(om, c["moments"].astype(np.float64))
    assert not oh.any()
    oc, om, oh, _ = R.temporal(c["color"], None, c["aov"], None, None, 17, 23, c["prev_camera"], samples=4)
    col = c["color"].astype(np.float64)
    with np.errstate(all="ignore"):
        assert np.array_equal(om[:, 0:3], 4.0 * (col * col), equal_nan=True) and np.all(om[:, 3] == 4)


def test_identity_unmoved_camera_merges_by_counts():
    W, H, K, n = 19, 13, 5, 8.0
    rng = np.random.default_rng(3)
    cam = _camera((0.3, -0.2, 1.0), (0.1, 0.0, -1.0))
    frames = [_plane_frame(cam, W, H, rng, n) for _ in range(K)]
    aov = frames[0][2]
    hist = None
    for k, (color, mom, _a, _x) in enumerate(frames):
        oc, om, oh, _ = R.temporal(color, mom, aov, hist, None, W, H, cam)
        assert np.all(oh == k * n) and np.all(om[:, 3] == (k + 1) * n)                   # one tap of weight 1
        hist = (oc.astype(F), om.astype(F), aov)
    # in float64 end to end (no float32 round trip between the frames): the count-weighted mean to 1e-12
    hist64 = None
    for color, mom, _a, _x in frames:
        oc, om, _, _ = _temporal64(color, mom, aov, hist64, W, H, cam)
        hist64 = (oc, om, aov)
    mean = np.mean([f[0].astype(np.float64) for f in frames], axis=0)
    assert np.all(np.abs(oc - mean) <= 1e-12 * np.abs(mean))
    assert np.allclose(om[:, 0:3], np.sum([f[1][:, 0:3].astype(np.float64) for f in frames], axis=0), rtol=1e-12, atol=0)


def _temporal64(color, mom, aov, hist, W, H, cam, **kw):
    """R.temporal with a float64 history: the restatement converts its inputs to float32 first, which this bypasses"""
    keep = R.F32
    try:
        R.F32 = np.float64
        return R.temporal(color, mom, aov, hist, None, W, H, cam, **kw)
    finally:
        R.F32 = keep


def test_identity_pan_by_whole_pixels():
    W, H, k = 24, 16, 3
    rng = np.random.default_rng(4)
    prev = _camera()
    b = R.camera_basis(prev, W, H)
    pixel = 2 * 5.0 * b["half_width"] / W                                            # a pixel's width on the plane z = -5
    cam = _camera((k * pixel, 0.0, 0.0), (k * pixel, 0.0, -1.0))                    # moved right by k pixels: the image moves left
    albedo = lambda X: 0.5 + 0.4 * np.sign(np.sin(7.0 * X[:, 0:1]) * np.sin(5.0 * X[:, 1:2])) * np.ones(3)      # a checker
    hcol, hmom, haov, _ = _plane_frame(prev, W, H, rng, 16.0, albedo)
    hcol = (haov[:, 0:3] + R.EPS) * F(0.7)                                           # a constant demodulated signal under the texture
    color, mom, aov, _ = _plane_frame(cam, W, H, rng, 16.0, albedo)
    oc, om, oh, near = R.temporal(color, mom, aov, (hcol.astype(F), hmom, haov), None, W, H, prev, max_history=INF)
    x = np.arange(W * H) % W
    src = x + k                                                                       # current column x shows what the history had at x + k
    inside = src < W
    assert np.all(oh[inside] == 16) and not oh[~inside].any()                        # the columns that left the image carry nothing
    mean_h = (oc * 32 - 16 * color.astype(np.float64)) / 16
    demod = mean_h / (aov[:, 0:3].astype(np.float64) + R.EPS)
    assert np.allclose(demod[inside], 0.7, rtol=1e-6), float(np.abs(demod[inside] - 0.7).max())      # the texture is not blurred
    idx = np.arange(W * H)
    assert np.allclose(om[inside, 0:3] - mom[inside, 0:3], 16 * (hmom[idx[inside] + k, 0:3] / 16) *
                       ((aov[inside, 0:3] + R.EPS) / (haov[idx[inside] + k, 0:3] + R.EPS)) ** 2, rtol=1e-5)


def test_identity_projection_inverts_the_oracles_rays(oracle):
    cams = []
    for name in ("C1_random_spheres", "C2_cornell_box", "C3_suzanne"):
        try:
            _s, r = scenes.config(name, 33, 21, 1)
            cams.append(r._camera)
        except Exception:
            pass
    assert len(cams) == 3
    cams.append(api.CameraSettings.default().cam_pos((3.0, 2.0, 7.0)).look_at((0.5, -1.0, 0.0)).field_of_view(55.0).aperture(0.4).focus_dist(6.0))
    W, H = 33, 21
    for cam in cams:
        oc = oracle.camera(cam, W, H)
        basis = R.camera_basis(cam, W, H)
        idx = np.arange(W * H)
        px, row = idx % W, idx // W
        u, v = (px + 0.5) / W, (H - row + 0.5) / H
        d = (oc["lower_left"][None] + u[:, None] * oc["horizontal"][None] + v[:, None] * oc["vertical"][None] - oc["position"][None]).astype(np.float64)
        for t in (0.05, 1.0, 37.5):
            x, y, depth = R.project(basis, oc["position"][None].astype(np.float64) + t * d, W, H)
            assert np.all(depth > 0)
            assert np.abs(x - px).max() <= 1e-4 and np.abs(y - row).max() <= 1e-4, (float(np.abs(x - px).max()), float(np.abs(y - row).max()))
            x32, y32, _ = R.project32(basis, (oc["position"][None].astype(np.float64) + t * d).astype(F), W, H)      # the float32 form agrees
            assert np.abs(x32 - px).max() <= 1e-3 and np.abs(y32 - row).max() <= 1e-3
        assert row.min() == 0 and row.max() == H - 1


def test_identity_edges_reject_taps():
    W, H = 16, 12
    rng = np.random.default_rng(5)
    cam = _camera()
    color, mom, aov, X = _plane_frame(cam, W, H, rng)
    hist_aov = aov.copy()
    col = np.arange(W * H) % W
    hist_aov[col >= 8, 10] -= 2.0                       # the history saw a surface 2 units deeper on the right half: a depth edge
    hist_aov[col < 3, 4:7] = (1.0, 0.0, 0.0)            # ... and another orientation on the left: a normal edge
    oc, om, oh, _ = R.temporal(color, mom, aov, (color, mom, hist_aov), None, W, H, cam)
    ok = (col >= 3) & (col < 8)
    assert np.all(oh[ok] == 16) and not oh[~ok].any()
    assert np.array_equal(oc[~ok], color[~ok].astype(np.float64)) and np.array_equal(om[~ok], mom[~ok].astype(np.float64))


def test_identity_max_history_caps():
    W, H = 9, 7
    rng = np.random.default_rng(6)
    cam = _camera()
    color, mom, aov, _ = _plane_frame(cam, W, H, rng, 16.0)
    hcol, hmom, _a, _x = _plane_frame(cam, W, H, rng, 400.0)
    for cap, want in ((INF, 400.0), (1000.0, 400.0), (64.0, 64.0), (0.5, 0.5)):
        oc, om, oh, _ = R.temporal(color, mom, aov, (hcol, hmom, aov), None, W, H, cam, max_history=cap)
        assert np.all(oh == want) and np.all(om[:, 3] == want + 16)
        assert np.allclose(oc, (want * hcol.astype(np.float64) + 16 * color.astype(np.float64)) / (want + 16), rtol=1e-9)


def test_identity_non_finite_values():
    for W, H, seed in ((40, 30, 7), (64, 33, 8)):
        c = R.synthetic_case(W, H, seed=seed)
        oc, om, oh, _ = R.temporal(c["color"], c["moments"], c["aov"], c["history"], None, W, H, c["prev_camera"])
        col, aov = c["color"].astype(np.float64), c["aov"]
        passes = (aov[:, 3] == 0) | ~np.all(np.isfinite(col), axis=1) | ~np.all(np.isfinite(aov[:, 8:11]), axis=1)
        assert passes.sum() >= 4
        assert np.array_equal(oc[passes], col[passes], equal_nan=True) and np.array_equal(om[passes], c["moments"][passes].astype(np.float64))
        assert not oh[passes].any()
        bad_in = ~np.all(np.isfinite(col), axis=1)
        assert np.all(np.isfinite(oc[~bad_in])) and np.all(np.isfinite(om)) and np.all(np.isfinite(oh))
        assert (oh > 0).mean() > 0.7                                     # ... and the rest of the frame does carry its history
        # a history that is bad everywhere is rejected everywhere
        hc, hm, ha = (a.copy() for a in c["history"])
        hm[:, 3] = 0
        oc2, om2, oh2, _ = R.temporal(c["color"], c["moments"], c["aov"], (hc, hm, ha), None, W, H, c["prev_camera"])
        assert not oh2.any() and np.array_equal(oc2, col, equal_nan=True)


# the synthetic cases of tests/test_gpu_temporal.py: the share of pixels it has to leave out (near a threshold in the restatement alone)
GPU_SYNTHETIC_CASES = ((1, 1, 11), (7, 300, 12), (257, 129, 13))
MAX_EXCLUDED_SHARE = 0.01


def test_gpu_synthetic_cases_stay_clear_of_thresholds():
    for W, H, seed in GPU_SYNTHETIC_CASES:
        c = R.synthetic_case(W, H, seed=seed)
        _oc, _om, oh, near = R.temporal(c["color"], c["moments"], c["aov"], c["history"], None, W, H, c["prev_camera"], max_history=40.0)
        assert near.mean() <= MAX_EXCLUDED_SHARE, (W, H, float(near.mean()))
        if W * H > 1:
            assert 0.5 < (oh > 0).mean() < 1.0 and (oh == 40.0).any() and ((oh > 0) & (oh < 40.0)).any()


# ---- quality on oracle renders ----------------------------------------------------------------------------------------------------
# Measured on this test's inputs (cornell_box 128 x 128, 8 frames of a 36-per-turn orbit at 16 spp, guides of 4 stratified samples, L = 5,
# max_history = api.DEFAULT_MAX_HISTORY): (temporal + filter) / (filter alone) RMSE of the last frame against 1024 spp = MEASURED_RATIO
# (DESIGN.md §9j).  The bound is the geometric mean of the measured ratio and 1: room for seed-to-seed spread, and a failure if the
# benefit is lost.
MEASURED_RATIO = 0.8785
QUALITY_RATIO = float(np.sqrt(MEASURED_RATIO * 1.0))
FRAMES, SPP = 8, 16


def orbit_quality(oracle, max_history=None, frames=FRAMES, size=128, **consts):
    """-> (temporal + filter RMSE, filter-alone RMSE, merged linear mean, raw linear mean, mean carried-over count) of the last frame.
    Frame k's sample j is the oracle's one-sample render under seed 100 + SPP k + j (frame 0: test_quality_on_oracle_renders' own
    seeds 100..115), so that the frames' noise is independent and each has fw_render_adaptive's moments."""
    max_history = api.DEFAULT_MAX_HISTORY if max_history is None else max_history
    scene, r = scenes.cornell_box()
    r.width(size).height(size)
    cams = api.orbit_cameras(r._camera, 36)[:frames]
    hist, prev_cam = None, None
    for k, cam in enumerate(cams):
        r.camera(cam)
        s_sum = q_sum = None
        for j in range(SPP):
            x = oracle.render(scene, r.samples(1).seed(100 + SPP * k + j)).linear.astype(F)
            s_sum = x if s_sum is None else (s_sum + x).astype(F)
            q_sum = x * x if q_sum is None else (q_sum + x * x).astype(F)
        r.seed(0)
        color = (s_sum / F(SPP)).astype(F)
        moments = np.concatenate([q_sum, np.full((len(q_sum), 1), SPP, F)], axis=1)
        aov = _oracle_aovs(oracle, scene, r, 4)
        oc, om, oh, _ = R.temporal(color, moments, aov, hist, None, size, size, prev_cam if prev_cam is not None else cam,
                                   max_history=max_history, **consts)
        hist, prev_cam = (oc.astype(F), om.astype(F), aov), cam
    hi = oracle.render(scene, r.samples(1024))
    _, gam_t, _ = D.denoise(hist[0], aov, hist[1], size, size, D.ITERATIONS, 2.2)
    _, gam_f, _ = D.denoise(color, aov, moments, size, size, D.ITERATIONS, 2.2)
    return (_rmse(gam_t, hi.gamma), _rmse(gam_f, hi.gamma), float(hist[0].astype(np.float64).mean()), float(color.astype(np.float64).mean()),
            float(oh.mean()))


@pytest.mark.slow
def test_quality_on_oracle_orbit(oracle):
    tp_err, dn_err, m_tp, m_raw, n_h = orbit_quality(oracle)
    print(f"temporal + filter {tp_err:.5f}, filter alone {dn_err:.5f}, ratio {tp_err / dn_err:.3f}, mean history {n_h:.1f}")
    assert tp_err <= QUALITY_RATIO * dn_err, (tp_err, dn_err)
    assert abs(m_tp - m_raw) <= BRIGHTNESS_SHIFT * m_raw, (m_tp, m_raw)
