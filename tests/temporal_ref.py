"""Test infrastructure for fw_temporal (the product never imports it): a numpy restatement of include/firework_hip.h's statement,
vectorised over the pixels, one pass per bilinear tap: in float64 from the float32 inputs, except the image coordinates of step 2,
which are the statement's own float32 values (project32, in the statement's association; IEEE without contraction, as numpy computes).
A bilinear weight multiplies whatever contrast neighbouring history pixels have — at 16 spp two neighbours' sums of squares differ by
orders of magnitude — so a coordinate that differs in its seventh digit (what float32 and float64 arithmetic on coordinates of
several hundred units give, measured: 1e-5 px at 96 x 80) moves an output by more than 1e-4 of its value.  Everything downstream of
the coordinates — the tests, the demodulated sums, the merge — is float64.

- camera_basis(): make_camera's basis (camera.rs:74-107) from a fw_camera_settings, in float32 steps as the host forms it.
- project(): step 2 in float64, world positions -> (continuous column, continuous row, depth); project32(): the same in float32.
- temporal(): the whole operation; also returns the mask of pixels where one of the restatement's own threshold tests sits within
  NEAR of its threshold — the pixels a float32 kernel may decide differently, which the GPU comparison leaves out.
"""
import math
import os
import re

import numpy as np

from firework_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# the constants, as the header states them (tests/test_temporal_cpu.py checks the three places agree)
EPS = 0.01              # FW_DENOISE_EPS
NORMAL_COS = 0.9
PLANE = 0.02
MIN_TAP = 1e-3
NEAR = 1e-4             # a tested value within NEAR (relative) of its threshold; for a tap weight, NEAR of the unit weight


def header_constants():
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    return {name: float(re.search(r"#define FW_TEMPORAL_%s\s+([0-9.e-]+)f?" % name, text).group(1)) for name in ("NORMAL_COS", "PLANE", "MIN_TAP")}


def _fma32(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def camera_basis(cam, width, height):
    """pos, u, v, w (float64 arrays of the float32 values) and half_width, half_height of a fw_camera_settings (or CameraSettings)."""
    c = cam if isinstance(cam, A.fw_camera_settings) else cam.to_abi()
    pos = np.array([c.cam_pos.x, c.cam_pos.y, c.cam_pos.z], F32)
    at = np.array([c.look_at.x, c.look_at.y, c.look_at.z], F32)

    def dot(a, b):
        return _fma32(a[0], b[0], _fma32(a[1], b[1], F32(a[2] * b[2])))

    def cross(a, b):
        return np.array([_fma32(a[1], b[2], -F32(a[2] * b[1])), _fma32(a[2], b[0], -F32(a[0] * b[2])), _fma32(a[0], b[1], -F32(a[1] * b[0]))], F32)

    def normalized(a):
        return (a / np.sqrt(dot(a, a))).astype(F32)
    w = normalized((pos - at).astype(F32))
    u = normalized(cross(np.array([0, 1, 0], F32), w))
    v = cross(w, u)
    theta = F32(F32(c.vfov) * F32(3.14159265358979323846) / F32(180.0))
    hh = F32(math.tan(float(F32(theta / F32(2.0)))))          # (the correctly rounded float32 tangent)
    hw = F32(F32(hh * F32(width)) / F32(height))
    return dict(pos=pos.astype(np.float64), u=u.astype(np.float64), v=v.astype(np.float64), w=w.astype(np.float64), half_width=float(hw),
                half_height=float(hh))


def project(basis, X, width, height):
    """(x, row, depth) of world positions X (N, 3): the continuous column and row of the previous image; NaN where depth <= 0."""
    e = np.asarray(X, np.float64) - basis["pos"]
    depth = -(e @ basis["w"])
    with np.errstate(all="ignore"):
        ok = depth > 0
        d = np.where(ok, depth, np.nan)
        u = 0.5 + (e @ basis["u"]) / (2 * basis["half_width"] * d)
        v = 0.5 + (e @ basis["v"]) / (2 * basis["half_height"] * d)
    return u * width - 0.5, height - (v * height - 0.5), depth


def project32(basis, X, width, height):
    """project() in float32, operation for operation as the header writes step 2 (sums of three products left to right)."""
    f = np.float32
    X = np.asarray(X, f)
    pos, bu, bv, bw = (np.asarray(basis[k], f) for k in ("pos", "u", "v", "w"))
    hw, hh, Wf, Hf = f(basis["half_width"]), f(basis["half_height"]), f(width), f(height)
    with np.errstate(all="ignore"):
        e = (X - pos[None]).astype(f)
        dot = lambda a: ((e[:, 0] * a[0] + e[:, 1] * a[1]) + e[:, 2] * a[2]).astype(f)
        depth = -dot(bw)
        ok = depth > 0
        d = np.where(ok, depth, f(np.nan))
        u = f(0.5) + dot(bu) / ((f(2) * hw) * d)
        v = f(0.5) + dot(bv) / ((f(2) * hh) * d)
        x = u * Wf - f(0.5)
        row = Hf - (v * Hf - f(0.5))
    assert x.dtype == f and row.dtype == f and depth.dtype == f
    return x, row, depth


def _finite_rows(a):
    return np.all(np.isfinite(a), axis=-1)


def temporal(color, moments, aov, history, prev_position, width, height, prev_camera, samples=0, max_history=np.inf,
             normal_cos=NORMAL_COS, plane=PLANE, min_tap=MIN_TAP):
    """fw_temporal restated.  history = (hist_color, hist_moments, hist_aov) or None.  Returns (out_color (N, 3), out_moments (N, 4),
    out_history (N,), near (N,) bool), float64."""
    W, H = int(width), int(height)
    n = W * H
    c32 = np.asarray(color, F32).reshape(n, 3)
    c = c32.astype(np.float64)
    a = np.asarray(aov, F32).reshape(n, 12).astype(np.float64)
    if moments is not None:
        cur = np.asarray(moments, F32).reshape(n, 4).astype(np.float64)
    else:
        with np.errstate(all="ignore"):
            cur = np.concatenate([float(samples) * (c * c), np.full((n, 1), float(samples))], axis=1)
    out_c, out_m, out_h = c.copy(), cur.copy(), np.zeros(n)
    near = np.zeros(n, bool)
    if history is None:
        return out_c, out_m, out_h, near
    hc = np.asarray(history[0], F32).reshape(n, 3).astype(np.float64)
    hm = np.asarray(history[1], F32).reshape(n, 4).astype(np.float64)
    ha = np.asarray(history[2], F32).reshape(n, 12).astype(np.float64)
    X = a[:, 8:11] if prev_position is None else np.asarray(prev_position, F32).reshape(n, 3).astype(np.float64)
    basis = camera_basis(prev_camera, W, H)
    with np.errstate(all="ignore"):
        nl = np.sqrt(np.sum(a[:, 4:7] ** 2, axis=1))
        live = (a[:, 3] != 0) & _finite_rows(c) & _finite_rows(X) & (nl > 0) & np.isfinite(nl)
        n_p = a[:, 4:7] / np.where(live, nl, 1.0)[:, None]
        Xs = np.where(live[:, None], X, 0.0)
        x32, row32, depth = project32(basis, Xs, W, H)
        e_len = np.sqrt(np.sum((Xs - basis["pos"]) ** 2, axis=1))
        near |= live & (np.abs(depth) <= NEAR * e_len)
        live = live & (depth > 0)
        live = live & (x32 > -1) & (x32 < F32(W)) & (row32 > -1) & (row32 < F32(H))
        x32, row32 = np.where(live, x32, F32(0)), np.where(live, row32, F32(0))
        fx, fy = np.floor(x32), np.floor(row32)
        bx32, by32 = (x32 - fx).astype(np.float32), (row32 - fy).astype(np.float32)
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        one = np.float32(1)
        plane_max = plane * e_len
        ok4, b4, tn4, tm4, tq4 = [], [], [], [], []
        for k in range(4):
            dx, dy = k & 1, k >> 1
            qx, qy = ix + dx, iy + dy
            ok = live & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            b = ((bx32 if dx else one - bx32) * (by32 if dy else one - by32)).astype(np.float64)      # the float32 weight
            near |= ok & (np.abs(b - min_tap) <= NEAR)
            ok = ok & (b >= min_tap)
            q = np.where(ok, qy * W + qx, 0)
            m, g, col = hm[q], ha[q], hc[q]
            ok = ok & _finite_rows(m) & (m[:, 3] > 0)
            ok = ok & _finite_rows(g[:, 0:4]) & (g[:, 3] != 0)
            ok = ok & _finite_rows(col) & _finite_rows(g[:, 8:11])
            ql = np.sqrt(np.sum(g[:, 4:7] ** 2, axis=1))
            ok = ok & (ql > 0) & np.isfinite(ql)
            n_q = g[:, 4:7] / np.where(ok, ql, 1.0)[:, None]
            cosq = np.sum(n_p * n_q, axis=1)
            near |= ok & (np.abs(cosq - normal_cos) <= NEAR * normal_cos)
            ok = ok & (cosq >= normal_cos)
            pd = np.abs(np.sum(n_p * (g[:, 8:11] - Xs), axis=1))
            near |= ok & (np.abs(pd - plane_max) <= NEAR * plane_max)
            ok = ok & (pd <= plane_max)
            aq = g[:, 0:3] + EPS
            ok4.append(ok)
            b4.append(np.where(ok, b, 0.0))
            tn4.append(np.where(ok, m[:, 3], 0.0))
            tm4.append(np.where(ok[:, None], col / aq, 0.0))
            tq4.append(np.where(ok[:, None], m[:, 0:3] / np.where(ok, m[:, 3], 1.0)[:, None] / (aq * aq), 0.0))
        sw = sum(b4)
        has = sw > 0
        sws = np.where(has, sw, 1.0)
        sn = sum((b4[k] / sws) * tn4[k] for k in range(4))
        sm = sum((b4[k] / sws)[:, None] * tm4[k] for k in range(4))
        sq = sum((b4[k] / sws)[:, None] * tq4[k] for k in range(4))
        ap = a[:, 0:3] + EPS
        nh = np.minimum(sn, float(max_history))
        nn = nh + cur[:, 3]
        m_c = (nh[:, None] * (ap * sm) + cur[:, 3:4] * c) / nn[:, None]
        m_q = nh[:, None] * ((ap * ap) * sq) + cur[:, 0:3]
        # (float32 finiteness of the merge, as the kernel tests it)
        fin = _finite_rows(m_c.astype(F32)) & _finite_rows(m_q.astype(F32)) & np.isfinite(nn.astype(F32))
        take = has & fin
    out_c = np.where(take[:, None], m_c, out_c)
    out_m = np.where(take[:, None], np.concatenate([m_q, nn[:, None]], axis=1), out_m)
    out_h = np.where(take, nh, 0.0)
    return out_c, out_m, out_h, near


# ---- synthetic frame pairs (shared by the CPU and GPU tests) ------------------------------------------------------------------------
def _settings(pos, at, vfov=40.0):
    c = A.fw_camera_settings()
    c.cam_pos, c.look_at, c.vfov, c.aperture, c.focus_dist = A.vec3(pos), A.vec3(at), vfov, 0.0, 1.0
    return c


def _synthetic_frame(cam, width, height, rng, count):
    """One frame of a world of two fronto-parallel planes (z = -5, and z = -7 for world x > 0.8: a depth edge) with a band of tilted
    normals (a normal edge) and a position-dependent albedo: jittered pixel rays, float32 records.  -> (color, moments, aov)"""
    W, H = width, height
    n = W * H
    b = camera_basis(cam, W, H)
    idx = np.arange(n)
    px, row = idx % W, idx // W
    jx, jy = rng.uniform(0.3, 0.7, n), rng.uniform(0.3, 0.7, n)
    u, v = (px + jx) / W, (H - row + jy) / H
    d = -b["w"][None] + ((2 * u - 1) * b["half_width"])[:, None] * b["u"][None] + ((2 * v - 1) * b["half_height"])[:, None] * b["v"][None]
    X5 = b["pos"][None] + (-5.0 - b["pos"][2]) / d[:, 2:3] * d
    far = X5[:, 0] > 0.8
    X = np.where(far[:, None], b["pos"][None] + (-7.0 - b["pos"][2]) / d[:, 2:3] * d, X5)
    tilted = (np.abs(X[:, 1]) < 0.3) & (X[:, 0] < -0.5)
    nrm = np.where(tilted[:, None], np.array([0.6, 0.0, 0.8]), np.array([0.0, 0.0, 1.0]))
    alb = 0.5 + 0.3 * np.sin(X[:, 0:1] * np.array([3.0, 4.0, 5.0]) + X[:, 1:2] * np.array([5.0, 3.0, 4.0]))
    irr = 0.8 + 0.15 * np.sin(2.0 * X[:, 0:1] + 1.5 * X[:, 1:2]) + 0.03 * rng.uniform(-1, 1, (n, 3))
    aov = np.zeros((n, 12), F32)
    aov[:, 0:3], aov[:, 3], aov[:, 4:7] = alb, 1.0, nrm
    aov[:, 7] = np.linalg.norm(X - b["pos"][None], axis=1)
    aov[:, 8:11] = X
    color = (alb * irr).astype(F32)
    cnt = np.asarray(count, np.float64) * np.ones(n)
    mom = np.concatenate([cnt[:, None] * (color.astype(np.float64) ** 2 + rng.uniform(0.0, 0.05, (n, 3))), cnt[:, None]], axis=1).astype(F32)
    return color, mom, aov


def synthetic_case(width, height, seed=0, shift=(0.0371, 0.0213, 0.0), inject=True):
    """A current frame and the history of a camera `shift` away, with injected NaN / Inf and zero-coverage pixels.
    -> dict(color, moments, aov, history=(hist_color, hist_moments, hist_aov), camera, prev_camera)"""
    rng = np.random.default_rng(seed)
    n = width * height
    cam = _settings((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    prev = _settings(shift, (shift[0], shift[1], shift[2] - 1.0))
    color, mom, aov = _synthetic_frame(cam, width, height, rng, 16)
    hc, hm, ha = _synthetic_frame(prev, width, height, rng, rng.choice([16.0, 32.0, 48.0], n))
    if inject and n >= 64:
        pick = lambda: rng.choice(n, max(1, n // 150), replace=False)
        color[pick(), 0] = np.nan; color[pick(), 2] = np.inf
        aov[pick(), 3] = 0; aov[pick(), 9] = np.nan; aov[pick(), 4:7] = 0
        hc[pick(), 1] = np.nan; hc[pick(), 0] = -np.inf
        hm[pick(), 2] = np.inf; hm[pick(), 3] = 0
        ha[pick(), 3] = 0; ha[pick(), 1] = np.nan; ha[pick(), 10] = np.inf; ha[pick(), 4:7] = 0
    return dict(color=color, moments=mom, aov=aov, history=(hc, hm, ha), camera=cam, prev_camera=prev)
