"""Test infrastructure for fw_render_aovs / fw_denoise (the product never imports it).

- denoise(): a numpy restatement of fw_denoise's filter (include/firework_hip.h), in float64 from the float32 inputs, vectorised over
  shifted copies of the image.
- aovs_from_hits(): fw_render_aovs' composition from per-sample hits, in float32 and sample order: albedo through the oracle's
  texture_sample / env_sample and the SceneDesc's material table.
- aovs_composed(): the same from the library's own ray queries (fw_camera_rays for each sample, fw_trace_rays with key_base 0).
"""
import re
import os

import numpy as np

from firework_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# the filter's constants, as the header states them (tests/test_denoise_cpu.py checks the three places agree)
EPS = 0.01
NORMAL_POW = 128
PLANE = 0.01
LUM = 128.0
ITERATIONS = 5
KAPPA = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def header_constants():
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    return {name: float(re.search(r"#define FW_DENOISE_%s\s+([0-9.]+)f?" % name, text).group(1))
            for name in ("EPS", "NORMAL_POW", "PLANE", "LUM", "ITERATIONS", "MAX_ITERATIONS")}


def _shift(img, dy, dx):
    """img[y + dy, x + dx] for every (y, x), and the mask of the taps inside the image (0 where outside)."""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    ok = np.zeros((h, w), bool)
    if abs(dy) >= h or abs(dx) >= w:
        return out, ok
    ys, yd = slice(max(0, dy), min(h, h + dy)), slice(max(0, -dy), min(h, h - dy))
    xs, xd = slice(max(0, dx), min(w, w + dx)), slice(max(0, -dx), min(w, w - dx))
    out[yd, xd] = img[ys, xs]
    ok[yd, xd] = True
    return out, ok


def _finite_rows(a):
    return np.all(np.isfinite(a), axis=-1)


def filtered_linear(color, aov, moments, width, height, iterations=ITERATIONS):
    """The filter's output colour out_p (float64, (N, 3)) before the resolve: e^(L) (a + eps), or the input colour where a pixel passes."""
    H, W = int(height), int(width)
    c = np.asarray(color, F32).reshape(H, W, 3).astype(np.float64)
    a4 = np.asarray(aov, F32).reshape(H, W, 12).astype(np.float64)
    alb, cov, nrm, dist, pos = a4[..., 0:3], a4[..., 3], a4[..., 4:7], a4[..., 7], a4[..., 8:11]
    ae = alb + EPS
    e = c / ae
    with np.errstate(all="ignore"):
        if moments is not None:
            m = np.asarray(moments, F32).reshape(H, W, 4).astype(np.float64)
            nf = m[..., 3:4]
            var = np.where(nf >= 2, (m[..., 0:3] - nf * c * c) / (nf - 1), 0.0)
            var = np.where(var > 0, var, 0.0)
            q = var / (ae * ae)
            v = ((q[..., 0] + q[..., 1]) + q[..., 2]) / 3 / nf[..., 0]
        else:
            v = np.zeros((H, W))
        for i in range(int(iterations)):
            h = 1 << i
            ev = np.concatenate([e, v[..., None]], axis=-1)
            ok_ev = _finite_rows(ev)
            l_p = (e[..., 0] + e[..., 1] + e[..., 2]) / 3
            if moments is not None:
                gs, gw = np.zeros((H, W)), np.zeros((H, W))
                k3 = (0.25, 0.5, 0.25)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        vq, ok = _shift(v, dy, dx)
                        ok = ok & np.isfinite(vq)
                        wt = k3[dx + 1] * k3[dy + 1] * ok
                        gs += wt * np.where(ok, vq, 0.0)
                        gw += wt
                g = np.where(gw > 0, gs / np.where(gw > 0, gw, 1.0), 0.0)
                lum_den = LUM * np.sqrt(g) + 1e-6
            plane_den = PLANE * dist + 1e-6
            sw = np.full((H, W), KAPPA[2] ** 2)
            se = sw[..., None] * e
            sv = sw * sw * v
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        continue
                    evq, ok = _shift(ev, h * dy, h * dx)
                    okq, _ = _shift(ok_ev, h * dy, h * dx)
                    ok = ok & okq
                    nq, _ = _shift(nrm, h * dy, h * dx)
                    xq, _ = _shift(pos, h * dy, h * dx)
                    wn = np.sum(nrm * nq, axis=-1)
                    wn = np.where(wn > 0, wn, 0.0) ** NORMAL_POW
                    pd = np.abs(np.sum(nrm * (xq - pos), axis=-1))
                    w = KAPPA[dx + 2] * KAPPA[dy + 2] * wn * np.exp(-(pd / plane_den))
                    if moments is not None:
                        l_q = (evq[..., 0] + evq[..., 1] + evq[..., 2]) / 3
                        w = w * np.exp(-(np.abs(l_p - l_q) / lum_den))
                    w = np.where(ok, w, 0.0)
                    evq = np.where(ok[..., None], evq, 0.0)
                    se += w[..., None] * evq[..., 0:3]
                    sv += w * w * evq[..., 3]
                    sw += w
            e = se / sw[..., None]
            v = sv / (sw * sw)
        out = e * ae
    passthrough = (int(iterations) == 0) | (cov == 0) | ~_finite_rows(c)
    out = np.where(passthrough[..., None], c, out)
    return out.reshape(-1, 3)


def resolve(linear, gamma=2.2):
    """resolve_pixel at one sample in float32: (linear, gamma floats clamped to [0, 1], rgb8)."""
    lin = np.asarray(linear, F32)
    with np.errstate(all="ignore"):
        g = np.power(lin, F32(1.0) / F32(gamma)).astype(F32)
    g = np.where(np.isnan(g), g, np.clip(g, 0, 1)).astype(F32)
    q = g * F32(255.99)
    rgb8 = np.where(q > 0, np.minimum(np.where(np.isnan(q), 0, q), 255), 0).astype(np.uint8)
    return lin, g, rgb8


def denoise(color, aov, moments, width, height, iterations=ITERATIONS, gamma=2.2):
    """(linear, gamma, rgb8) of the restated filter; linear in float32 from the float64 result."""
    return resolve(filtered_linear(color, aov, moments, width, height, iterations).astype(F32), gamma)


# ---- fw_render_aovs' composition -----------------------------------------------------------------------------------------------
def _clamp01(x):
    return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)


def _len32(v):
    v = np.asarray(v, F32)
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F32)


class _DescScene:
    """what oracle.env_sample takes (an object with to_desc), for a SceneDesc already built"""

    def __init__(self, sd):
        self.sd = sd

    def to_desc(self):
        return self.sd


def sample_values(sd, rays, hit, oracle):
    """One sample's per-pixel values from hits: (albedo (N, 3), hit mask, normal (N, 3), distance (N,), position (N, 3)), float32."""
    n = rays.shape[0]
    rays = np.asarray(rays, F32)
    is_hit = hit["object"] != A.FW_NO_HIT
    alb = np.zeros((n, 3), F32)
    mats, texs = sd.desc.materials, sd.desc.textures
    const_cache = {}
    for i in np.nonzero(is_hit)[0]:
        m = mats[int(hit["material"][i])]
        if m.kind == A.FW_MAT_METAL:
            alb[i] = (m.albedo.x, m.albedo.y, m.albedo.z)
        elif m.kind == A.FW_MAT_DIELECTRIC:
            alb[i] = 1.0
        else:
            t = texs[m.texture]
            if t.kind == A.FW_TEX_CONSTANT:
                if m.texture not in const_cache:
                    const_cache[m.texture] = oracle.texture_sample(sd, m.texture, 0.0, 0.0, np.zeros(3, F32))
                c = const_cache[m.texture]
            else:
                c = oracle.texture_sample(sd, m.texture, float(hit["u"][i]), float(hit["v"][i]), hit["point"][i])
            alb[i] = _clamp01(c) if m.kind == A.FW_MAT_EMISSIVE else c
    miss = ~is_hit
    if miss.any():
        env = sd.desc.environment
        d = rays[miss, 3:6]
        dirs = (d / _len32(d)[:, None]).astype(F32)
        if env.kind == A.FW_ENV_COLOR:
            vals = np.tile(np.array([env.color.x, env.color.y, env.color.z], F32), (len(dirs), 1))
        else:
            scene = _DescScene(sd)
            vals = np.array([oracle.env_sample(scene, dd) for dd in dirs], F32).reshape(-1, 3)
        alb[miss] = _clamp01(vals)
    nl = _len32(hit["normal"])
    with np.errstate(all="ignore"):
        nrm = np.where((nl == 0)[:, None], F32(0), hit["normal"] / nl[:, None]).astype(F32)
    dist = (hit["t"].astype(F32) * _len32(rays[:, 3:6])).astype(F32)
    nrm[miss] = 0
    return alb, is_hit, nrm, dist, hit["point"].astype(F32)


def aovs_from_hits(sd, samples, oracle):
    """fw_render_aovs' records (N, 12) float32 from `samples` = [(rays, hits) per sample, in sample order]."""
    n = samples[0][0].shape[0]
    s_a, s_n, s_x = np.zeros((n, 4), F32), np.zeros((n, 4), F32), np.zeros((n, 3), F32)
    for rays, hit in samples:
        alb, is_hit, nrm, dist, pt = sample_values(sd, rays, hit, oracle)
        s_a[:, 0:3] = s_a[:, 0:3] + alb
        s_a[:, 3] = np.where(is_hit, s_a[:, 3] + F32(1), s_a[:, 3])
        s_n[:, 0:3] = np.where(is_hit[:, None], s_n[:, 0:3] + nrm, s_n[:, 0:3])
        s_n[:, 3] = np.where(is_hit, s_n[:, 3] + dist, s_n[:, 3])
        s_x = np.where(is_hit[:, None], s_x + pt, s_x).astype(F32)
    S = F32(len(samples))
    hits = s_a[:, 3]
    out = np.zeros((n, 12), F32)
    out[:, 0:3] = s_a[:, 0:3] / S
    out[:, 3] = hits / S
    out[:, 4:7] = s_n[:, 0:3] / S
    with np.errstate(all="ignore"):
        out[:, 7] = np.where(hits > 0, s_n[:, 3] / hits, F32(0))
        out[:, 8:11] = np.where((hits > 0)[:, None], s_x / hits[:, None], F32(0))
    return out


def aovs_composed(ds, sd, renderer, samples, oracle):
    """The composition over the library's own ray queries: rays from fw_camera_rays(sample s), hits from fw_trace_rays (key_base 0)."""
    s = renderer.settings
    per = []
    for k in range(int(samples)):
        rays = ds.camera_rays(renderer, k)
        per.append((rays, ds.trace(rays, s["use_bvh"], seed=s["seed"])))
    return aovs_from_hits(sd, per, oracle)
