"""Float64 restatement of environment sampling's table (FW_FLAG_ENV_SAMPLING) and the quadrature the GPU tests compare with.

A map is (h, w, 3), row 0 at the top.  env_texel restates env_sample's lookup (the reference's sphere_uv, `(y as f32 * width) as usize + x`,
the clamp at the poles) in float32 as the device computes it; the table weights texel (x, y) by max(r, g, b) x Omega_row(y), negative and
non-finite channels counted as 0."""
import numpy as np


def row_bounds(h):
    """sin(theta) at the top and bottom edge of each row: row y covers dir.y in [cos((y+1) pi / h), cos(y pi / h)]"""
    y = np.arange(h, dtype=np.float64)
    return np.cos(y * np.pi / h), np.cos((y + 1) * np.pi / h)


def omega_row(w, h):
    """solid angle of one texel of each row"""
    hi, lo = row_bounds(h)
    return 2 * np.pi / w * (hi - lo)


def texel_weights(rgb):
    m = np.asarray(rgb, np.float64)
    m = np.where(np.isfinite(m) & (m > 0), m, 0.0)
    h, w = m.shape[:2]
    return m.max(-1) * omega_row(w, h)[:, None]


def table(rgb):
    """-> (per-texel probabilities (h, w), per-texel density p / Omega (h, w), total weight)"""
    wt = texel_weights(rgb)
    tot = wt.sum()
    p = wt / tot if tot > 0 else np.zeros_like(wt)
    h, w = p.shape
    return p, p / omega_row(w, h)[:, None], tot


def env_texel(dirs, w, h):
    """env_sample's texel index of unit directions (n, 3), float32 as on the device (sphere_uv, then the reference's index and clamp)"""
    d = np.asarray(dirs, np.float32)
    f = np.float32
    with np.errstate(invalid="ignore"):
        phi = np.arctan2(d[:, 2], d[:, 0]).astype(f)
        theta = np.arcsin(np.clip(d[:, 1], -1, 1)).astype(f)
        u = (f(1) - (phi + f(np.pi)) / f(2 * np.pi)).astype(f)
        v = ((theta + f(np.pi / 2)) / f(np.pi)).astype(f)
        x = np.floor(np.maximum(u * f(w), 0)).astype(np.int64)
        y = np.floor(np.maximum((f(1) - v) * f(h), 0)).astype(np.int64)
        idx = np.floor((y.astype(f) * f(w)).astype(np.float64)).astype(np.int64) + x
    return np.minimum(idx, w * h - 1)


def texel_cos3(w, h):
    """int over each texel of 2 cos^3(theta') / pi dw for a floor with normal +y (theta' from the normal: cos = max(dir.y, 0)): per row
    (2 pi / w) int 2 s^3 / pi ds = (max(s_hi, 0)^4 - max(s_lo, 0)^4) / w.  -> (h,) per texel of each row"""
    hi, lo = row_bounds(h)
    return (np.maximum(hi, 0) ** 4 - np.maximum(lo, 0) ** 4) / w


def floor_answer(rgb, albedo):
    """albedo x sum_t L_t int_t 2 cos^3 / pi dw per channel, and the default estimator's per-sample variance per channel"""
    m = np.asarray(rgb, np.float64)
    h, w = m.shape[:2]
    c = texel_cos3(w, h)[:, None, None]
    mean = albedo * (m * c).sum((0, 1))
    second = albedo ** 2 * (m ** 2 * c).sum((0, 1))
    return mean, second - mean ** 2
