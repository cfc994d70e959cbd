"""The bounds shared by the probe-visibility tests (tests/test_probe_depth_cpu.py, tests/test_gpu_probe_depth.py); the statements
themselves are api.probe_depth_reduce, api.probe_depth_moments and api.probe_lookup_vis (include/firework_hip.h).

Nothing here is measured on the GPU: every quantity comes from the test's own inputs and the numpy statement.  u = 2^-53 throughout.
As in tests/probe_lookup_ref.py the device and numpy evaluate the same float64 expression operation for operation; + - * / floor min
max abs are correctly rounded on both sides, so the two can first part at a square root, where S = 4 float64 ulps are allowed for, and
from there every later operation adds one more rounding's worth of difference.  The bounds are first-order in u.

reduce_bound(acc, G, prior, D, k) — fw_probe_depth_reduce.  Per texel and accumulator (A, B, W; all terms are non-negative: t >= 0)
    |gpu - (prior + acc)| <= e + 2^-24 (|prior| + |acc| + e),    e = 2^-24 |acc| + u (2^k (S + 4) G + (k + 2 S + 8 + D) |acc|)
  the float64 terms, proportional to D and k
    T = (x, y, z) / l:  l carries S, a component S + 1.
    c = (Tx dx + Ty dy) + Tz dz:  three products and two additions on top: off by at most (S + 4) u sum |T_i d_i| <= (S + 4) u |d|
        absolutely (|T| = 1; the dot product can cancel, so nothing relative to c holds).  max(0, .) does not widen it.
    w = c^(2^k) by k squarings:  |dw| <= 2^k |d|^(2^k - 1) dc + k u w  <=  2^k (S + 4) u |d|^(2^k) + k u w.
    dist = min(t * sqrt((dx dx + dy dy) + dz dz), r_max): S + 3 relative; min does not widen it; a miss is exactly r_max.
    the terms  w dist: dist dw + (S + 4) u w dist;  (w dist) dist: dist^2 dw + (2 S + 8) u w dist^2.
    the sequential sum of D non-negative terms: each addition rounds by at most u of a partial sum, which the total bounds: D u acc.
    Summed over j with G = sum_j |d_j|^(2^k) dist_j^m (m = 1, 2, 0 for A, B, W; api.probe_depth_reduce(..., terms=True)):
        u (2^k (S + 4) G + (k + 2 S + 8 + D) acc), the largest of the three counts taken for all.
  half an ulp of float32 per accumulator, for the one rounding: 2^-24 |acc| (of the device's own float64 value, which is within the
    terms above of acc: first order).
  the float32 addition to the running sum: 2^-24 of its exact result, at most |prior| + |acc| + e.
  If the device's float64 sqrt is correctly rounded — IEEE 754 asks it, numpy's is — the float64 accumulators are bit-equal and only the
  two float32 roundings remain, which the test then sees as an error of 0: the reference rounds the same way.

moments: one IEEE division and one rounding per value on both sides from the same float32 sums: bit-equal, no bound.

vis_bound(ref, T, X, grid, pd, positions, normal_bias) — fw_probe_irradiance_vis.  Per channel
    |gpu - ref| <= 2^-24 |ref| + (34 u + eps_w) T
  34 is probe_lookup_ref.rounding_count(False): the normal, the basis, the sums and the product with the float32 rounding; T as there.
  eps_w is the relative error of a normalised weight  w_d = N_d / sum N,  N_d = ((wx wy) wz) g_d: the trilinear part is bit-equal, so
  rel(N_d) = rel(g_d) + u and, the numerators being positive,  eps_w <= 2 max_d rel(N_d) + 8 u  (a weighted mean of the numerators'
  errors, up to 7 additions, the division).  rel(g_d), per corner, from the statement's chain:
    kappa  the relative perturbation of r' = q - P:  q = p + bias nh carries bias (S + 2) u from nh and u |q| from its own two roundings,
           the subtraction one more u |r'|; P is bit-equal (lo, the index and the host's step are).  With |q|, |P| <= Q:
           kappa = u (2 Q + bias (S + 2)) / dist + u.
    dist   sqrt of three squares: relative kappa + (S + 3) u;  d_dist = dist (kappa + (S + 3) u).
    r'/dist a component (at most 1 in magnitude) is off by d_comp = 2 kappa + (S + 4) u.
    ox     = x / s1 with s1 = |x| + |y| + |z| >= 1:  |d ox| <= d_comp + |x| d s1 <= 4 d_comp + 3 u; the fold keeps that (1 - |oy| times a
           sign).  The sign only differs between the two sides where a component of r' is within kappa of zero: the tests' random
           points are not, and the bound relies on it.
    su     = ((ox + 1) 0.5) R - 0.5:  d_su = (R / 2) (4 d_comp + 3 u) + 3 R u;  clamping, floor and fu = su - i keep it (the bilinear
           form is continuous across texel borders, so a floor that differs moves nothing at first order).
    mu     bilinear in (fu, fv) with slopes at most 2 M1 (a difference of two texels, each at most M1 = the map's largest |mu|):
           d_mu = 2 M1 (2 d_su) + 6 u M1;  d_mu2 likewise with M2.
    var    = |mu mu - mu2|:  d_var = 2 |mu| d_mu + d_mu2 + u (2 mu mu + mu2 + var).  The difference can cancel: the bound carries
           d_var / var as it is, and is large where the moments leave no variance.
    t      = dist - mu:  d_t = d_dist + d_mu + u |t|.
    c      = var / (var + t t):  d c / c <= (t t / (var + t t)) d_var / var + (2 |t| / (var + t t)) d_t + 3 u, evaluated at |t| + d_t so that
           the switch at dist <= mu (where v = 1 meets c = 1 with zero slope) is covered.
    v      = (c c) c:  rel_v = 3 rel_c + 2 u  (0 where dist + d_dist <= mu - d_mu on both sides: v = 1 exactly).
    fac    the wrap factor: probe_lookup_ref's ceil(2.24 (2 S + 6)) + 2 = 34 u, or 0 without wrap.
    g      = fac v: rel_fac + rel_v + u;  max(1e-6, .) does not widen a relative error;  the crush (g (g g)) 25 triples it and adds 3 u
           (it is continuous at 0.2, so a switch that differs moves nothing at first order):  rel_g = 3 (rel_fac + rel_v + u) + 3 u."""
import math

import numpy as np

import probe_lookup_ref as L

S = L.S
U = 2.0 ** -53


def reduce_bound(acc, G, prior, D: int, k: int) -> np.ndarray:
    """the bound above for the float64 accumulators acc (N, R, R, 3) of api.probe_depth_reduce, their G (N, 3) and the float32 sums
    before the call, prior (N, R, R, 3)"""
    acc = np.abs(np.asarray(acc, np.float64))
    e = 2.0 ** -24 * acc + U * (2.0 ** k * (S + 4) * np.asarray(G, np.float64)[:, None, None, :] + (k + 2 * S + 8 + D) * acc)
    return e + 2.0 ** -24 * (np.abs(np.asarray(prior, np.float64)) + acc + e)


REL_FAC = math.ceil(2.24 * (2 * S + 6)) + 2


def weight_error(X, grid, R: int, positions, normal_bias: float) -> np.ndarray:
    """eps_w (N,) of the derivation above from api.probe_lookup_vis(..., terms=True)'s X"""
    p = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    Q = np.maximum(np.abs(p).max(axis=1) + float(normal_bias), max(abs(v) for v in tuple(grid.lo) + tuple(grid.hi)))[:, None]
    dist, mu, mu2 = X["dist"], X["mu"], X["mu2"]
    with np.errstate(all="ignore"):
        kappa = U * (2.0 * Q + float(normal_bias) * (S + 2)) / dist + U
        d_dist = dist * (kappa + (S + 3) * U)
        d_comp = 2.0 * kappa + (S + 4) * U
        d_su = (R / 2.0) * (4.0 * d_comp + 3.0 * U) + 3.0 * R * U
        d_mu = 2.0 * X["m1"] * (2.0 * d_su) + 6.0 * U * X["m1"]
        d_mu2 = 2.0 * X["m2"] * (2.0 * d_su) + 6.0 * U * X["m2"]
        var = np.abs(mu * mu - mu2)
        d_var = 2.0 * np.abs(mu) * d_mu + d_mu2 + U * (2.0 * mu * mu + np.abs(mu2) + var)
        d_t = d_dist + d_mu + U * np.abs(dist - mu)
        t = np.abs(dist - mu) + d_t
        rel_c = (t * t / (var + t * t)) * (d_var / var) + (2.0 * t / (var + t * t)) * d_t + 3.0 * U
        rel_v = np.where((dist == 0.0) | (dist + d_dist <= mu - d_mu), 0.0, 3.0 * rel_c + 2.0 * U)
    rel_fac = REL_FAC * U if grid.wrap else 0.0
    rel_g = 3.0 * (rel_fac + rel_v + U) + 3.0 * U
    return 2.0 * (rel_g.max(axis=1) + U) + 8.0 * U


def vis_bound(ref, T, X, grid, R: int, positions, normal_bias: float) -> np.ndarray:
    """the bound above for api.probe_lookup_vis(..., terms=True)'s (ref, T, X)"""
    eps = weight_error(X, grid, R, positions, normal_bias)[:, None]
    return 2.0 ** -24 * np.abs(np.asarray(ref, np.float64)) + (L.rounding_count(False) * U + eps) * np.asarray(T, np.float64)
