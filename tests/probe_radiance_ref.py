"""The bounds shared by the probe-radiance tests (tests/test_probe_radiance_cpu.py, tests/test_gpu_probe_radiance.py); the statements
themselves are api.probe_radiance_reduce, api.probe_radiance_prefilter, api.probe_radiance_lookup and api.probe_glossy_ref
(include/firework_hip.h).

Nothing here is measured on the GPU: every quantity comes from the test's own inputs and the numpy statement.  u = 2^-53 throughout.
As in tests/probe_depth_ref.py the device and numpy evaluate the same float64 expression operation for operation; + - * / floor min max
abs and comparisons are correctly rounded (or exact) on both sides, so the two can first part at a square root, where S = 4 float64 ulps
are allowed for, and from there every later operation adds one more rounding's worth of difference.  The bounds are first-order in u.

reduce_bound(acc, G, B, prior, D, k) — fw_probe_radiance_reduce.  Per texel and accumulator (A_r, A_g, A_b, W)
    |gpu - (prior + acc)| <= e + 2^-24 (|prior| + |acc| + e),    e = 2^-24 |acc| + u (2^k (S + 4) G + (k + 2 + D) B)
  T = (x, y, z) / l and c = (Tx dx + Ty dy) + Tz dz are probe_depth_ref's: c is off by at most (S + 4) u |d| absolutely, and
    w = c^(2^k) by |dw| <= 2^k (S + 4) u |d|^(2^k) + k u w.  A ray whose c is within that of 0 can be skipped on one side and counted on
    the other: what it then adds or leaves out is a w within dw of 0, which the same term covers.
  L_c = (double)accum.c / samples is one correctly rounded division of bit-equal operands: bit-equal.
  the term w L_c: |L_c| dw + u w |L_c|; the sequential sum of D terms, each addition rounding by at most u of a partial sum of
    magnitudes, which B = sum_j w_j |L_cj| bounds: D u B.  Summed over j with G = sum_j |d_j|^(2^k) |L_cj| (1 in L's place for W):
        u (2^k (S + 4) G + (k + 1 + D) B), and one more u B for the product where W has none: (k + 2 + D) taken for all four.
  half an ulp of float32 for the accumulator's one rounding and the float32 addition to the running sum: as probe_depth_ref.

prefilter_bound(pr, level, q, Wt, B, on) — fw_probe_radiance_prefilter, a texel of a level >= 1, per channel
    |gpu - float32(q)| <= 2^-24 |q| + dq (1 + 2^-24),    dq = (dA + |q| dWt) / Wt + u |q|
  Level 0 is one division and one rounding of bit-equal float32 sums on both sides: bit-equal, no bound; the flags are exact.
  T and S are unit vectors with S + 1 ulps per component; c = (Tx Sx + Ty Sy) + Tz Sz: each product carries 2 (S + 1) + 1, the two
    additions one each of a partial sum at most sum |T_i S_i| <= 1:  e_c = (2 S + 5) u, absolute.  A source whose c is within e_c of 0
    can be skipped on one side only; its weight is then within dw of 0 (w is proportional to c): covered.
  h = (1 + c) 0.5: e_c / 2 + u absolutely (h <= 1).  a2 = (rho rho)(rho rho): 3 u relative.  den = h (a2 - 1) + 1 lies in [a2, 1] and
    is off by at most (1 - a2) (e_c / 2 + u) + 3 u a2 + 3 u absolutely:  r_den = ((1 - a2) (e_c / 2 + u) + 6 u) / den  relative.
  omega = (4 / (R R)) / ((len len) len): len carries S + 2 roundings under and at the root, cubed: 3 (S + 2) + 4 = r_om u relative.
  w = ((a2 / (den den)) c) omega:  dw <= w (2 r_den + 3 u + 4 u + r_om u) + (a2 / (den den)) omega e_c,  the last term for c's absolute
    error.  dWt = sum_s dw + n_src u Wt and dA = sum_s dw |L_s| + (n_src + 1) u B over the flagged sources with c > 0 (L_s is a stored
    float32: bit-equal), B = sum w |L|.  The quotient adds u |q|; its float32 rounding differs from the statement's by at most one
    float32 ulp where the two float64 values straddle a rounding boundary: 2^-24 (|q| + dq) on top of dq.

lookup_bound(ref, T, X, grid, pr, maps, positions, normal_bias, placement, depth_R) — fw_probe_radiance_lookup, per channel
    |gpu - ref| <= 2^-24 |ref| + (eps_w + 16 u) T + d_fetch
  eps_w: probe_place_ref.placed_bound's factor of T — the corner weights are the placed lookup's, operation for operation.
  r = dirs / sqrt((x x + y y) + z z): a component carries (S + 4) u = d_comp.  ox = x / s1 with s1 = |x| + |y| + |z| >= 1:
    |d ox| <= 4 d_comp + 3 u, and the fold keeps that; su = ((ox + 1) 0.5) R_l - 0.5:  d_su = (R_l / 2) (4 d_comp + 3 u) + 3 R_l u.  The
    sign of a folded coordinate only differs between the two sides where a component of r is within d_comp of zero: the tests' random
    directions are not, and the bound relies on it.
  a fetch is bilinear in (fu, fv) with slopes at most 2 Mx (Mx the largest |rgb| in the corner probe's pyramid), continuous across
    texel borders: d_m = 2 Mx (2 d_su) + 8 u Mx with R_l <= R taken for every level.  The level and t are comparisons and one
    subtraction and division of bit-equal float32 values widened: bit-equal.  m = m_l (1 - t) + m_(l+1) t: convex, so d_m holds for m,
    with 4 u more of its magnitude; the product with the weight and the sum over 8 corners: 9 u: 16 u in all on T, generous.
  d_fetch = sum_d |w_d| d_m(d).

glossy.  Where rho is not > 0 the kernel evaluates fw_probe_shade_placed's arithmetic in its order: bit-equal to that call.  Elsewhere
    the float32 arithmetic after the lookup is stated operation for operation (api.probe_glossy_ref) and fed the device lookup's own
    output at the statement's r; r and S part from the statement only through the two square roots (at most one float32 ulp where a
    float64 value straddles a rounding boundary), which the tests' inputs avoid being sensitive to: they compare bit for bit and report
    the count of differing pixels if any."""
import numpy as np

import probe_lookup_ref as L
import probe_place_ref as PP

S = L.S
U = 2.0 ** -53


def reduce_bound(acc, G, B, prior, D: int, k: int) -> np.ndarray:
    """the bound above for api.probe_radiance_reduce(..., terms=True)'s (acc, G, B) and the float32 sums before the call, prior"""
    acc = np.abs(np.asarray(acc, np.float64))
    e = 2.0 ** -24 * acc + U * (2.0 ** k * (S + 4) * np.asarray(G, np.float64)[:, None, None, :] + (k + 2 + D) * np.asarray(B, np.float64))
    return e + 2.0 ** -24 * (np.abs(np.asarray(prior, np.float64)) + acc + e)


def prefilter_bound(api, pr, level: int, x: dict, level0) -> np.ndarray:
    """the bound above for one level >= 1: x = api.probe_radiance_prefilter(..., terms=True)[1][level - 1], level0 (N, R^2, 4) float32 the
    statement's level 0.  Returns (N, R_l^2, 3)."""
    w, c, den = api.probe_radiance_weights(pr, level)
    _S, omega = api.probe_radiance_sources(pr.resolution)
    rho = float(np.float32(pr.roughness[level]))
    a2 = (rho * rho) * (rho * rho)
    n_src = w.shape[1]
    e_c = (2 * S + 5) * U
    r_den = ((1.0 - a2) * (e_c / 2.0 + U) + 6.0 * U) / den
    r_om = (3 * (S + 2) + 4) * U
    dw = np.where(c > 0.0, w * (2.0 * r_den + 7.0 * U + r_om), 0.0) + np.where(c > -e_c, (a2 / (den * den)) * omega[None, :] * e_c, 0.0)   # (m, n_src)
    L0 = np.abs(np.asarray(level0, np.float32).astype(np.float64))[..., 0:3]                       # (N, n_src, 3)
    on = np.asarray(x["on"], bool).astype(np.float64)                                              # (N, n_src)
    dWt = np.einsum("ms,ns->nm", dw, on) + n_src * U * x["Wt"]
    dA = np.einsum("ms,nsc->nmc", dw, L0 * on[..., None]) + (n_src + 1) * U * x["B"]
    q = np.abs(x["q"])
    with np.errstate(all="ignore"):
        dq = np.where(x["Wt"][..., None] > 0.0, (dA + q * dWt[..., None]) / x["Wt"][..., None] + U * q, 0.0)
    return 2.0 ** -24 * q + dq * (1.0 + 2.0 ** -24)


def lookup_bound(ref, T, X, grid, pr, maps, positions, normal_bias: float, placement, depth_R) -> np.ndarray:
    """the bound above for api.probe_radiance_lookup(..., terms=True)'s (ref, T, X); depth_R None: no depth maps; placement None: neutral"""
    ref, T = np.asarray(ref, np.float64), np.asarray(T, np.float64)
    n = ref.shape[0]
    if placement is None:
        placement = np.tile(np.array([0.0, 0.0, 0.0, 1.0], np.float32), (grid.n_probes, 1))
    eps_w = PP.placed_bound(np.zeros((n, 3)), np.ones((n, 3)), X, grid, depth_R, positions, normal_bias, placement)
    mp = np.asarray(maps, np.float32).astype(np.float64).reshape(grid.n_probes, -1, 4)[..., 0:3]
    with np.errstate(all="ignore"):
        mx = np.nanmax(np.where(np.isfinite(mp), np.abs(mp), 0.0), axis=(1, 2))                    # (n_probes,)
    R = float(pr.resolution)
    d_comp = (S + 4) * U
    d_su = (R / 2.0) * (4.0 * d_comp + 3.0 * U) + 3.0 * R * U
    d_m = 2.0 * mx[X["probe"]] * (2.0 * d_su) + 8.0 * U * mx[X["probe"]]                          # (N, corners)
    d_fetch = (np.abs(X["w"]) * d_m).sum(axis=1)[:, None]
    return 2.0 ** -24 * np.abs(ref) + (eps_w + 16.0 * U) * T + d_fetch
