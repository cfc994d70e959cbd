"""Bounds shared by the probe tests (tests/test_probes_cpu.py, tests/test_gpu_probes.py); the statements themselves are api.ProbeSet.rays,
api.sh_basis and api.sh_project.

lattice_bound(f): the quadrature error of the shifted spherical Fibonacci lattice, derived, not measured.
The lattice of D points is c_j = 1 - 2 (j + xi_u) / D, phi_j = 2 pi frac(j g + xi_v) with g = (sqrt 5 - 1) / 2, and the estimate of
I = int f d omega is Q = (4 pi / D) sum_j f(c_j, phi_j).  Write f(c, phi) = sum_m a_m(c) exp(i m phi); the integrands here are
polynomials of degree <= 4 in (x, y, z), so |m| <= 4 and a_(-m) = conj(a_m).
  m = 0: I = 2 pi int a_0 dc, and (4 pi / D) sum_j a_0(c_j) is a rectangle rule with one node somewhere in each cell of width 2 / D, so
         its error is at most 2 pi (2 / D) TV(a_0): the sum over the cells of width x variation inside the cell.
  m != 0: the exact integral is 0, and the sum is sum_j a_m(c_j) w_j with w_j = z^j exp(2 pi i m xi_v), z = exp(2 pi i m g).  Summation by
         parts with W_J = w_0 + ... + w_J, |W_J| = |1 - z^(J+1)| / |1 - z| <= 1 / |sin(pi m g)|, gives
         |sum_j a_m(c_j) w_j| <= (|a_m(c_(D-1))| + sum_j |a_m(c_(j+1)) - a_m(c_j)|) / |sin(pi m g)| <= (max |a_m| + TV(a_m)) / |sin(pi m g)|
         because the c_j are monotone.
Together |Q - I| <= C / D for every D and every shift, with
    C = 4 pi (TV(a_0) + 2 sum_(m = 1..4) (max |a_m| + TV(a_m)) / |sin(pi m g)|).
a_m comes from an exact 16-point DFT in phi (|m| <= 4 < 8) on 4001 values of c; a sum of |differences| on a grid never exceeds the
true variation and misses it by O(h^2) at each of the few extrema, so the result is multiplied by 1.001.
The rays are float32: each direction is off its float64 value by at most 2^-24 per component, which moves f by at most
Lip(f) sqrt(3) 2^-24; float32_term(f) = 4 pi Lip(f) sqrt(3) 2^-24 is added where a test evaluates f on stored rays (Lip from the same
grid's finite differences, times 1.01).

project_bound(...): fw_probe_project against api.sh_project — see its docstring."""
import numpy as np

G = (np.sqrt(5.0) - 1.0) / 2.0
_NC, _NPHI = 4001, 16


def _grid():
    c = np.linspace(-1.0, 1.0, _NC)[:, None]
    phi = (2.0 * np.pi / _NPHI) * np.arange(_NPHI)[None, :]
    rad = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    return np.stack([rad * np.cos(phi), np.broadcast_to(c, (_NC, _NPHI)), rad * np.sin(phi)], axis=-1)


def lattice_bound(f) -> float:
    """C with |(4 pi / D) sum_j f(d_j) - int f| <= C / D for a polynomial f of degree <= 4 (f maps (..., 3) directions to (...) values)"""
    a = np.fft.fft(f(_grid()), axis=1) / _NPHI                       # a[:, m] = a_m(c), m = 0..15 (negative m wrap round)
    assert np.abs(a[:, 5:12]).max() <= 1e-12 * max(1.0, np.abs(a).max()), "f has azimuthal orders above 4"
    tv = np.abs(np.diff(a, axis=0)).sum(axis=0)
    amax = np.abs(a).max(axis=0)
    total = tv[0]
    for m in range(1, 5):
        total += 2.0 * (amax[m] + tv[m]) / abs(np.sin(np.pi * m * G))
    return float(1.001 * 4.0 * np.pi * total)


def float32_term(f) -> float:
    v = f(_grid())
    d = _grid()                                  # the slope along the chord between neighbours on the grid, in c and in phi
    lip = 0.0
    for axis in (0, 1):
        dv = np.abs(np.diff(v, axis=axis))
        dd = np.linalg.norm(np.diff(d, axis=axis), axis=-1)
        ok = dd > 0
        lip = max(lip, float((dv[ok] / dd[ok]).max()))
    return float(4.0 * np.pi * 1.01 * lip * np.sqrt(3.0) * 2.0 ** -24)


def quadrature_bound(f, D: int) -> float:
    """lattice_bound(f) / D, plus float32_term(f) for the stored float32 directions, plus the float64 arithmetic of the estimate itself:
    D terms of at most max |f|, each with a few roundings, summed in any order: at most (D + 16) 2^-53 4 pi max |f|"""
    fmax = float(np.abs(f(_grid())).max())
    return lattice_bound(f) / D + float32_term(f) + (D + 16) * 2.0 ** -53 * 4.0 * np.pi * fmax


def project_bound(ref, abs_terms, sums_in, directions):
    """|gpu sums - (sums_in + ref)| for fw_probe_project, from its construction.  ref = api.sh_project(...) (float64), abs_terms =
    (4 pi / D) sum_j |Y_k a_j / S|, sums_in the float32 sums before the call.
      float64 inside: each term carries a few roundings (basis, division, product) and passes through at most ceil(D / 64) sequential
        additions and 6 tree levels on the device, D additions in numpy: together at most (D + ceil(D / 64) + 40) 2^-53 abs_terms.
      one float32 rounding of proj: at most 2^-24 |proj| (round to nearest), or 2^-150 where proj is subnormal.
      one float32 addition: at most 2^-24 |sums_in + proj32|, proj32 the rounded projection.
    The float32 terms are written with the reference's values: the device's float64 projection differs from them by the float64 term
    (the factor 1 + 2^-20 on the rounding), and proj32 from the reference by the two terms before it."""
    ref = np.asarray(ref, np.float64)
    s_in = np.asarray(sums_in, np.float64)
    e64 = (directions + (directions + 63) // 64 + 40) * 2.0 ** -53 * np.asarray(abs_terms, np.float64)
    r32 = e64 + 2.0 ** -24 * np.abs(ref) * (1.0 + 2.0 ** -20) + 2.0 ** -149
    return r32 + 2.0 ** -24 * (np.abs(s_in + ref) + r32)


def abs_terms(api, rays, accum, samples, directions):
    """(4 pi / D) sum_j |Y_k(d_pj) accum[p D + j][c] / samples|: (N, 9, 3)"""
    D = int(directions)
    r = np.asarray(rays, np.float64).reshape(-1, D, 6)
    a = np.abs(np.asarray(accum, np.float64).reshape(-1, D, 4)[..., :3]) / float(samples)
    return (4.0 * np.pi / D) * np.einsum("pjk,pjc->pkc", np.abs(api.sh_basis(r[..., 3:])), a)
