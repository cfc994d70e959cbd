"""The bounds and the closed-form scenes shared by the probe-placement tests (tests/test_probe_place_cpu.py,
tests/test_gpu_probe_place.py); the statements themselves are api.probe_survey, api.probe_relocate_step and api.probe_lookup_placed
(include/firework_hip.h).

Nothing here is measured on the GPU: every quantity comes from the test's own inputs and the numpy statement.  u = 2^-53 throughout.
As in tests/probe_lookup_ref.py and tests/probe_depth_ref.py the device and numpy evaluate the same float64 expression operation for
operation; + - * / floor min max abs and comparisons are correctly rounded (or exact) on both sides, so the two can first part at a
square root, where S = 4 float64 ulps are allowed for, and from there every later operation adds one more rounding's worth.

survey.  The counts are integers and the class of a hit is the sign of a sum of three products of float32 values, each exact in
    float64, added in the stated order: equal on both sides.  dist = t * sqrt((dx dx + dy dy) + dz dz): two products, two additions (3 u
    under the root, halved by it: counted whole), the root's S and the product with t: (S + 3) u relative, survey_dist_rel.  The stored
    distance is one float32 rounding of the device's own float64 value, half a float32 ulp of it:
        |gpu - ref| <= ((S + 3) u + 2^-24 (1 + (S + 3) u)) |ref|      against the statement's float64 distance, survey_dist_bound.
    The argmin is exact provided the nearest and the runner-up of a class differ by more than 2 (S + 3) u relative; the tests ask 1e-9
    (argmin_gap) from their own inputs, on the CPU, before the device is asked, and exclude nothing.  Exact ties (equal float64
    distances from equal inputs) are resolved to the lowest j on both sides.  The stored direction is a copy: bit-equal.

step.  `inside` compares an exact integer with one product of two exactly widened float32 values: equal on both sides.  A candidate
    component is o_k +- (d_k / len) * s with s = dist + 0.5 min_front or min_front - dist: the quotient carries S + 2, the product one
    more, the sum one more — (S + 4) u of |o| + dist + min_front — and one float32 rounding, 2^-24 of the same.  Between the two
    sides' roundings lies at most one float32 ulp of the larger:
        |gpu_k - ref_k| <= 2^-23 (|o_k| + dist + min_front)      step_bound, per component, with the distance of the branch taken
    (the back face's for a probe inside, the front face's otherwise); a probe that takes neither branch keeps o bit for bit.
    A candidate within that of max_offset could be accepted on one side and rejected on the other: the tests' cases keep clear of it and
    assert so from their own inputs.

lookup.  placed_bound(ref, T, X, grid, R, positions, normal_bias, placement): per channel
        |gpu - ref| <= 2^-24 |ref| + (c u + eps_w) T
    without depth maps: probe_lookup_ref's count with one more addition for P' = P + o (a correctly rounded sum of bit-equal operands,
    counted all the same), and, without wrap, the 7 additions and the division of the normalisation that fw_probe_irradiance does not
    have there: c = rounding_count(wrap) + 1 (+ 8 without wrap), eps_w = 0.
    with depth maps: probe_depth_ref's vis_bound with the same one more addition in kappa, the relative perturbation of r' = q - P':
        kappa = u (3 Q' + bias (S + 2)) / dist + u,      Q' = Q + max |o|
    and skipped corners left out of the maximum over corners (nothing of them enters a sum).  c = 34 as there."""
import numpy as np

import probe_depth_ref as PD
import probe_lookup_ref as L

S = L.S
U = 2.0 ** -53

survey_dist_rel = (S + 3) * U
argmin_gap = 1e-9
assert argmin_gap > 2 * survey_dist_rel


def survey_gap(rays, hits_t, hits_normal, hits_object, D: int) -> float:
    """the smallest relative difference between the nearest and the runner-up distance of a class over all probes, exact ties left out
    (they are resolved by index on both sides); inf when no class has two different distances"""
    d = np.asarray(rays, np.float32).astype(np.float64).reshape(-1, D, 6)[..., 3:]
    t = np.asarray(hits_t, np.float32).astype(np.float64).reshape(-1, D)
    nr = np.asarray(hits_normal, np.float32).astype(np.float64).reshape(-1, D, 3)
    obj = np.asarray(hits_object).astype(np.uint32).reshape(-1, D)
    hit = ~np.all(d == 0.0, axis=2) & (obj != np.uint32(0xFFFFFFFF))
    dist = t * np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    back = hit & (((nr[..., 0] * d[..., 0] + nr[..., 1] * d[..., 1]) + nr[..., 2] * d[..., 2]) > 0.0)
    gap = np.inf
    for m in (back, hit & ~back):
        for p in range(d.shape[0]):
            v = np.unique(dist[p][m[p]])
            if v.size >= 2:
                gap = min(gap, (v[1] - v[0]) / max(abs(v[1]), 1e-300))
    return float(gap)


def survey_dist_bound(ref_dist) -> np.ndarray:
    return (survey_dist_rel + 2.0 ** -24 * (1.0 + survey_dist_rel)) * np.abs(np.asarray(ref_dist, np.float64))


def step_bound(placement, survey, min_front: float, back_fraction: float, directions: int) -> np.ndarray:
    """(N, 3): the bound above, per component, from the placement before the step and the survey: dist is the distance of the branch
    that makes the candidate — the back face's for a probe inside, the front face's for one too near it — and a probe that takes neither
    branch keeps its offset bit for bit: 0"""
    o = np.abs(np.asarray(placement, np.float32).astype(np.float64).reshape(-1, 4)[:, 0:3])
    sv = np.asarray(survey, np.float32).astype(np.float64).reshape(-1, 3, 4)
    mf = float(np.float32(min_front))
    inside = sv[:, 2, 0] > float(np.float32(back_fraction)) * float(int(directions))
    near = ~inside & (sv[:, 2, 1] > 0.0) & (sv[:, 1, 3] < mf)
    dist = np.where(inside, sv[:, 0, 3], sv[:, 1, 3])
    bound = 2.0 ** -23 * (o + np.where(np.isfinite(dist), dist, 0.0)[:, None] + mf)
    return np.where((inside | near)[:, None], bound, 0.0)


def placed_bound(ref, T, X, grid, R, positions, normal_bias: float, placement) -> np.ndarray:
    """the bound above for api.probe_lookup_placed(..., terms=True)'s (ref, T, X); R None: no depth maps"""
    ref, T = np.asarray(ref, np.float64), np.asarray(T, np.float64)
    if R is None:
        c = L.rounding_count(grid.wrap) + 1 + (0 if grid.wrap else 8)
        return 2.0 ** -24 * np.abs(ref) + c * U * T
    p = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    omax = float(np.abs(np.asarray(placement, np.float32)[:, 0:3]).max())
    Q = (np.maximum(np.abs(p).max(axis=1) + float(normal_bias), max(abs(v) for v in tuple(grid.lo) + tuple(grid.hi))) + omax)[:, None]
    dist, mu, mu2 = X["dist"], X["mu"], X["mu2"]
    with np.errstate(all="ignore"):
        kappa = U * (3.0 * Q + float(normal_bias) * (S + 2)) / dist + U
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
    rel_fac = PD.REL_FAC * U if grid.wrap else 0.0
    rel_g = np.where(X["active"], 3.0 * (rel_fac + rel_v + U) + 3.0 * U, 0.0)
    eps = (2.0 * (rel_g.max(axis=1) + U) + 8.0 * U)[:, None]
    return 2.0 ** -24 * np.abs(ref) + (L.rounding_count(False) * U + eps) * T


# ---- closed-form scenes: the hits a walk would report, from the numpy lattice ------------------------------------------------------------
MISS = np.uint32(0xFFFFFFFF)


def sphere_hits(rays, radius: float = 1.0):
    """(t, normal, object) of rays from inside or outside a sphere of `radius` at the origin with outward normals, in float64 rounded to
    float32 once: the nearest root above 0"""
    r = np.asarray(rays, np.float32).astype(np.float64)
    o, d = r[:, 0:3], r[:, 3:6]
    a = (d * d).sum(axis=1)
    b = (o * d).sum(axis=1)
    c = (o * o).sum(axis=1) - radius * radius
    disc = b * b - a * c
    with np.errstate(all="ignore"):
        sq = np.sqrt(np.maximum(disc, 0.0))
        t0, t1 = (-b - sq) / a, (-b + sq) / a
        t = np.where(t0 > 1e-3, t0, t1)
        ok = (disc >= 0.0) & (t > 1e-3)
    pt = o + t[:, None] * d
    nrm = np.where(ok[:, None], pt / radius, 0.0).astype(np.float32)
    return np.where(ok, t, 0.0).astype(np.float32), nrm, np.where(ok, np.uint32(0), MISS).astype(np.uint32)


def floor_hits(rays, height: float = 0.0):
    """(t, normal, object) of rays against the plane y = height, normal +y, seen from both sides (a single-sided wall: from below the
    ray meets its back)"""
    r = np.asarray(rays, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = (height - r[:, 1]) / r[:, 4]
    ok = np.isfinite(t) & (t > 1e-3)
    nrm = np.zeros((r.shape[0], 3), np.float32)
    nrm[ok, 1] = 1.0
    return np.where(ok, t, 0.0).astype(np.float32), nrm, np.where(ok, np.uint32(0), MISS).astype(np.uint32)


def no_hits(rays):
    n = np.asarray(rays).shape[0]
    return np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.full(n, MISS, np.uint32)
