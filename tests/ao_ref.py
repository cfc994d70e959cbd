"""Bounds and fixtures shared by the ambient-occlusion tests (tests/test_ao_cpu.py, tests/test_gpu_ao.py); the statements themselves are
api.ao_rays, api.ao_reduce and api.ao_resolve (include/firework_hip.h).

Nothing here is measured on the GPU: every quantity comes from the test's own inputs and the numpy statement.  u = 2^-53 throughout.
As in tests/probe_depth_ref.py the device and numpy evaluate the same float64 expression operation for operation — api.ao_reduce sums
in the device's own order: G partial sums, then the xor butterfly — and + - * / are correctly rounded on both sides, so the two can first
part at the square root, where S = 4 float64 ulps are allowed for; from there every later operation adds one more rounding's worth of
difference.  The bounds are first-order in u.

reduce_bound(acc, T, A, prior, D) — fw_ao_reduce.  Per point and accumulator (Bx, By, Bz, O), acc = (1 / D) sum_j term_j
    |gpu - (prior + acc)| <= e + 2^-24 (|prior| + |acc| + e),    e = 2^-24 |acc| + u ((S + 7) A + (D + 2) T)
  the float64 terms
    dist = t * sqrt((dx dx + dy dy) + dz dz): the squares and their sums are bit-equal, the root carries S, the product one more: S + 1
        relative (written S + 3 as §9s writes it: the same expression).
    o: with falloff 0 it is exactly 0 or 1 on both sides PROVIDED both sides decide dist >= radius alike.  The test guarantees that: it
        asserts on the CPU, before the device is asked, that no dist lies within 1e-6 radius of radius, and (S + 3) u is 1e-9 of that
        margin.  A miss is exactly 0.  With falloff 1, o = 1 - dist / radius: the quotient carries S + 4 relative and is below 1, the
        subtraction adds u |o| <= u: |do| <= (S + 5) u.
    w = 1 - o: |dw| <= (S + 6) u.  The terms: w d_k is off by at most (S + 7) u |d_k|; o by (S + 5) u <= (S + 7) u x 1.
        Summed over j and divided by D: (S + 7) u A with A_k = (1 / D) sum_j |d_jk| over the non-zero rays, and A = (number of non-zero
        rays) / D for O.  (With falloff 0 these differences are zero; the bound does not use that.)
    the sum: every value is the result of at most ceil(D / G) + log2 G <= D additions in the same order on both sides, each rounding by at
        most u of a partial sum, which sum_j |term_j| bounds: D u T with T = (1 / D) sum_j |term_j| (api.ao_reduce(..., terms=True));
        the product with 1 / D — itself one rounding of 1 / D, the same bits on both sides — one more: (D + 2) u T in all.
  half an ulp of float32 per accumulator, for the one rounding: 2^-24 |acc| (of the device's own float64 value: first order).
  the float32 addition to the running sum: 2^-24 of its exact result, at most |prior| + |acc| + e.
  If the device's float64 sqrt is correctly rounded the float64 accumulators are bit-equal and only the two float32 roundings remain.

occluder_count(D, rho, h): the closed form of §9o's occluder.  A sphere of radius rho centred h > rho above the point on its normal
subtends sin(theta) < rho / h; a lattice ray has sin^2(theta) = u_j = (j + xi_u) / D, so it hits iff u_j < rho^2 / h^2.  The u_j are one
per cell [j / D, (j + 1) / D), so the number of hits is within 1 of D rho^2 / h^2 whatever the shift: |ao - (1 - rho^2 / h^2)| <= 1 / D."""
import numpy as np

from firework_amd import _abi as A
from firework_amd import _lib

S = 4
U = 2.0 ** -53
MISS = np.uint32(0xFFFFFFFF)


def abs_dirs(rays, D: int) -> np.ndarray:
    """A (n, 4) of the derivation above from the stored rays (n * D, 6)"""
    d = np.abs(np.asarray(rays, np.float32).astype(np.float64).reshape(-1, D, 6)[..., 3:])
    nonzero = np.any(d != 0.0, axis=-1)
    return np.concatenate([d.sum(axis=1), nonzero.sum(axis=1, keepdims=True).astype(np.float64)], axis=1) / float(D)


def reduce_bound(acc, T, Aabs, prior, D: int) -> np.ndarray:
    """the bound above for api.ao_reduce(..., terms=True)'s (acc, T), abs_dirs' A and the float32 sums before the call (n, 4 each)"""
    acc = np.abs(np.asarray(acc, np.float64))
    e = 2.0 ** -24 * acc + U * ((S + 7) * np.asarray(Aabs, np.float64) + (D + 2) * np.asarray(T, np.float64))
    return e + 2.0 ** -24 * (np.abs(np.asarray(prior, np.float64)) + acc + e)


def clear_of_radius(dist, radius: float) -> bool:
    """the condition the reduce tests assert before the device is asked: no traced distance within 1e-6 radius of radius"""
    d = np.asarray(dist, np.float64)
    d = d[np.isfinite(d)]
    return bool(np.isinf(radius) or np.all(np.abs(d - radius) > 1e-6 * radius))


def hand_made(n, D, radius, rng):
    """rays with directions of length 0.5 .. 2 — every seventh ray all zero — and hits that miss, lie beyond the radius, sit at t = 0 and
    in between, in turn; drawn so that no dist is within 1e-6 radius of radius (t lies in [0, 0.45 r] or at 3 r, |d| in [0.5, 2])"""
    r = 4.0 if np.isinf(radius) else float(radius)
    d = rng.normal(size=(n * D, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n * D, 1))
    rays = np.zeros((n * D, 6), np.float32)
    rays[:, :3] = rng.normal(size=(n * D, 3))
    rays[:, 3:] = d
    rays[(np.arange(n * D) + 3) % 7 == 0] = 0.0
    hits = np.zeros(n * D, _lib.HIT_DTYPE)
    kind = (np.arange(n * D) + rng.integers(4)) % 4
    hits["t"] = rng.uniform(0.001, 0.45 * r, size=n * D)
    hits["t"][kind == 1] = 3.0 * r
    hits["t"][kind == 2] = 0.0
    hits["object"] = rng.integers(0, 9, size=n * D)
    hits["object"][kind == 0] = A.FW_NO_HIT
    hits["t"][kind == 0] = 0.0                                                           # a miss has every other field 0
    hits["point"], hits["normal"], hits["prim"] = rng.normal(size=(n * D, 3)), rng.normal(size=(n * D, 3)), 5   # never read
    return rays, hits


def points(n, rng, unusable=True):
    """n float32 surface points: normals (0, 0, 1), (0, 0, -1) (the frame's two poles), unit and unnormalised ones in turn; with
    `unusable`, points 4, 9 and 14 (where they exist) carry a NaN position, an infinite normal component and a zero normal"""
    pos = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]
    nrm = nrm.astype(np.float32)
    nrm[0::6] = (0.0, 0.0, 1.0)
    nrm[1::6] = (0.0, 0.0, -1.0)
    if unusable:
        if n > 4:
            pos[4, 1] = np.nan
        if n > 9:
            nrm[9, 0] = np.inf
        if n > 14:
            nrm[14] = 0.0
    return pos, nrm


def sphere_hits(rays, centre, rho):
    """(t float32, object uint32) of the rays (m, 6) against one sphere, in float64: the nearer root where it is positive, else a miss"""
    o, d = rays[:, :3].astype(np.float64) - np.asarray(centre, np.float64), rays[:, 3:].astype(np.float64)
    a, b, c = (d * d).sum(axis=1), (o * d).sum(axis=1), (o * o).sum(axis=1) - rho * rho
    with np.errstate(all="ignore"):
        disc = b * b - a * c
        t = (-b - np.sqrt(disc)) / a
    hit = (disc > 0.0) & (t > 0.0)
    return np.where(hit, t, 0.0).astype(np.float32), np.where(hit, np.uint32(0), MISS).astype(np.uint32)
