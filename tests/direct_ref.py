"""Bounds and fixtures shared by the direct-light tests (tests/test_direct_cpu.py, tests/test_gpu_direct.py); the statements themselves
are api.direct_rays, api.direct_reduce and api.direct_resolve (include/firework_hip.h).

Nothing here is measured on the GPU: every quantity comes from the test's own inputs and the numpy statement.  u = 2^-53 throughout.
As in tests/ao_ref.py the device and numpy evaluate the same float64 expression operation for operation — api.direct_reduce sums in the
device's own order: G partial sums, then the xor butterfly — and + - * / are correctly rounded on both sides, so the two can first part
at a square root, where S = 4 float64 ulps are allowed for; from there every later operation adds one more rounding's worth of
difference, multiplied by the condition of the operation it enters.  The bounds are first-order in u.

ray_bound(rays) — fw_direct_rays.  §9k's bound: a stored component differs from the statement's by at most 2^-23 x the largest
    component of its vector (origin or direction): the float64 values differ by a few u relative to that magnitude — the square root
    of the normal's length, three divisions, a product and a sum — and 2^-23 is one float32 ulp of it, 2^29 times more.  Which entries
    are zero must agree exactly; well_clear() is the condition under which they must, asserted on the CPU before the device is asked.

well_clear(terms, lights) — no culling decision within 64 ulp of its threshold: every c = nh . w is further than 64 x 2^-52 from 0
    (|c| <= 1, so that is 64 float64 ulps of the largest value it takes), every spot cosine cs further than 64 x 2^-52 from cos_outer
    (where the factor s leaves 0), every d2 above 0 by more than 64 ulps of itself.  The device's c, cs and d2 differ from numpy's by
    at most (S + 8) u x 3 — the root, the division, a dot product of three products of magnitude <= 1 — well inside 64 x 2^-52.

reduce_bound(acc, T, prior, Ln) — fw_direct_reduce.  Per point and accumulator (E.rgb, N, S.rgb), acc = sum_i term_i
    |gpu - (prior + acc)| <= e + 2^-24 (|prior| + |acc| + e),    e = 2^-24 |acc| + u (K C + Ln + 1) T,   T = sum_i |term_i|
  the float64 terms.  A term is the result of fewer than K = 128 float64 operations (a glossy term: about 110; a diffuse one: about
    40), at most four of them square roots; each rounds by u (a root by S u) relative to its own result, and an operation that cancels
    multiplies what it received by its condition.  well_conditioned() asserts on the CPU what bounds every such condition by C = 2^18:
        c = nh . w and co = nh . wo at least 2^-5 on every entry that contributes: 1 / c and 1 / co enter squared in Smith's
            tangent (x - z nh)^2 / z^2: <= 2^10;
        rho >= 0.03, GgxMat's own floor: alpha = rho^2 >= 9e-4, and hn = nh . h >= (c + co) / |wo + w| >= 2^-5: the cancelling
            tangential part h - hn nh enters sd = |.|^2 + a2 hn^2 with condition <= 1 / (alpha hn) < 2^15.2 (AM-GM on the two parts of
            sd), and D = a2 / (pi sd^2) doubles it: < 2^16.2;
        F0 >= 2^-6 on every glossy point: m = 1 - oh cancels, F = F0 + (1 - F0) m^5 is off by at most 5 times that absolutely, and F
            >= F0: <= 5 x 2^6 < 2^8.4;
        a spot's smoothstep t t (3 - 2 t) has condition 2 / t relative to t, t = (cs - co) / (ci - co): entries with 0 < t < 2^-10
            are excluded; cs - co cancels with condition |cs| / (cs - co) <= 1 / (2^-10 (ci - co)), with ci - co >= 2^-6 asserted:
            <= 2^17 in all.
    The conditions do not multiply with one another beyond these products (they sit in different factors of the term, whose relative
    errors add), so K C u bounds the relative difference of a term and K C u T the sum of the terms' differences.
  the sum: every value is the result of at most ceil(Ln / G) + log2 G <= Ln additions in the same order on both sides, each rounding by
    at most u of a partial sum, which T bounds: Ln u T, written with one to spare: (Ln + 1) u T.
  half an ulp of float32 per accumulator, for the one rounding: 2^-24 |acc| (of the device's own float64 value: first order).
  the float32 addition to the running sum: 2^-24 of its exact result, at most |prior| + |acc| + e.
  K C u = 2^-28 is a sixteenth of the float32 rounding: a float32 evaluation of a term, off by 2^-24 per operation, fails the bound.
  N is a sum of ones: exact in float64, and exact in float32 below 2^24; the tests assert it with ==.

shadow_radius(R, a, h): a sphere of radius R centred at height a above a floor point P under a point light at height h > a + R on the
    same vertical shadows exactly the floor points closer to P than h tan(theta), sin(theta) = R / (h - a): the cone of tangents from
    the light."""
import numpy as np

from firework_amd import _abi as A
from firework_amd import _lib, api

S = 4
U = 2.0 ** -53
K = 128
C = 2.0 ** 18
MISS = np.uint32(0xFFFFFFFF)
CLEAR = 64.0 * 2.0 ** -52


def ray_bound(ref) -> np.ndarray:
    """(m, 6): 2^-23 x the largest component of the origin (columns 0..2) and of the direction (3..5) of the statement's rays"""
    r = np.abs(np.asarray(ref, np.float32).astype(np.float64).reshape(-1, 6))
    return 2.0 ** -23 * np.concatenate([np.repeat(r[:, 0:3].max(axis=1, keepdims=True), 3, axis=1),
                                        np.repeat(r[:, 3:6].max(axis=1, keepdims=True), 3, axis=1)], axis=1)


def well_clear(terms, lights) -> bool:
    """the condition the ray tests assert before the device is asked (see above); entries with a NaN quantity (an unusable point, a
    light at the point itself) decide by other means and are skipped"""
    kind, rec = api.light_records(lights)
    c, cs, d2 = terms["c"], terms["cs"], terms["d2"]
    ok = np.isfinite(c)
    good = np.all(np.abs(c[ok]) > CLEAR)
    spot = np.isfinite(cs) & ok
    co = np.broadcast_to(rec[None, :, 11], cs.shape)
    good &= np.all(np.abs(cs[spot] - co[spot]) > CLEAR)
    good &= np.all((d2[ok] == 0.0) | (d2[ok] > 1e-300))
    return bool(good)


def reduce_bound(acc, T, prior, Ln: int) -> np.ndarray:
    """the bound above for api.direct_reduce(..., terms=True)'s (acc, T) and the float32 sums before the call (n, 7 each)"""
    acc = np.abs(np.asarray(acc, np.float64))
    e = 2.0 ** -24 * acc + U * (K * C + Ln + 1) * np.asarray(T, np.float64)
    return e + 2.0 ** -24 * (np.abs(np.asarray(prior, np.float64)) + acc + e)


def _conditions(direct, lights, positions, normals, rays, ids, view, spec):
    """(bad entries (n, Ln), bad points (n,), the lights' own condition): where reduce_bound's C does not hold (see above), among the
    entries whose stored ray is not zero"""
    kind, rec = api.light_records(lights)
    ids_, p32, ok, nh, vw, sp = api._direct_points(direct, positions, normals, ids, view, spec)
    n, Ln = ids_.size, kind.size
    d = np.asarray(rays, np.float32).astype(np.float64).reshape(n, Ln, 6)[..., 3:]
    live = np.any(d != 0.0, axis=-1) & ok[:, None]
    if sp is not None:
        live &= ~(sp[:, 3] < 0)[:, None]
    bad_point = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        d2, w, s = api._direct_geometry(kind, rec, d)
        c = api._dot3(nh[:, None, :], w)
        live &= c > 0.0
        bad = live & ~(c >= 2.0 ** -5)
        ci, co = np.broadcast_to(rec[None, :, 7], c.shape), np.broadcast_to(rec[None, :, 11], c.shape)
        ramp = (kind == 1) & (rec[:, 7] > rec[:, 11])
        lights_ok = bool(np.all((rec[:, 7] - rec[:, 11])[ramp] >= 2.0 ** -6))
        t = (-api._dot3(w, rec[None, :, 4:7]) - co) / (ci - co)
        bad |= live & ramp[None, :] & (t > 0.0) & (t < 2.0 ** -10)
        if sp is not None and np.any(sp[:, 3] > 0):
            glossy = sp[:, 3] > 0
            wo = -(vw / np.sqrt(api._dot3(vw, vw))[:, None])
            co_v = api._dot3(nh, wo)
            bad_point = glossy & ((co_v > 0.0) & (co_v < 2.0 ** -5) | (sp[:, 3] < np.float32(0.03)) | np.any(sp[:, 0:3] < 2.0 ** -6, axis=1))
    return bad, bad_point, lights_ok


def well_conditioned(direct, lights, positions, normals, rays, ids=None, view=None, spec=None) -> bool:
    """the conditions reduce_bound's C rests on (see above), asserted on the CPU before the device is asked"""
    bad, bad_point, lights_ok = _conditions(direct, lights, positions, normals, rays, ids, view, spec)
    return lights_ok and not bad.any() and not bad_point.any()


def tame(direct, lights, positions, normals, rays, ids=None, view=None, spec=None):
    """(rays, spec) made well conditioned by hand: an entry that is not gets a zero ray, a glossy point that is not becomes diffuse (its
    spec record is indexed by id)"""
    bad, bad_point, _ = _conditions(direct, lights, positions, normals, rays, ids, view, spec)
    rays = np.array(rays, np.float32).reshape(bad.shape + (6,))
    rays[bad] = 0.0
    if spec is not None:
        spec = np.array(spec, np.float32)
        at = np.arange(spec.shape[0]) if ids is None else np.asarray(ids).astype(np.int64)
        spec[at[bad_point], 3] = 0.0
    return rays.reshape(-1, 6), spec


def shadow_radius(R: float, a: float, h: float) -> float:
    s = R / (h - a)
    return h * s / np.sqrt(1.0 - s * s)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def lights(Ln: int, rng):
    """Ln lights of mixed kinds, in turn point, spot, directional, a spot with cos_inner == cos_outer, a dark point light (every 11th):
    positions 2..5 above and around the origin's unit cube, spots aimed near the origin with cones that cut through the points"""
    out = []
    for i in range(Ln):
        pos = rng.uniform(-4.0, 4.0, size=3)
        pos[1] = rng.uniform(2.0, 5.0)
        inten = rng.uniform(1.0, 30.0, size=3)
        k = i % 4
        if i % 11 == 10:
            out.append(api.PointLight(pos, (0.0, 0.0, 0.0)))
        elif k == 0:
            out.append(api.PointLight(pos, inten))
        elif k == 1:
            out.append(api.SpotLight(pos, -pos + rng.uniform(-0.5, 0.5, size=3), inten, rng.uniform(5.0, 15.0), rng.uniform(25.0, 40.0)))
        elif k == 2:
            out.append(api.DirectionalLight((rng.uniform(-1, 1), -rng.uniform(0.3, 1.0), rng.uniform(-1, 1)), inten * 0.1))
        else:
            a = rng.uniform(10.0, 30.0)
            out.append(api.SpotLight(pos, -pos, inten, a, a))
    return out


def points(n: int, rng, unusable=True):
    """n float32 surface points in the unit cube around the origin: normals mostly up (so that most lights are in front), some down
    (most lights behind: culled), unnormalised; with `unusable`, points 4, 9 and 14 (where they exist) carry a NaN position, an infinite
    normal component and a zero normal"""
    pos = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)) * 0.3
    nrm[:, 1] += 1.0
    nrm[3::7] *= -1.0
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]).astype(np.float32)
    nrm[0::6] = (0.0, 1.0, 0.0)
    if unusable:
        if n > 4:
            pos[4, 1] = np.nan
        if n > 9:
            nrm[9, 0] = np.inf
        if n > 14:
            nrm[14] = 0.0
    return pos, nrm


def views(pos, rng):
    """directions from an eye above the points: (n, 3) float32, unnormalised"""
    eye = np.array([0.5, 6.0, 7.0])
    return ((pos.astype(np.float64) - eye) * rng.uniform(0.5, 2.0, size=(pos.shape[0], 1))).astype(np.float32)


def specs(n: int, rng):
    """(n, 4) float32 (F0.rgb, rho): in turn diffuse (rho 0), glossy at rho 0.03, 0.3 and 1.0, and a point that takes no light (rho -1)"""
    sp = np.zeros((n, 4), np.float32)
    sp[:, 0:3] = rng.uniform(0.1, 1.0, size=(n, 3))
    sp[:, 3] = np.array([0.0, 0.03, 0.3, 1.0, -1.0], np.float32)[np.arange(n) % 5]
    return sp


def hand_hits(m: int, kinds, rng):
    """hits for m rays towards lights of `kinds` (m,): in turn a miss, t = 0.5, t = 1.0 exactly, t = the float32 just below 1, t = 7 — so
    a directional light sees a hit too — the other fields filled with values that are never read"""
    hits = np.zeros(m, _lib.HIT_DTYPE)
    sel = (np.arange(m) + rng.integers(5)) % 5
    t = np.array([0.0, 0.5, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 7.0], np.float32)[sel]
    hits["t"] = t
    hits["object"] = rng.integers(0, 9, size=m)
    hits["object"][sel == 0] = A.FW_NO_HIT
    hits["point"], hits["normal"], hits["prim"] = rng.normal(size=(m, 3)), rng.normal(size=(m, 3)), 5   # never read
    return hits
