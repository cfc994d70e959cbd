"""The bound of tests/test_gpu_ggx_table.py on |device - statement| for fw_ggx_terms, derived here and nowhere measured
on the device, and the inputs that go with it.

Both sides — api.ggx_terms in numpy and k_ggx_terms — run one sequence of IEEE float64 operations in one order.  + - * round correctly
on both, so from equal operands they give equal results; a sine, a cosine, a square root or a division may differ: the device's may be
its library's, allowed 2 ulps here.  What this module accounts for is how such a difference is carried to the sums, not the distance
of the quadrature from the integral.

The account is a running forward error analysis over the test's own samples: every intermediate x of the statement carries a bound e_x
on |x' - x|, x' the other side's value.
    x + y, x - y   e = e_x + e_y + ETA |result|
    x y            e = |x| e_y + |y| e_x + e_x e_y + ETA |result|          (+ - *: no ETA where e_x = e_y = 0 — equal operands, equal results)
    x / y          e = (e_x + |x / y| e_y) / (|y| - e_y) + ETA_P |result|
    sqrt x         e = e_x / (2 sqrt(x - e_x)) + ETA_P |result|                (x - e_x > 0 is asserted: `fit`)
    sin, cos       e = e_x + ETA_P                                             (|d/dx| <= 1, |result| <= 1)
    max(x, c)      e = e_x                                                     (1-Lipschitz)
ETA = 2^-51 covers the two sides' own roundings of an exactly rounded operation (half an ulp each, 2^-52 together) twice over;
ETA_P = 2^-50 a result that is 2 ulps off (2^-51) and the statement's own half ulp, again with room.  Nothing else is assumed: the one
ill-conditioned step, nz = sqrt(1 - p1^2 - p2^2) (its argument falls to 1 / (2 m1) at the rim of the disc, and an error of the argument is
amplified by 1 / (2 nz)), the division by |g| >= alpha in h = g / |g| and the division by wi.z^2 near the horizon are all carried by
these rules with the values the samples really take; `amp` reports the first.

Every term k (1 - Fc), k Fc is non-negative, so a lane's running sum never exceeds the sum of its terms and the additions cost at most
(trips + 9) ETA sum|term| (trips per lane, six in the xor tree, three across the waves); the division by m1 m2 costs ETA_P.  With
S = sum|term| / (m1 m2):
    |float64 device - float64 statement| <= K 2^-53 S,     K = (sum e_term / sum|term|) 2^53 + 4 (trips + 9) + 8
and the device's float32 is the rounding of its float64: |device - x| <= 2^-24 |x| + K 2^-53 S (1 + 2^-24).  K 2^-53 < 2^-30 is
asserted by the test for every pair: a float32 evaluation, whose K 2^-53 is 2^-24 at the very least, fails it.

The decision wi.z > 0 is a select in the sums: the bound holds only where both sides decide alike, so every sample's |wi.z| must
exceed its own error bound; the test asks for 2^-40, far above it, on the CPU and before the device is asked.  A pair that cannot
satisfy that, or whose root arguments are not safely positive, is `unfit` and replaced (pairs())."""
import numpy as np

ETA = 2.0 ** -51
ETA_P = 2.0 ** -50
WZ_MARGIN = 2.0 ** -40
K_LIMIT = 2.0 ** -30


def _eta(a, b):
    """ETA, or 0 where both operands are the same on both sides: a correctly rounded operation then gives the same result on both"""
    return np.where((a.e == 0.0) & (b.e == 0.0), 0.0, ETA)


class V:
    """a float64 array with a bound on the other side's distance from it"""

    def __init__(self, x, e=0.0):
        self.x = np.asarray(x, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.x.shape) if np.ndim(e) == 0 else np.asarray(e, np.float64)

    @staticmethod
    def of(v):
        return v if isinstance(v, V) else V(np.float64(v))

    def __add__(self, o):
        o = V.of(o)
        x = self.x + o.x
        return V(x, self.e + o.e + _eta(self, o) * np.abs(x))

    def __sub__(self, o):
        o = V.of(o)
        x = self.x - o.x
        return V(x, self.e + o.e + _eta(self, o) * np.abs(x))

    def __rsub__(self, o):
        return V.of(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = V.of(o)
        x = self.x * o.x
        return V(x, np.abs(self.x) * o.e + np.abs(o.x) * self.e + self.e * o.e + _eta(self, o) * np.abs(x))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        x = self.x / o.x
        den = np.abs(o.x) - o.e
        return V(x, np.where(den > 0, (self.e + np.abs(x) * o.e) / np.where(den > 0, den, 1.0), np.inf) + ETA_P * np.abs(x))

    def sqrt(self):
        x = np.sqrt(self.x)
        lo = self.x - self.e
        e = np.where(self.e == 0.0, 0.0, np.where(lo > 0, self.e / (2.0 * np.sqrt(np.where(lo > 0, lo, 1.0))), np.inf))
        return V(x, e + ETA_P * np.abs(x))

    def fmax(self, c):
        return V(np.fmax(self.x, c), self.e)


def exact(x):
    return V(x, 0.0)


def terms_bound(mu, rho, m1, m2):
    """(AB (n, 2) float64, bound (n, 2), info) for float32 pairs: AB is api.ggx_terms' float64 value before its rounding (asserted equal
    by the CPU test), bound the allowance on |device float32 - AB|, info a dict of (n,) or (n, 2) arrays: K (bound's K), S, min_wz, amp,
    fit (every root argument safely positive, every |wi.z| above WZ_MARGIN and its own error bound)."""
    m1, m2 = int(m1), int(m2)
    muf = np.asarray(mu, np.float32).reshape(-1)
    rhof = np.asarray(rho, np.float32).reshape(-1)
    n = muf.shape[0]
    with np.errstate(all="ignore"):
        ok = (muf > 0) & (muf <= 1) & (rhof >= 0) & (rhof <= 1)
        cm = exact(np.where(ok, muf, np.float32(1.0)).astype(np.float64)[:, None])
        alpha = exact(np.where(ok, rhof * rhof, np.float32(0.0)).astype(np.float64)[:, None])
        a2 = alpha * alpha
        sx = (1.0 - cm * cm).fmax(0.0).sqrt()
        vx = alpha * sx
        vl = (vx * vx + cm * cm).sqrt()
        vhx, vhz = vx / vl, cm / vl
        s = 0.5 * (1.0 + vhz)
        s1 = 1.0 - s
        lo1 = 1.0 + 0.5 * ((1.0 + a2 * ((sx * sx) / (cm * cm))).sqrt() - 1.0)
        sr = (exact(np.arange(m1, dtype=np.float64) + 0.5) / exact(float(m1))).sqrt()
        phi = exact(2.0 * np.pi) * (exact(np.arange(m2, dtype=np.float64) + 0.5) / exact(float(m2)))
        cphi, sphi = V(np.cos(phi.x), phi.e + ETA_P), V(np.sin(phi.x), phi.e + ETA_P)
        total = m1 * m2
        trips = (total + 255) // 256
        accA, accB = np.zeros((n, 256)), np.zeros((n, 256))
        errA, errB = np.zeros(n), np.zeros(n)
        absA, absB = np.zeros(n), np.zeros(n)
        min_wz, amp, fit = np.full(n, np.inf), np.zeros(n), np.ones(n, bool)
        for it in range(trips):
            raw = it * 256 + np.arange(256)
            valid = (raw < total)[None, :]
            ids = np.minimum(raw, total - 1)
            a, b = ids // m2, ids % m2
            r, cp, sp = V(sr.x[a][None, :], sr.e[a][None, :]), V(cphi.x[b][None, :], cphi.e[b][None, :]), V(sphi.x[b][None, :], sphi.e[b][None, :])
            p1 = r * cp
            q1 = 1.0 - p1 * p1
            p2 = s1 * q1.fmax(0.0).sqrt() + s * (r * sp)
            arg = q1 - p2 * p2
            nz = arg.fmax(0.0).sqrt()
            nhx, nhz = nz * vhx - p2 * vhz, p2 * vhx + nz * vhz
            gx, gy, gz = alpha * nhx, alpha * p1, nhz.fmax(0.0)
            hl = ((gx * gx + gy * gy) + gz * gz).sqrt()
            hx, hy, hz = gx / hl, gy / hl, gz / hl
            oh = sx * hx + cm * hz
            t2 = 2.0 * oh
            wx, wy, wz = t2 * hx - sx, t2 * hy, t2 * hz - cm
            alive = wz.x > 0.0
            zz = V(np.where(alive, wz.x, 1.0), np.where(alive, wz.e, 0.0))
            xy0 = wx * wx + wy * wy
            xy = V(np.where(alive, xy0.x, 0.0), np.where(alive, xy0.e, 0.0))
            li = 0.5 * ((1.0 + a2 * (xy / (zz * zz))).sqrt() - 1.0)
            k0 = lo1 / (lo1 + li)
            use = alive & valid
            k = V(np.where(use, k0.x, 0.0), np.where(use, k0.e, 0.0))
            m = (1.0 - oh).fmax(0.0)
            fc = ((m * m) * (m * m)) * m
            tA, tB = k * (1.0 - fc), k * fc
            accA = accA + tA.x
            accB = accB + tB.x
            errA += np.sum(np.where(valid, tA.e, 0.0), axis=1)
            errB += np.sum(np.where(valid, tB.e, 0.0), axis=1)
            absA += np.sum(np.abs(tA.x), axis=1)
            absB += np.sum(np.abs(tB.x), axis=1)
            min_wz = np.minimum(min_wz, np.min(np.where(valid, np.abs(wz.x), np.inf), axis=1))
            amp = np.maximum(amp, np.max(np.where(valid & (arg.x > 0), 0.5 / np.where(arg.x > 0, arg.x, 1.0), 0.0), axis=1))
            safe = (arg.x - arg.e > 0) & (q1.x - q1.e > 0) & (np.abs(wz.x) >= WZ_MARGIN) & (np.abs(wz.x) > 4.0 * wz.e) & np.isfinite(tA.e) & np.isfinite(tB.e)
            fit &= np.all(safe | ~valid, axis=1)

        def tree(v):
            v = v.reshape(n, 4, 64)
            lanes = np.arange(64)
            for d in (32, 16, 8, 4, 2, 1):
                v = v + v[:, :, lanes ^ d]
            w = v[:, :, 0]
            return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]

        count = float(m1) * float(m2)
        AB = np.stack([tree(accA) / count, tree(accB) / count], axis=1)
        err, tot = np.stack([errA, errB], axis=1), np.stack([absA, absB], axis=1)
        K = np.where(tot > 0, err / np.where(tot > 0, tot, 1.0), 0.0) * 2.0 ** 53 + 4.0 * (trips + 9) + 8.0
        S = tot / count
        bound = 2.0 ** -24 * np.abs(AB) + K * 2.0 ** -53 * S * (1.0 + 2.0 ** -24)
        AB, bound, K, S = (np.where(ok[:, None], v, 0.0) for v in (AB, bound, K, S))
    return AB, bound, {"K": K, "S": S, "min_wz": np.where(ok, min_wz, np.inf), "amp": np.where(ok, amp, 0.0), "fit": fit | ~ok, "ok": ok}


QUADS = [(1, 1), (3, 2), (9, 7), (8, 8), (13, 5), (17, 15), (16, 16), (257, 1), (40, 25)]       # m1 m2 = 1, 6, 63, 64, 65, 255, 256, 257, 1000
COUNTS = [1, 5, 200]
MAX_REPLACED = 0.1


def raw_pairs(n, seed):
    """n seeded float32 pairs: the corners the issue names first — rho = 0, rho = 1, mu = 1, mu = 2^-6, a mu and a rho out of range, a
    NaN of each — then uniform ones with mu in [2^-6, 1] and rho in [0, 1].  n = 1: one in-range pair."""
    rng = np.random.default_rng(seed)
    mu = (2.0 ** -6 + (1.0 - 2.0 ** -6) * rng.random(n)).astype(np.float32)
    rho = rng.random(n).astype(np.float32)
    if n >= 5:
        fixed = [(0.6, 0.0), (0.3, 1.0), (1.0, 0.4), (2.0 ** -6, 0.5)]
        if n >= 12:
            fixed += [(0.0, 0.5), (-0.25, 0.5), (1.5, 0.5), (0.5, -0.125), (0.5, 1.25), (np.nan, 0.5), (0.5, np.nan)]
        for i, (m, r) in enumerate(fixed):
            mu[i], rho[i] = m, r
    return mu, rho


def pairs(n, seed, m1, m2):
    """(mu, rho, replaced): raw_pairs with every unfit pair replaced by a fresh seeded one (up to eight tries each); the test asserts
    replaced <= MAX_REPLACED n; the seeds in use need none"""
    mu, rho = raw_pairs(n, seed)
    fit = terms_bound(mu, rho, m1, m2)[2]["fit"]
    replaced = int(np.sum(~fit))
    rng = np.random.default_rng(seed + 7919)
    for _ in range(8):
        bad = np.nonzero(~fit)[0]
        if bad.size == 0:
            break
        mu[bad] = (2.0 ** -6 + (1.0 - 2.0 ** -6) * rng.random(bad.size)).astype(np.float32)
        rho[bad] = rng.random(bad.size).astype(np.float32)
        fit[bad] = terms_bound(mu[bad], rho[bad], m1, m2)[2]["fit"]
    assert np.all(fit), "no fit replacement found"
    return mu, rho, replaced
