"""What the reflection-gather tests share: an independent float64 restatement of fw_reflect_rays built on ggx_ref (the
frame, Heitz's sampler and Smith's Lambda as GgxMat's own tests state them — another order of operations than api.reflect_rays, so the
two agree to float64 rounding, not bit for bit), a plain-loop restatement of fw_reflect_reduce, and the points the ray tests use."""
import numpy as np

from firework_amd import api

import ggx_ref as G
from gather_ref import F32, add_to, one_probe, random_probes, synthetic_records, u32      # noqa: F401  (shared with the gather tests)

GOLDEN = (np.sqrt(5.0) - 1.0) / 2.0
# the seed of the ray tests: with it no ray of the cases below lies within 1e-9 of the horizon (test_reflect_cpu asserts it)
SEED = 11
DIRECTIONS = (1, 5, 64, 200)
STRIDES = (3, 12, 16)


def lattice(D, xi):
    """(xi1, xi2) (n, D): the shifted Fibonacci lattice of the statement"""
    j = np.arange(D, dtype=np.float64)[None, :]
    t = j * GOLDEN + xi[:, 1:2]
    return (j + xi[:, 0:1]) / float(D), t - np.floor(t)


def rays_ref(reflect, positions, normals, view, spec, ids=None, round=0):
    """dict of float64 arrays for the points id = ids[q]: "origin", "direction" (n, D, 3), "g", "s", "wi_z", "wo_z" (n, D), "alive" (n, D)
    bool, "usable" (n,): fw_reflect_rays' statement through ggx_ref"""
    D = reflect.directions
    P, N = np.asarray(positions, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    V, S = np.asarray(view, F32).reshape(-1, 3), np.asarray(spec, F32).reshape(-1, 4)
    ids = np.arange(P.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)
    at = ids.astype(np.int64)
    p, nr, vw, rho = P[at].astype(np.float64), N[at].astype(np.float64), V[at].astype(np.float64), S[at, 3]
    with np.errstate(all="ignore"):
        usable = (np.all(np.isfinite(p), 1) & np.all(np.isfinite(nr), 1) & np.all(np.isfinite(vw), 1) & np.any(nr != 0, 1) & np.any(vw != 0, 1)
                  & np.isfinite(rho) & (rho > 0))
        xi = api.texel_jitter(reflect._seed, round, ids) if reflect._jitter else np.full((ids.size, 2), 0.5)
        xi1, xi2 = lattice(D, xi)
        alpha = G.alpha_of(rho)[:, None]
        fr = G.frame(nr / np.sqrt(np.sum(nr * nr, -1))[:, None], vw)
        wo = fr[3][:, None, :] + np.zeros((1, D, 1))
        wi, h = G.sample_local(wo, alpha, xi1, xi2)
        alive = (wi[..., 2] > 0.0) & (wo[..., 2] > 0.0) & usable[:, None]
        safe = np.where(alive[..., None], wi, np.array([0.0, 0.0, 1.0]))
        so = np.where(alive[..., None], wo, np.array([0.0, 0.0, 1.0]))
        lo, li = G.lam(so, alpha), G.lam(safe, alpha)
        g = (1.0 + lo) / (1.0 + lo + li)
        s = (1.0 - np.sum(wo * h, -1)) ** 5
        t, b, n, _ = fr
        d = wi[..., 0:1] * t[:, None, :] + wi[..., 1:2] * b[:, None, :] + wi[..., 2:3] * n[:, None, :]
        o = (p + float(F32(reflect._bias)) * n)[:, None, :] + np.zeros((1, D, 1))
    z = lambda a: np.where(alive[..., None] if a.ndim == 3 else alive, a, 0.0)
    return dict(origin=z(o), direction=z(d), g=z(g), s=z(s), wi_z=wi[..., 2], wo_z=wo[..., 2], alive=alive, usable=usable)


def points(rng, n=37, stride=3):
    """(records (n, stride), pos, nrm, view, spec): n glossy points with rho from 0.03 to 1, normals of every length and direction, views from
    head-on to grazing and from behind the stored normal, and the five kinds of unusable point at the indices UNUSABLE; pos, nrm and
    view are column ranges of `records` / of a view array with the same stride"""
    rec = rng.uniform(-1.0, 1.0, size=(n, max(stride, 6))).astype(F32)
    if stride < 6:
        pos, nrm = np.ascontiguousarray(rec[:, 0:3]), np.ascontiguousarray(rec[:, 3:6])
    else:
        rec = rng.uniform(-1.0, 1.0, size=(n, stride)).astype(F32)
        pos, nrm = rec[:, 8:11], rec[:, 4:7]                                                 # where AOV and surface records hold them
    pos *= F32(50.0)
    nrm *= rng.uniform(0.2, 3.0, size=(n, 1)).astype(F32)
    unit = nrm.astype(np.float64) / np.sqrt(np.sum(nrm.astype(np.float64) ** 2, -1))[:, None]
    # views: -(cos t n + sin t tangent) with t from 0 to just short of, and just past, 90 degrees
    tang = np.cross(unit, rng.normal(size=(n, 3)))
    tang /= np.sqrt(np.sum(tang ** 2, -1))[:, None]
    theta = np.concatenate([np.linspace(0.0, 1.45, n - 10), [1.5, 1.55, 1.565, 1.5705, 1.5707, 1.58, 1.7, 2.4, 3.0, 0.7]])
    vrec = np.zeros((n, stride), F32)
    vrec[:, 0:3] = (-(np.cos(theta)[:, None] * unit + np.sin(theta)[:, None] * tang) * rng.uniform(0.1, 4.0, size=(n, 1))).astype(F32)
    view = vrec[:, 0:3]
    spec = np.zeros((n, 4), F32)
    spec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
    spec[:, 3] = np.concatenate([[0.03, 1.0, 0.03, 1.0], np.exp(rng.uniform(np.log(0.03), 0.0, size=n - 4))]).astype(F32)
    spec[3, 3], view[3] = 1.0, (-unit[3] * 2.0).astype(F32)                                   # rho = 1 seen head-on
    for i, what in zip(UNUSABLE, ("nan position", "zero normal", "zero view", "rho 0", "rho nan")):
        if what == "nan position":
            pos[i, 1] = np.nan
        elif what == "zero normal":
            nrm[i] = 0.0
        elif what == "zero view":
            view[i] = 0.0
        elif what == "rho 0":
            spec[i, 3] = 0.0
        else:
            spec[i, 3] = np.nan
    return rec, pos, nrm, view, spec


UNUSABLE = (5, 11, 17, 23, 29)


def ray_cases():
    """the (D, stride, with ids, round, jitter) of the ray tests, CPU and GPU"""
    out = []
    for D in DIRECTIONS:
        for k, stride in enumerate(STRIDES):
            out.append((D, stride, (k + D) % 2 == 1, (k + D // 5) % 2, True))
    out.append((5, 3, False, 1, False))
    return out


def case_inputs(D, stride, with_ids, jitter=True):
    rng = np.random.default_rng(1000 * D + stride)
    rec, pos, nrm, view, spec = points(rng, 37, stride)
    ids = rng.permutation(37)[:31].astype(np.uint32) if with_ids else None
    reflect = api.ReflectionGather(D).bias(0.01).seed(SEED).jitter(jitter)
    return reflect, pos, nrm, view, spec, ids


def ulp32(x):
    """one float32 unit in the last place at |x|, as float64 (the spacing of the float32 grid there)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def vector_ulp(v):
    """(..., 1): one float32 ulp at the scale of each 3-vector's largest component (DESIGN.md §9k's bound)"""
    return ulp32(np.max(np.abs(np.asarray(v, np.float64)), axis=-1, keepdims=True))


# ---- fw_reflect_reduce --------------------------------------------------------------------------------------------------------------
def reduce_loop(surface, irradiance, weights, D, direct=None):
    """fw_reflect_reduce's statement as a plain loop over Python floats (IEEE float64): (n, 8) = (P.rgb, alive, Q.rgb, sky), before the
    one rounding to float32"""
    s = np.asarray(surface, F32).reshape(-1, D, 16)
    E = np.asarray(irradiance, F32).reshape(-1, D, 3)
    W = np.asarray(weights, F32).reshape(-1, D, 2)
    Ed = None if direct is None else np.asarray(direct, F32).reshape(-1, D, 8)
    Gp = 1
    while Gp < min(D, 64):
        Gp *= 2
    inv_pi = 1.0 / 3.141592653589793
    out = np.zeros((s.shape[0], 8))
    for q in range(s.shape[0]):
        part = [[0.0] * 8 for _ in range(Gp)]
        for l in range(Gp):
            for j in range(l, D, Gp):
                kind, g, sw = float(s[q, j, 3]), float(W[q, j, 0]), float(W[q, j, 1])
                if g > 0.0:
                    part[l][3] = part[l][3] + 1.0
                if kind == -2.0:
                    continue
                if kind == -1.0 or kind == 3.0:
                    L = [float(s[q, j, 12 + c]) for c in range(3)]
                    if kind == -1.0:
                        part[l][7] = part[l][7] + 1.0
                else:
                    L = []
                    for c in range(3):
                        e = float(E[q, j, c])
                        t = e if e > 0.0 else 0.0
                        if Ed is not None:
                            t = t + float(Ed[q, j, c])
                        L.append((float(s[q, j, c]) * t) * inv_pi)
                wa, wb = g * (1.0 - sw), g * sw
                for c in range(3):
                    part[l][c] = part[l][c] + wa * L[c]
                    part[l][4 + c] = part[l][4 + c] + wb * L[c]
        m = Gp // 2
        while m >= 1:
            part = [[part[l][c] + part[l ^ m][c] for c in range(8)] for l in range(Gp)]
            m //= 2
        out[q] = [(1.0 / D) * part[0][c] for c in range(8)]
    return out


def synthetic_weights(n, D, rng, surface):
    """(n D, 2) float32 weights (g, s) in [0, 1] with a fifth of them dead (0, 0), and `surface` with kind -2 at the dead rays, as
    fw_hit_surface leaves them"""
    w = rng.uniform(0.0, 1.0, size=(n * D, 2)).astype(F32)
    dead = rng.uniform(size=n * D) < 0.2
    w[dead] = 0.0
    surface = surface.copy()
    surface[dead, 3] = -2.0
    return w, surface


def estimate(mu, rho, f0, D, R, seed=SEED):
    """(f0 P + Q) / R from api.reflect_rays' weights with L = 1 on every alive ray, over R rounds of D rays at one point seen at cosine mu"""
    reflect = api.ReflectionGather(D).seed(seed)
    view = -np.array([np.sqrt(max(1.0 - mu * mu, 0.0)), 0.0, mu])
    spec = np.array([[f0, f0, f0, rho]], F32)
    surface = np.zeros((D, 16), F32)
    surface[:, 3], surface[:, 12:15] = -1.0, 1.0
    sums = np.zeros((1, 8), F32)
    for r in range(R):
        _rays, w = api.reflect_rays(reflect, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [view], spec, round=r)
        s = surface.copy()
        s[w[:, 0] == 0, 3] = -2.0
        sums = add_to(sums, api.reflect_reduce(s, np.zeros((D, 3), F32), w, D))
    return float(api.reflect_resolve(sums, spec, R)[0, 0])
