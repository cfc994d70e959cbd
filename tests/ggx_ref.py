"""GgxMat (FW_MAT_GGX) restated in float64 from the specification in include/firework_hip.h: the frame, the visible-normal
sampler, the attenuation of a sampled direction, f cos and the density p_b of a given one, and the directional albedo E(mu, alpha) by
quadrature.  Vectorised: every argument may carry leading axes (..., 3); scalars broadcast."""
import numpy as np


def _a(x):
    return np.asarray(x, np.float64)


def _dot(a, b):
    return np.sum(a * b, -1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def alpha_of(roughness):
    """alpha = roughness^2 as the host computes it: in float32"""
    r = np.asarray(roughness, np.float32)
    return (r * r).astype(np.float64)


def basis(n):
    """Duff et al. 2017: the tangent vectors t, b around the unit vector n (right-handed: t x b = n)"""
    n = _a(n)
    s = np.copysign(1.0, n[..., 2])
    a = -1.0 / (s + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    t = np.stack([1.0 + s * n[..., 0] ** 2 * a, s * b, -s * n[..., 0]], -1)
    u = np.stack([b, s + n[..., 1] ** 2 * a, -n[..., 1]], -1)
    return t, u


def frame(normal, ray_d):
    """(t, b, n, wo_local) at a hit with the reported normal, reached along ray_d (any length): wo = -normalized(ray_d), n flipped towards it"""
    normal, ray_d = np.broadcast_arrays(_a(normal), _a(ray_d))
    wo = -_unit(ray_d)
    n = np.where((_dot(wo, normal) < 0.0)[..., None], -normal, normal)
    t, b = basis(n)
    return t, b, n, np.stack([_dot(wo, t), _dot(wo, b), _dot(wo, n)], -1)


def to_local(fr, w):
    t, b, n, _ = fr
    w = _a(w)
    return np.stack([_dot(w, t), _dot(w, b), _dot(w, n)], -1)


def to_world(fr, w):
    t, b, n, _ = fr
    return w[..., 0:1] * t + w[..., 1:2] * b + w[..., 2:3] * n


def schlick(f0, c):
    f0 = _a(f0)
    return f0 + (1.0 - f0) * ((1.0 - _a(c)) ** 5)[..., None]


def lam(w, alpha):
    """Smith's Lambda of a local direction (z > 0)"""
    t2 = (w[..., 0] ** 2 + w[..., 1] ** 2) / w[..., 2] ** 2
    return 0.5 * (np.sqrt(1.0 + alpha ** 2 * t2) - 1.0)


def d_ggx(h, alpha):
    """D of a unit local half vector, from its tangential and normal parts"""
    return alpha ** 2 / (np.pi * (h[..., 0] ** 2 + h[..., 1] ** 2 + alpha ** 2 * h[..., 2] ** 2) ** 2)


def sample_local(wo, alpha, xi1, xi2):
    """Heitz 2018: (wi, h) local for the uniform pair (xi1, xi2); wi may point below the surface"""
    wo, alpha, xi1, xi2 = _a(wo), _a(alpha), _a(xi1), _a(xi2)
    vh = _unit(np.stack([alpha * wo[..., 0], alpha * wo[..., 1], wo[..., 2] + 0.0 * alpha], -1))
    l2 = vh[..., 0] ** 2 + vh[..., 1] ** 2
    il = 1.0 / np.sqrt(np.where(l2 > 0, l2, 1.0))
    t1 = np.where((l2 > 0)[..., None], np.stack([-vh[..., 1] * il, vh[..., 0] * il, 0.0 * il], -1), np.array([1.0, 0.0, 0.0]))
    t2 = np.cross(vh, t1)
    r, phi = np.sqrt(xi1), 2.0 * np.pi * xi2
    p1, s = r * np.cos(phi), 0.5 * (1.0 + vh[..., 2])
    p2 = (1.0 - s) * np.sqrt(np.maximum(1.0 - p1 * p1, 0.0)) + s * (r * np.sin(phi))
    nh = p1[..., None] * t1 + p2[..., None] * t2 + np.sqrt(np.maximum(1.0 - p1 * p1 - p2 * p2, 0.0))[..., None] * vh
    h = _unit(np.stack([alpha * nh[..., 0], alpha * nh[..., 1], np.maximum(nh[..., 2], 0.0)], -1))
    wi = 2.0 * _dot(wo, h)[..., None] * h - wo
    return wi, h


def sample(normal, ray_d, roughness, f0, xi1, xi2):
    """-> (wi world, attenuation rgb, alive, wi.n): the scattered direction of the pair (xi1, xi2); attenuation = F G2 / G1(wo), 0 where the
    path ends (wi.n <= 0)"""
    alpha = alpha_of(roughness)
    fr = frame(normal, ray_d)
    wo = fr[3]
    wi, h = sample_local(wo, alpha, xi1, xi2)
    alive = (wi[..., 2] > 0.0) & (wo[..., 2] > 0.0)
    safe = np.where(alive[..., None], wi, np.array([0.0, 0.0, 1.0]))
    lo, li = lam(wo, alpha), lam(safe, alpha)
    att = schlick(f0, _dot(wo, h)) * ((1.0 + lo) / (1.0 + lo + li))[..., None]
    return to_world(fr, wi), np.where(alive[..., None], att, 0.0), alive, wi[..., 2]


def eval_local(wo, wi, alpha, f0):
    """-> (f cos(theta_i) rgb, p_b) of the local unit directions; 0 where either lies in or below the surface"""
    wo, wi = np.broadcast_arrays(_a(wo), _a(wi))
    ok = (wi[..., 2] > 0.0) & (wo[..., 2] > 0.0)
    up = np.array([0.0, 0.0, 1.0])
    so, si = np.where(ok[..., None], wo, up), np.where(ok[..., None], wi, up)
    h = _unit(so + si)
    lo, li = lam(so, alpha), lam(si, alpha)
    d4 = d_ggx(h, alpha) / (4.0 * so[..., 2])
    fcos = schlick(f0, _dot(so, h)) * (d4 / (1.0 + lo + li))[..., None]
    return np.where(ok[..., None], fcos, 0.0), np.where(ok, d4 / (1.0 + lo), 0.0)


def evaluate(normal, ray_d, roughness, f0, omega):
    """-> (f cos rgb, p_b) towards the world direction omega (normalised here)"""
    fr = frame(normal, ray_d)
    return eval_local(fr[3], to_local(fr, _unit(_a(omega))), alpha_of(roughness), f0)


def wo_of(mu):
    """a local wo of cosine mu, in the xz plane"""
    return np.array([np.sqrt(max(1.0 - mu * mu, 0.0)), 0.0, mu])


def half_vector_grid(alpha, n_theta=512, n_phi=1024):
    """Midpoints of an n_theta x n_phi grid in (theta_h, phi_h) over the half vector's hemisphere: uniform in phi_h, and theta_h =
    atan(alpha tan(pi t / 2)) at uniform t, which spreads the nodes over a lobe of any width (uniform in theta_h at alpha = 1).
    -> (h (n_theta, n_phi, 3), solid-angle weights (n_theta, n_phi))"""
    t = 0.5 * np.pi * (np.arange(n_theta) + 0.5) / n_theta
    th = np.arctan(alpha * np.tan(t))
    dth = alpha / (np.cos(t) ** 2 + (alpha * np.sin(t)) ** 2) * (0.5 * np.pi / n_theta)
    ph = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    h = np.stack([st * np.cos(ph)[None, :], st * np.sin(ph)[None, :], ct + 0.0 * ph[None, :]], -1)
    return h, (st * dth[:, None]) * (2.0 * np.pi / n_phi) * np.ones((1, n_phi))


def pdf_mass(mu, roughness, n_theta=512, n_phi=1024):
    """The integral of p_b over ALL wi, the mass below the horizon included: in the half vector's measure dwi = 4 (wo.h) dwh the density of
    h is the visible-normal distribution G1(wo) max(wo.h, 0) D(h) / wo.n, which integrates to 1."""
    alpha = alpha_of(roughness)
    wo = wo_of(mu)
    h, w = half_vector_grid(alpha, n_theta, n_phi)
    g1 = 1.0 / (1.0 + lam(wo, alpha))
    return float(np.sum(g1 * np.maximum(_dot(h, wo), 0.0) * d_ggx(h, alpha) / wo[2] * w))


def albedo(mu, roughness, f0=1.0, n_theta=512, n_phi=1024):
    """E(mu, alpha) = the integral of f cos over the upper hemisphere of wi (one channel of F0), over the same grid in h:
    f cos dwi = F D G2 / (4 wo.n) x 4 (wo.h) dwh wherever wi = reflect(-wo, h) lies above the surface"""
    alpha = alpha_of(roughness)
    wo = wo_of(mu)
    h, w = half_vector_grid(alpha, n_theta, n_phi)
    oh = _dot(h, wo)
    wi = 2.0 * oh[..., None] * h - wo
    ok = (wi[..., 2] > 0.0) & (oh > 0.0)
    si = np.where(ok[..., None], wi, np.array([0.0, 0.0, 1.0]))
    g2 = 1.0 / (1.0 + lam(wo, alpha) + lam(si, alpha))
    f = f0 + (1.0 - f0) * (1.0 - oh) ** 5
    return float(np.sum(np.where(ok, f * d_ggx(h, alpha) * g2 * oh / wo[2], 0.0) * w))


def expected_attenuation(mu, roughness, f0=1.0, m=256, seed=1):
    """The mean of the sampled attenuation (0 for a path that ends) over m x m stratified (xi1, xi2), one uniform point in every cell: an
    unbiased estimate of the expectation whose variance is at most that of m^2 independent samples"""
    rng = np.random.default_rng(seed)
    g = np.arange(m) / m
    xi1, xi2 = np.meshgrid(g, g, indexing="ij")
    xi1, xi2 = xi1 + rng.random((m, m)) / m, xi2 + rng.random((m, m)) / m
    alpha = alpha_of(roughness)
    wo = wo_of(mu)
    wi, h = sample_local(wo, alpha, xi1, xi2)
    alive = wi[..., 2] > 0.0
    si = np.where(alive[..., None], wi, np.array([0.0, 0.0, 1.0]))
    lo, li = lam(wo, alpha), lam(si, alpha)
    f = f0 + (1.0 - f0) * (1.0 - _dot(h, wo)) ** 5
    return float(np.mean(np.where(alive, f * (1.0 + lo) / (1.0 + lo + li), 0.0)))
