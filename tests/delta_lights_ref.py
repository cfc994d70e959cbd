"""Float64 restatement of the three delta-light contributions, for the tests.

At a Lambertian or Isotropic vertex x with BSDF-sampling normal n_b (the reported unit normal; 0 for Isotropic), one light picked with
probability p adds  beta * albedo * p_b(w) * L / p  where it is visible:
    point        w = normalized(pos - x),  L = I / d^2
    spot         as point, L = I s / d^2: c = -w . axis, t = clamp((c - cos_outer) / (cos_inner - cos_outer), 0, 1), s = t^2 (3 - 2t);
                 cos_inner == cos_outer: s = 1 where c >= cos_outer, else 0
    directional  w = -dir,  L = E
p_b is §9g's density of the direction of n_b + u, u uniform in the unit ball: 2 cos^3 / pi for |n_b| = 1, 1 / 4 pi for n_b = 0.
The lights are the api's objects; their fields are taken as the library receives them (float32 record fields, the direction normalised in
double and rounded to float32)."""
import numpy as np

from firework_amd import _abi as A


def scatter_pdf(n_b, w):
    n_b, w = np.asarray(n_b, np.float64), np.asarray(w, np.float64)
    c = float(n_b @ w)
    disc = c * c - float(n_b @ n_b) + 1.0
    if not disc >= 0.0:
        return 0.0
    s = np.sqrt(disc)
    tp, tm = c + s, max(c - s, 0.0)
    if not tp > 0.0:
        return 0.0
    return (tp ** 3 - tm ** 3) / (4.0 * np.pi)


def _record(light):
    l = light.to_abi()
    v = lambda a: np.array([a.x, a.y, a.z], np.float64)
    d = v(l.direction)
    n = np.linalg.norm(d)
    if n > 0:
        d = (d / n).astype(np.float32).astype(np.float64)
    return l.kind, v(l.position), d, v(l.intensity), float(l.cos_inner), float(l.cos_outer)


def incident(light, x):
    """(w, L, d): the unit direction towards the light from x, L (rgb) of the table above, and the distance to the light (inf for a
    directional one)"""
    kind, pos, axis, inten, ci, co = _record(light)
    x = np.asarray(x, np.float64)
    if kind == A.FW_LIGHT_DIRECTIONAL:
        return -axis, inten, np.inf
    v = pos - x
    d2 = float(v @ v)
    if not d2 > 0.0:
        return np.zeros(3), np.zeros(3), 0.0
    d = np.sqrt(d2)
    w = v / d
    s = 1.0
    if kind == A.FW_LIGHT_SPOT:
        c = float(-(w @ axis))
        if ci > co:
            t = min(max((c - co) / (ci - co), 0.0), 1.0)
            s = t * t * (3.0 - 2.0 * t)
        else:
            s = 1.0 if c >= co else 0.0
    return w, inten * (s / d2), d


def spot_cosine(light, x):
    """c = -w . axis of a spot light seen from x"""
    _, pos, axis, _, _, _ = _record(light)
    v = pos - np.asarray(x, np.float64)
    return float(-(v / np.linalg.norm(v)) @ axis)


def contribution(light, x, n_b, albedo, beta=1.0, p=1.0):
    """rgb a visible sample of `light` adds at x"""
    w, L, _ = incident(light, x)
    return np.asarray(beta, np.float64) * np.asarray(albedo, np.float64) * scatter_pdf(n_b, w) * L / p


# ---- the far-field room of tests/test_gpu_delta_lights.py (check 6) -------------------------------------------------------------------
# A closed Lambertian room [-3, 3] x [0, 6] x [-3, 3] lit by an emissive sphere of radius ROOM_R at ROOM_LIGHT, or by a point light of
# intensity Le pi r^2 there.  Every surface is at least 2 away from the sphere.
ROOM_HALF, ROOM_HEIGHT = 3.0, 6.0
ROOM_LIGHT = (0.6, 3.4, -0.2)
ROOM_R = 0.02
ROOM_LE = 8000.0


def sphere_direct(centre, r, le, x, n, m=400):
    """The direct term at a Lambertian point x (unit normal n) under an emissive sphere: le * int over the cone it subtends of
    2 cos^3(theta) / pi dw, by midpoint quadrature (m x m)"""
    c = np.asarray(centre, np.float64) - np.asarray(x, np.float64)
    n = np.asarray(n, np.float64)
    d = np.linalg.norm(c)
    w = c / d
    omc = 1.0 - np.sqrt(1.0 - (r / d) ** 2)
    ct = 1.0 - (np.arange(m) + 0.5) / m * omc
    ph = (np.arange(m) + 0.5) / m * 2 * np.pi
    CT, PH = np.meshgrid(ct, ph, indexing="ij")
    ST = np.sqrt(1.0 - CT ** 2)
    a = np.array([1.0, 0, 0]) if abs(w[0]) < 0.9 else np.array([0, 1.0, 0])
    e1 = np.cross(w, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(w, e1)
    cn = ST * np.cos(PH) * (e1 @ n) + ST * np.sin(PH) * (e2 @ n) + CT * (w @ n)
    return le * float((2 * np.clip(cn, 0, None) ** 3 / np.pi).mean() * 2 * np.pi * omc)
