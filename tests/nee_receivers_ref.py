"""Float64 restatement of light sampling at receivers whose reported normal n is not the unit +y of a floor,
and the probe tables tests/test_gpu_nee_receivers.py renders.  Plain numpy, independent of the kernels.

A Lambertian vertex scatters along n + u, u uniform in the unit ball, n the *reported* normal: unnormalised (p0 - p2) x (p1 - p2) for a mesh
without vertex normals, never turned towards the ray, negated by flip_normals; an Isotropic vertex has n = 0.  The density of the unit
direction w is p_b(w; n) = (t+^3 - max(t-, 0)^3) / 4 pi, t+- = c +- sqrt(c^2 - |n|^2 + 1), c = n . w (scatter_density).

A light seen from a point P is a *quadrature set*: directions w_k, solid angles dw_k, the light sampler's density p_l(w_k) (pick probability
included) and the radiance L_k.  From one set (or several, of disjoint directions) come
    want           = f sum L p_b dw,                       f = beta x albedo per channel
    default        second moment f^2 sum L^2 p_b dw        (a bounce reaches the light or it does not: Bernoulli for one radiance)
    MIS            the light-sample part  X = f L p_b p_l / (p_l^2 + p_b^2) drawn with density p_l,
                   the BSDF part          Y = f L p_b^2  / (p_l^2 + p_b^2) drawn with density p_b,
                   independent draws: variance = E X^2 - (E X)^2 + E Y^2 - (E Y)^2, and E X + E Y = want.
Delta lights are deterministic: want = f p_b(w) L / p (delta_lights_ref.contribution), with a condition number kappa of p_b by finite
difference.  The single-scattering answer of an Isotropic medium is a one-dimensional quadrature along the probe's chord (medium_answer).

Every table is built here, from the geometry alone, before anything is rendered; tests/test_nee_receivers_cpu.py asserts its composition."""
import functools
import os
import sys

import numpy as np

from firework_amd import _abi as A
from firework_amd import _lib
from firework_amd.api import (CheckerTexture, ColorEnv, ConstantTexture, DirectionalLight, EmissiveMat, GgxMat, HdrEnvironment, LambertianMat,
                              MetalMat, PointLight, Rect3d, RenderObject, Rotor3, Scene, SpotLight, Sphere, TriangleMesh, XZRect, YZRect)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_lights_ref as DR  # noqa: E402
import emitters_ref as ER  # noqa: E402
import env_dist_ref as VR  # noqa: E402

F4, F8 = A.FW_FLAG_LIGHT_SAMPLING, A.FW_FLAG_ENV_SAMPLING
F16 = A.FW_FLAG_ALL_EMITTERS
N_MAX = 1 << 18
N_MIN = 1 << 12
EPS23 = 2.0 ** -23


# ---- the density -----------------------------------------------------------------------------------------------------------------------
def density_cn(c, nn):
    """p_b from c = n . w and nn = |n|^2 (arrays)"""
    c, nn = np.asarray(c, np.float64), np.asarray(nn, np.float64)
    disc = c * c - nn + 1.0
    ok = disc >= 0.0
    s = np.sqrt(np.where(ok, disc, 0.0))
    tp, tm = c + s, np.maximum(c - s, 0.0)
    # (a normal of length >= 1 puts the vertex outside or on the ball around its tip: no direction with c <= 0 meets it.  Stated apart, as
    #  t+ = c + sqrt(c^2) there is 0 only in exact arithmetic; a unit normal computed in float64 counts as one of length 1)
    return np.where(ok & (tp > 0.0) & ~((nn >= 1.0 - 1e-12) & (c <= 0.0)), (tp ** 3 - tm ** 3) / (4.0 * np.pi), 0.0)


def scatter_density(n, w):
    """p_b(w; n): n (3,) or (..., 3), any length, 0 included; w (..., 3) unit"""
    n, w = np.asarray(n, np.float64), np.asarray(w, np.float64)
    return density_cn((n * w).sum(-1), (n * n).sum(-1))


def kappa(n, w):
    """condition number of p_b at (n, w): the largest relative change of p_b when c and |n|^2 move by one part in 2^23 each, either way,
    over that relative step; at least 1"""
    n, w = np.asarray(n, np.float64), np.asarray(w, np.float64)
    c, nn = float(n @ w), float(n @ n)
    p = float(density_cn(c, nn))
    if not p > 0:
        return np.inf
    worst = 0.0
    for sc in (1.0, -1.0):
        for sn in (1.0, -1.0):
            q = float(density_cn(c * (1 + sc * EPS23), nn * (1 + sn * EPS23)))
            worst = max(worst, abs(q - p) / p)
    return max(1.0, worst / EPS23)


# ---- quadrature sets ---------------------------------------------------------------------------------------------------------------------
class QSet:
    def __init__(self, w, dw, pl, L):
        self.w, self.dw, self.pl = np.asarray(w, np.float64), np.asarray(dw, np.float64), np.asarray(pl, np.float64)
        self.L = np.broadcast_to(np.asarray(L, np.float64), (self.w.shape[0], 3))

    @staticmethod
    def join(sets):
        return QSet(np.concatenate([s.w for s in sets]), np.concatenate([s.dw for s in sets]), np.concatenate([s.pl for s in sets]),
                    np.concatenate([s.L for s in sets]))


def _grid(m):
    s = (np.arange(m) + 0.5) / m
    S, T = np.meshgrid(s, s, indexing="ij")
    return S.ravel(), T.ravel()


def flat_set(points, normal, dA, P, L, area_of_pick, p_pick=1.0):
    """a flat emitter sampled uniformly in area: p_omega = d^2 / (|cos_l| A); area_of_pick: the area the pick probability p_pick stands
    for (entries of one radiance picked by area: p_pick A_i / sum A = 1 / sum A, so pass the sum and p_pick = 1)"""
    X = np.asarray(points, np.float64) - np.asarray(P, np.float64)
    d2 = (X ** 2).sum(-1)
    d = np.sqrt(d2)
    cos_l = np.abs(X @ np.asarray(normal, np.float64)) / d
    return QSet(X / d[:, None], cos_l * dA / d2, p_pick * d2 / (cos_l * area_of_pick), L)


def rect_set(light, P, L, m=160, scale=1.0):
    """a rectangle as fw_selftest_lights reports it (world corners, p_pick); scale: what the other sampled lights leave of the pick"""
    c0, c1, c3 = light["corners"][0], light["corners"][1], light["corners"][3]
    e1, e2 = c1 - c0, c3 - c0
    nl = np.cross(e1, e2)
    area = np.linalg.norm(nl)
    S, T = _grid(m)
    pts = c0 + S[:, None] * e1 + T[:, None] * e2
    return flat_set(pts, nl / area, area / S.size, P, L, area, scale * light["p_pick"])


def sphere_set(light, P, L, m=160, scale=1.0):
    """a sphere as fw_selftest_lights reports it: uniform in the cone it subtends"""
    c = light["centre"] - np.asarray(P, np.float64)
    d = np.linalg.norm(c)
    w0 = c / d
    omc = 1.0 - np.sqrt(1.0 - (light["radius"] / d) ** 2)
    S, T = _grid(m)
    ct, ph = 1.0 - S * omc, 2 * np.pi * T
    st = np.sqrt(1.0 - ct ** 2)
    a = np.array([1.0, 0, 0]) if abs(w0[0]) < 0.9 else np.array([0, 1.0, 0])
    e1 = np.cross(w0, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(w0, e1)
    w = (st * np.cos(ph))[:, None] * e1 + (st * np.sin(ph))[:, None] * e2 + ct[:, None] * w0
    omega = 2 * np.pi * omc
    return QSet(w, np.full(S.size, omega / S.size), np.full(S.size, scale * light["p_pick"] / omega), L)


def triangle_points(v0, v1, v2, k=96):
    """centroids of the k^2 congruent sub-triangles, and the area each stands for"""
    v0, v1, v2 = (np.asarray(v, np.float64) for v in (v0, v1, v2))
    I, J = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    up, dn = (I + J) <= k - 1, (I + J) <= k - 2
    b1 = np.concatenate([(I[up] + 1 / 3) / k, (I[dn] + 2 / 3) / k])
    b2 = np.concatenate([(J[up] + 1 / 3) / k, (J[dn] + 2 / 3) / k])
    pts = v0 + b1[:, None] * (v1 - v0) + b2[:, None] * (v2 - v0)
    area = 0.5 * np.linalg.norm(np.cross(v1 - v0, v2 - v0))
    return pts, area / (k * k), area


def mesh_set(verts, tris, P, L, k=96):
    """a flat mesh of one radiance under FW_FLAG_ALL_EMITTERS: one entry per triangle, picked by area"""
    verts = np.asarray(verts, np.float64)
    total = sum(triangle_points(*verts[list(t)], k=1)[2] for t in tris)
    sets = []
    for t in tris:
        pts, dA, _ = triangle_points(*verts[list(t)], k=k)
        nl = np.cross(verts[t[1]] - verts[t[0]], verts[t[2]] - verts[t[0]])
        sets.append(flat_set(pts, nl / np.linalg.norm(nl), dA, P, L, total))
    return QSet.join(sets)


def disk_set(centre, rot, radius, inner, phi_max, P, L, m=160):
    """a Disk entry: the sector phi in [0, phi_max], r in [inner, radius] of the object's y = 0 plane, rotated by rot and moved to centre"""
    S, T = _grid(m)
    r, ph = inner + S * (radius - inner), T * phi_max
    local = np.stack([r * np.cos(ph), np.zeros_like(r), r * np.sin(ph)], -1)
    area = 0.5 * phi_max * (radius ** 2 - inner ** 2)
    dA = r * (radius - inner) * phi_max / S.size
    rot = np.asarray(rot, np.float64)
    return flat_set(local @ rot.T + np.asarray(centre, np.float64), rot @ np.array([0, 1.0, 0]), dA, P, L, area)


def box_set(lo, size, P, L, m=120):
    """a Rect3d's entries: six faces picked by area; a face whose outer side faces P is seen whole (the box is convex), the others are hidden
    by it, so their share of the picks carries nothing"""
    lo, size, P = (np.asarray(v, np.float64) for v in (lo, size, P))
    total = 2 * (size[0] * size[1] + size[0] * size[2] + size[1] * size[2])
    S, T = _grid(m)
    sets = []
    for ax in range(3):
        a1, a2 = [k for k in range(3) if k != ax]
        for side in (0, 1):
            nrm = np.zeros(3)
            nrm[ax] = 1.0 if side else -1.0
            pts = np.zeros((S.size, 3))
            pts[:, ax] = lo[ax] + side * size[ax]
            pts[:, a1] = lo[a1] + S * size[a1]
            pts[:, a2] = lo[a2] + T * size[a2]
            if nrm @ (P - pts[0]) > 0:
                sets.append(flat_set(pts, nrm, size[a1] * size[a2] / S.size, P, L, total))
    return QSet.join(sets)


def texel_dirs(x, y, w, h, m=64):
    """directions uniform in (phi, sin theta) inside texel (x, y) of a (h, w) map, as env_dist_ref lays it out: phi = pi (1 - 2 u),
    dir = (cos theta cos phi, sin theta, cos theta sin phi)"""
    hi, lo = VR.row_bounds(h)
    S, T = _grid(m)
    s = lo[y] + T * (hi[y] - lo[y])
    c = np.sqrt(np.maximum(1 - s * s, 0))
    phi = np.pi * (1 - 2 * (x + S) / w)
    return np.stack([c * np.cos(phi), s, c * np.sin(phi)], -1)


def map_set(rgb, p_env=1.0, m=64):
    """the texels of positive weight of an HDR map: numeric quadrature per texel, p_l = p_env x the table's density"""
    rgb = np.asarray(rgb, np.float64)
    h, w = rgb.shape[:2]
    _, dens, _ = VR.table(rgb)
    om = VR.omega_row(w, h)
    sets = []
    for y, x in zip(*np.nonzero(VR.texel_weights(rgb) > 0)):
        d = texel_dirs(x, y, w, h, m)
        sets.append(QSet(d, np.full(d.shape[0], om[y] / d.shape[0]), np.full(d.shape[0], p_env * dens[y, x]), rgb[y, x]))
    return QSet.join(sets)


def moments(q, n, f):
    """-> dict: want (3,), var_default (3,), var_nee (3,), parts (E X, E Y)"""
    f = np.asarray(f, np.float64)
    pb = scatter_density(n, q.w)
    fl = f[None, :] * q.L
    want = (fl * (pb * q.dw)[:, None]).sum(0)
    m2d = (fl ** 2 * (pb * q.dw)[:, None]).sum(0)
    den = q.pl ** 2 + pb ** 2
    X = fl * (pb * q.pl / den)[:, None]
    Y = fl * (pb ** 2 / den)[:, None]
    ex, ex2 = (X * (q.pl * q.dw)[:, None]).sum(0), (X ** 2 * (q.pl * q.dw)[:, None]).sum(0)
    ey, ey2 = (Y * (pb * q.dw)[:, None]).sum(0), (Y ** 2 * (pb * q.dw)[:, None]).sum(0)
    return dict(want=want, var_default=m2d - want ** 2, var_nee=(ex2 - ex ** 2) + (ey2 - ey ** 2), parts=(ex, ey),
                zero_safe=bool(np.all(outside(n, q.w))))


def outside(n, w, margin=1e-3):
    """directions that lie outside the support of p_b by a margin float32 cannot bridge: beyond the cone sin(theta) > 1 / |n| of a normal
    longer than 1 (disc <= -margin |n|^2), or behind a normal of length >= 1 (c <= -margin |n|)"""
    n, w = np.asarray(n, np.float64), np.asarray(w, np.float64)
    c, nn = w @ n, float(n @ n)
    return (c * c - nn + 1.0 <= -margin * nn) | ((nn >= 1.0 - 1e-12) & (c <= -margin * np.sqrt(nn)))


def samples_for(want, var, rel=0.01, z=4.0):
    """the smallest power of two N with z sqrt(var / N) <= rel want in every channel with want > 0"""
    want, var = np.atleast_1d(want), np.atleast_1d(var)
    pos = want > 0
    if not pos.any():
        return N_MIN
    need = float(((z / rel) ** 2 * var[pos] / want[pos] ** 2).max())
    n = N_MIN
    while n < need:
        n *= 2
    return n


# ---- the isotropic medium --------------------------------------------------------------------------------------------------------------------
def medium_answer(ray, centre, radius, rho, albedo, light, m=20000):
    """Single scattering in a spherical ConstantMedium (density rho, Isotropic albedo) along a probe ray from outside, lit by a delta light
    outside: the free path s has density rho ln10 10^(-rho s) (the reference draws -log10(xi) / rho), the vertex adds albedo / 4 pi x L(x_s),
    and its shadow ray survives its own draw with probability 10^(-rho l), l the chord from x_s to the boundary towards the light.
    -> (mean (3,), per-sample variance (3,), the largest L / 4 pi met (3,))"""
    o, d = np.asarray(ray[:3], np.float64), np.asarray(ray[3:], np.float64)
    d = d / np.linalg.norm(d)
    oc = o - np.asarray(centre, np.float64)
    b = oc @ d
    disc = b * b - (oc @ oc - radius * radius)
    assert disc > 0 and -b - np.sqrt(disc) > 0
    t1, chord = -b - np.sqrt(disc), 2 * np.sqrt(disc)
    s = (np.arange(m) + 0.5) / m * chord
    x = o + (t1 + s)[:, None] * d
    kind, pos, axis, inten, _, _ = DR._record(light)
    if kind == A.FW_LIGHT_DIRECTIONAL:
        w = np.broadcast_to(-axis, x.shape)
        L = np.broadcast_to(inten, x.shape)
    else:
        v = pos - x
        d2 = (v ** 2).sum(-1)
        w = v / np.sqrt(d2)[:, None]
        L = inten[None, :] / d2[:, None]
        assert kind == A.FW_LIGHT_POINT and np.sqrt(d2).min() > 0
    xc = x - np.asarray(centre, np.float64)
    xw = (xc * w).sum(-1)
    ell = -xw + np.sqrt(xw * xw - (xc * xc).sum(-1) + radius * radius)
    f = rho * np.log(10.0) * 10.0 ** (-rho * s) * (chord / m)
    c = albedo * L / (4 * np.pi)
    T = 10.0 ** (-rho * ell)
    mean = (f[:, None] * c * T[:, None]).sum(0)
    m2 = (f[:, None] * c ** 2 * T[:, None]).sum(0)
    return mean, m2 - mean ** 2, (L / (4 * np.pi)).max(0)


# ---- receivers --------------------------------------------------------------------------------------------------------------------------
ALB = (0.5, 0.5, 0.5)
LE = (4.0, 4.0, 4.0)
RAY_DIR = np.array([0.35, -1.0, 0.25])          # no zero component: the triangle test shears by the signed largest one
LIGHT_H = 1.5
TILT = np.array([0.15, 1.0, 0.1]) / np.linalg.norm([0.15, 1.0, 0.1])
MESH_ROTOR = Rotor3.from_rotation_xy(0.6)
RECT_ROTOR = Rotor3.from_rotation_yz(-0.5) * Rotor3.from_rotation_xy(0.4)
MESH_POS = (0.3, -0.2, 0.1)
METAL = (0.9, 0.6, 0.3)
MIRROR = dict(x=-1.5, y=(0.5, 0.9), z=(-0.4, 0.4))


class Probe:
    def __init__(self, ray, P, n, beta=(1.0, 1.0, 1.0)):
        self.ray, self.P, self.n, self.beta = np.asarray(ray, np.float32), np.asarray(P, np.float64), np.asarray(n, np.float64), np.asarray(beta, np.float64)


def _ray_to(target, direction, back=0.4):
    d = np.asarray(direction, np.float64)
    return np.concatenate([np.asarray(target, np.float64) - back * d, d]).astype(np.float32)


def _plane_hit(ray, p0, n):
    o, d = ray[:3].astype(np.float64), ray[3:].astype(np.float64)
    t = ((p0 - o) @ n) / (d @ n)
    assert t > 0
    return o + t * d


def mesh_vertices(nn):
    """a right triangle of legs a = 2 sqrt(nn) along e1 and b = sqrt(nn) / 2, in a tilted plane: (p0 - p2) x (p1 - p2) = nn TILT"""
    e1 = np.array([1.0, 0, 0]) - TILT[0] * TILT
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(e1, TILT)
    a, b = 2 * np.sqrt(nn), np.sqrt(nn) / 2
    return np.array([b * e2, a * e1, np.zeros(3)]).astype(np.float32), e1, e2, a, b


MESH_S = (0.04, 0.1, 0.17, 0.8, 0.88, 0.96)     # along the long leg; the light stands over s = 0.1
VERTEX_NORMALS = np.array([[0.35, 1.0, -0.1], [-0.2, 1.0, 0.3], [0.1, 1.0, 0.35]])


class Receiver:
    """name; add(scene): its objects; probes; light_at: where the local lights stand, up: the unit direction from the anchor to them"""

    def __init__(self, name):
        self.name = name
        self.nn = 1.0
        self.bvh = (True,)
        self.mirror = False


def mesh_receiver(nn, rotated=False, normals=False):
    r = Receiver(("mesh_rot_" if rotated else "mesh_vn_" if normals else "mesh_") + str(nn))
    r.nn = 1.0 if normals else nn
    r.bvh = (True,) if (rotated or normals) else (True, False)
    verts, e1, e2, a, b = mesh_vertices(nn)
    v64 = verts.astype(np.float64)
    R = ER.rotation(MESH_ROTOR) if rotated else np.eye(3)
    pos = np.asarray(MESH_POS if rotated else (0, 0, 0), np.float64)
    n_obj = np.cross(v64[0] - v64[2], v64[1] - v64[2])
    vn = None
    if normals:
        vn = (VERTEX_NORMALS / np.linalg.norm(VERTEX_NORMALS, axis=1)[:, None]).astype(np.float32)
    world = v64 @ R.T + pos

    def add(scene, mat):
        ro = RenderObject.new(TriangleMesh(verts, np.array([0, 1, 2], np.uint32), normals=vn, material=mat))
        if rotated:
            ro.rotate(MESH_ROTOR).position(*MESH_POS)
        scene.add_object(ro)
    r.add = add
    r.probes = []
    d = R @ RAY_DIR
    for s in MESH_S:
        tgt = world[2] + s * (world[1] - world[2]) + 0.25 * (1 - s) * (world[0] - world[2])
        ray = _ray_to(tgt, d)
        P = _plane_hit(ray, world[2], R @ n_obj)
        if normals:
            # barycentrics of P (affine coordinates along the two legs from p2), then the interpolated, normalised normal
            q = P - world[2]
            l0, l1 = world[0] - world[2], world[1] - world[2]
            (b0, b1), *_ = np.linalg.lstsq(np.stack([l0, l1], 1), q, rcond=None)
            ni = b0 * vn[0].astype(np.float64) + b1 * vn[1].astype(np.float64) + (1 - b0 - b1) * vn[2].astype(np.float64)
            n = R @ (ni / np.linalg.norm(ni))
        else:
            n = R @ n_obj
        r.probes.append(Probe(ray, P, n))
    r.obj_dir = RAY_DIR
    r.up = R @ n_obj / np.linalg.norm(n_obj)
    r.light_at = r.probes[1].P + LIGHT_H * r.up
    return r


def rect_receiver(kind):
    """kind: rotated (an XZRect under OF_ROTATED), below (hit from below: the normal stays +y), flipped (flip_normals, hit from above: -y)"""
    r = Receiver("rect_" + kind)
    R = ER.rotation(RECT_ROTOR) if kind == "rotated" else np.eye(3)
    sign = -1.0 if kind == "flipped" else 1.0

    def add(scene, mat):
        ro = RenderObject.new(XZRect.new(-3, 3, -3, 3, 0, mat))
        if kind == "rotated":
            ro.rotate(RECT_ROTOR)
        if kind == "flipped":
            ro.flip_normals()
        scene.add_object(ro)
    r.add = add
    up = R @ np.array([0, 1.0, 0])
    d = R @ (RAY_DIR * (np.array([1, -1, 1]) if kind == "below" else 1.0))
    r.probes = []
    for x, z in ((0.2, 0.1), (-0.5, 0.6), (0.9, -0.7), (1.6, 1.2), (2.7, 2.3)):      # (the last one sees the light 23 degrees above the plane)
        ray = _ray_to(R @ np.array([x, 0, z]), d)
        r.probes.append(Probe(ray, _plane_hit(ray, np.zeros(3), up), sign * up))
    r.up = up
    r.light_at = R @ np.array([0.2, 0, 0.1]) + LIGHT_H * up
    return r


def sphere_receiver():
    """a unit sphere probed at three latitudes (10, 30 and 50 degrees from its top), the rays aimed at its surface points"""
    r = Receiver("sphere")
    centre = np.array([0.0, -1.0, 0.0])
    r.add = lambda scene, mat: scene.add_object(RenderObject.new(Sphere.new(1.0, mat)).position(*centre))
    r.probes = []
    for lat, az in ((10.0, 0.7), (30.0, 2.4), (50.0, -1.9)):
        t = np.radians(lat)
        nrm = np.array([np.sin(t) * np.cos(az), np.cos(t), np.sin(t) * np.sin(az)])
        ray = _ray_to(centre + nrm, RAY_DIR)
        o, d = ray[:3].astype(np.float64), ray[3:].astype(np.float64)
        oc = o - centre
        aa, bb, cc = d @ d, 2 * (oc @ d), oc @ oc - 1.0
        tt = (-bb - np.sqrt(bb * bb - 4 * aa * cc)) / (2 * aa)
        P = o + tt * d
        r.probes.append(Probe(ray, P, P - centre))
    r.up = np.array([0, 1.0, 0])
    r.light_at = centre + (1.0 + LIGHT_H) * r.up
    return r


def metal_receiver():
    """a Lambertian floor seen in a mirror MetalMat (roughness 0): a YZRect at x = MIRROR.x whose reported normal +x faces the probes.  The
    mirror is small and low: no segment from a floor point to the light, or to the light's mirror image, crosses it (checked per table)"""
    r = Receiver("metal")
    r.mirror = True

    def add(scene, mat):
        scene.add_object(RenderObject.new(XZRect.new(-3, 3, -3, 3, 0, mat)))
        m = scene.add_material(MetalMat.new(METAL, 0.0))
        scene.add_object(RenderObject.new(YZRect.new(MIRROR["y"][0], MIRROR["y"][1], MIRROR["z"][0], MIRROR["z"][1], MIRROR["x"], m)))
    r.add = add
    r.probes = []
    for (px, pz), (my, mz) in (((-1.2, 0.1), (0.7, 0.0)), ((-1.05, -0.3), (0.62, -0.2)), ((-1.3, 0.35), (0.8, 0.25))):
        M, Pt = np.array([MIRROR["x"], my, mz]), np.array([px, 0.0, pz])
        out = Pt - M
        ray = _ray_to(M, out * np.array([-1.0, 1.0, 1.0]), back=0.8)
        o, d = ray[:3].astype(np.float64), ray[3:].astype(np.float64)
        hit = o + (MIRROR["x"] - o[0]) / d[0] * d
        assert MIRROR["y"][0] < hit[1] < MIRROR["y"][1] and MIRROR["z"][0] < hit[2] < MIRROR["z"][1]
        refl = d * np.array([-1.0, 1.0, 1.0])
        P = hit + (0.0 - hit[1]) / refl[1] * refl
        r.probes.append(Probe(ray, P, (0, 1.0, 0), METAL))
    r.up = np.array([0, 1.0, 0])
    r.light_at = np.array([0.5, 0.0, 0.1]) + LIGHT_H * r.up
    return r


def crosses_mirror(P, X):
    """does the segment from P to any point of X (n, 3) cross the mirror's rectangle?"""
    P, X = np.asarray(P, np.float64), np.asarray(X, np.float64)
    dx = X[:, 0] - P[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (MIRROR["x"] - P[0]) / dx
        y, z = P[1] + t * (X[:, 1] - P[1]), P[2] + t * (X[:, 2] - P[2])
    return bool(np.any((t > 0) & (t < 1) & (y > MIRROR["y"][0]) & (y < MIRROR["y"][1]) & (z > MIRROR["z"][0]) & (z < MIRROR["z"][1])))


MESH_SIZES = (0.05, 0.3, 1, 1.7, 4)


@functools.lru_cache(maxsize=None)
def receiver(name):
    if name.startswith("mesh_rot_"):
        return mesh_receiver(float(name[9:]), rotated=True)
    if name.startswith("mesh_vn_"):
        return mesh_receiver(float(name[8:]), normals=True)
    if name.startswith("mesh_"):
        return mesh_receiver(float(name[5:]))
    if name.startswith("rect_"):
        return rect_receiver(name[5:])
    return sphere_receiver() if name == "sphere" else metal_receiver()


# ---- lights --------------------------------------------------------------------------------------------------------------------------------
AREA_LIGHTS = ("rect", "sphere", "quad", "box", "map", "map_rect")
DELTA_LIGHTS = ("point", "spot", "sun")
LIGHT_FLAGS = dict(rect=F4, sphere=F4, quad=F4 | F16, box=F4 | F16, map=F8, map_rect=F4 | F8, point=0, spot=0, sun=0)
RECT_HALF = (0.3, 0.2)
SPHERE_R = 0.25
BOX_SIZE = (0.6, 0.0625, 0.4)
QUAD_VERTS = np.array([[-0.3, 0, -0.2], [0.3, 0, -0.2], [0.3, 0, 0.2], [-0.3, 0, 0.2]], np.float32)
QUAD_TRIS = ((0, 1, 2), (0, 2, 3))
MAP_SHAPE = (16, 32)
MAP_TEXELS = (((1, 29), (40.0, 30.0, 20.0)), ((14, 25), (2.5, 4.0, 6.0)))      # one above the horizon, one below
DELTA_I = (9.0, 6.0, 3.0)


def probe_map():
    m = np.zeros(MAP_SHAPE + (3,), np.float32)
    for (y, x), c in MAP_TEXELS:
        m[y, x] = c
    return m


def delta_light(light, rc):
    at, up = rc.light_at.astype(np.float32), rc.up
    if light == "point":
        return PointLight(at, DELTA_I)
    if light == "spot":       # aimed at the anchor, every probe inside the inner cone
        return SpotLight(at, -up, DELTA_I, 70.0, 80.0)
    side = np.cross(up, [0.0, 0.0, 1.0])
    return DirectionalLight(-(up + 0.25 * side / np.linalg.norm(side)), (2.0, 1.5, 1.0))


def unreachable(scene, what):
    """an object no path meets in practice: a sphere of radius 0.01 at distance 1000 subtends 3e-10 sr, so among the 1.6e6 bounces of a
    table's largest call fewer than 1e-3 are expected to find it.  `checker`: an expensive texture (the frame takes shading mode 0);
    `ggx`: a GgxMat (the frame takes the GX kernels)"""
    if what == "checker":
        m = scene.add_material(LambertianMat.new(CheckerTexture.with_colors((0.2, 0.4, 0.1), (0.9, 0.9, 0.9), 10.0)))
    else:
        m = scene.add_material(GgxMat.new((0.9, 0.7, 0.5), 0.3))
    scene.add_object(RenderObject.new(Sphere.new(0.01, m)).position(-600.0, -800.0, 0.0))


def build_scene(recv, light, extras=()):
    rc = receiver(recv)
    scene = Scene.new()
    mat = scene.add_material(LambertianMat.with_color(ALB))
    rc.add(scene, mat)
    at = rc.light_at.astype(np.float32).astype(np.float64)
    emit = scene.add_material(EmissiveMat.with_color(LE)) if light in ("rect", "sphere", "quad", "box", "map_rect") else None
    if light in ("rect", "map_rect"):
        scene.add_object(RenderObject.new(XZRect.new(-RECT_HALF[0], RECT_HALF[0], -RECT_HALF[1], RECT_HALF[1], 0, emit)).position(*at))
    elif light == "sphere":
        scene.add_object(RenderObject.new(Sphere.new(SPHERE_R, emit)).position(*at))
    elif light == "quad":
        scene.add_object(RenderObject.new(TriangleMesh(QUAD_VERTS, np.array(QUAD_TRIS, np.uint32).ravel(), material=emit)).position(*at))
    elif light == "box":
        scene.add_object(RenderObject.new(Rect3d.with_size(BOX_SIZE, emit)).position(*(at - 0.5 * np.asarray(BOX_SIZE))))
    if light in ("map", "map_rect"):
        scene.set_environment(HdrEnvironment(probe_map()))
    else:
        scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    if light in DELTA_LIGHTS:
        scene.add_light(delta_light(light, rc))
    for e in extras:
        unreachable(scene, e)
    return scene


def quadrature(recv, light, P, scene, fine=1):
    """the light(s) of build_scene(recv, light) seen from P"""
    at = receiver(recv).light_at.astype(np.float32).astype(np.float64)
    if light in ("rect", "sphere", "map_rect"):
        (l,) = _lib.selftest_lights(scene.to_desc())
    if light == "rect":
        return rect_set(l, P, LE, 160 * fine)
    if light == "sphere":
        return sphere_set(l, P, LE, 160 * fine)
    if light == "quad":
        e = _lib.selftest_emitters(scene.to_desc())
        assert len(e["obj"]) == 2 and np.allclose(e["area"], 0.5 * 4 * RECT_HALF[0] * RECT_HALF[1], rtol=1e-6)
        return mesh_set(QUAD_VERTS.astype(np.float64) + at, QUAD_TRIS, P, LE, 96 * fine)
    if light == "box":
        e = _lib.selftest_emitters(scene.to_desc())
        assert len(e["obj"]) == 6
        size = np.asarray(BOX_SIZE, np.float32).astype(np.float64)
        return box_set((at - 0.5 * np.asarray(BOX_SIZE)).astype(np.float32).astype(np.float64), size, P, LE, 120 * fine)
    if light == "map":
        return map_set(probe_map(), 1.0, 64 * fine)
    assert light == "map_rect" and l["p_pick"] == 1.0
    # beside the map the emitters share 1 - p_env = 1/2 of the picks; fw_selftest_lights reports the pick among emitters
    return QSet.join([rect_set(l, P, LE, 160 * fine, scale=0.5), map_set(probe_map(), 0.5, 64 * fine)])


class Table:
    pass


RECEIVER_LIGHTS = (
    [("mesh_%s" % s, l) for s in (0.05, 1) for l in ("rect", "point")]
    # (|n| = 4 has no deterministic probe: on the axis itself, c = |n|, kappa is already 3 c (t+^3 + t-^3) / (s (t+^3 - t-^3)) = 18.6)
    + [("mesh_4", "rect"), ("mesh_4", "sphere")]
    + [("mesh_%s" % s, l) for s in (0.3, 1.7) for l in AREA_LIGHTS + DELTA_LIGHTS]
    + [(r, l) for r in ("mesh_rot_1.7", "mesh_vn_1", "rect_rotated", "sphere", "rect_below", "rect_flipped", "metal") for l in ("rect", "point")]
    + [("sphere", "sun"), ("mesh_rot_1.7", "map"), ("rect_rotated", "sphere")])


@functools.lru_cache(maxsize=None)
def table(recv, light):
    """the probe table of one scene: rays, want (k, 3), the estimators' per-sample variances, N, and for delta lights kappa"""
    rc = receiver(recv)
    scene = build_scene(recv, light)
    t = Table()
    t.recv, t.light, t.flags, t.bvh = recv, light, LIGHT_FLAGS[light], rc.bvh
    t.rays = np.stack([p.ray for p in rc.probes])
    t.stochastic = light not in DELTA_LIGHTS
    t.want, t.var_nee, t.var_default, t.kappa, t.zero_safe = [], [], [], [], []
    for p in rc.probes:
        f = p.beta * np.asarray(ALB)
        if t.stochastic:
            q = quadrature(recv, light, p.P, scene)
            mo = moments(q, p.n, f)
            t.want.append(mo["want"]); t.var_nee.append(mo["var_nee"]); t.var_default.append(mo["var_default"])
            t.kappa.append(1.0)
            t.zero_safe.append(mo["zero_safe"])
        else:
            lt = delta_light(light, rc)
            w, L, _ = DR.incident(lt, p.P)
            t.want.append(DR.contribution(lt, p.P, p.n, ALB, beta=p.beta))
            t.var_nee.append(np.zeros(3)); t.var_default.append(np.zeros(3))
            pos = DR.scatter_pdf(p.n, w) > 0
            t.kappa.append(kappa(p.n, w) if pos else 1.0)
            t.zero_safe.append(bool(outside(p.n, w)))
    for k in ("want", "var_nee", "var_default", "kappa"):
        setattr(t, k, np.asarray(getattr(t, k), np.float64))
    t.zero_safe = np.asarray(t.zero_safe, bool)
    t.need = np.array([samples_for(t.want[k], t.var_nee[k]) for k in range(len(rc.probes))]) if t.stochastic else np.full(len(rc.probes), 16)
    t.N = int(t.need.max())
    return t


# ---- the isotropic medium's tables -------------------------------------------------------------------------------------------------------
MEDIUM_R, MEDIUM_RHO = 2.0, 0.5
MEDIUM_ALB = 2.0 ** -14
MEDIUM_LIGHTS = dict(point=PointLight((0.5, 8.0, 0.3), (9.0e6, 6.0e6, 3.0e6)), sun=DirectionalLight((0.2, -1.0, 0.15), (2.0e5, 1.5e5, 1.0e5)))
MEDIUM_RAYS = np.array([[0.1, 4.0, 0.2, 0.05, -1.0, 0.02], [1.2, 4.0, -0.5, -0.1, -1.0, 0.15], [-0.8, 4.0, 1.1, 0.3, -1.0, -0.35]], np.float32)


def medium_scene(light):
    scene = Scene.new()
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    scene.add_volume(RenderObject.new(Sphere.new(MEDIUM_R, 0)), MEDIUM_RHO, ConstantTexture.new((MEDIUM_ALB,) * 3))
    scene.add_light(MEDIUM_LIGHTS[light])
    return scene


@functools.lru_cache(maxsize=None)
def medium_table(light):
    """want, variance, N and the bound on every higher order.  A path's k-th vertex (k >= 2) carries beta = albedo^(k-1) and adds at most
    albedo x beta x max L / 4 pi (p_b = 1 / 4 pi, transmittance <= 1), whatever the geometry: the orders beyond the first sum to at most
    albedo^2 / (1 - albedo) x max L / 4 pi.  albedo is the power of two that keeps this under a tenth of the tolerance 4 sqrt(var / N)."""
    t = Table()
    t.rays = MEDIUM_RAYS
    res = [medium_answer(r, (0, 0, 0), MEDIUM_R, MEDIUM_RHO, MEDIUM_ALB, MEDIUM_LIGHTS[light]) for r in MEDIUM_RAYS]
    t.want = np.array([r[0] for r in res])
    t.var_nee = np.array([r[1] for r in res])
    t.need = np.array([samples_for(t.want[k], t.var_nee[k]) for k in range(len(res))])
    t.N = int(t.need.max())
    t.higher = np.array([MEDIUM_ALB ** 2 / (1 - MEDIUM_ALB) * r[2] for r in res])
    return t
