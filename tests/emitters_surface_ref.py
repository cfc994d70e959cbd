"""What the tests of every emitter at surface points share: a float64 restatement of the world-space records, records
made by hand, the closed forms and known-answer scenes, the estimate the numpy statements give when every sample that faces the
receiver arrives, a plain-loop restatement of fw_emitters_reduce, and the scenes of the device tests."""
import numpy as np

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import (Disk, EmissiveMat, EmitterLights, LambertianMat, Rect3d, RenderObject, Scene, Sphere, TriangleMesh, XYRect, XZRect,
                              YZRect)

import area_ref as AR
import emitters_ref as ER

F32 = np.float32
NO_HIT = A.FW_NO_HIT
DEAD = 0xFFFFFFFF


# ---- the records, restated ------------------------------------------------------------------------------------------------------------
def rows32(rotor):
    """the runtime's float32 rotation rows of a Rotor3, operation for operation"""
    s, xy, xz, yz = (F32(v) for v in (rotor.s, rotor.xy, rotor.xz, rotor.yz))
    two = F32(2.0)
    s2, a2, b2, c2 = s * s, xy * xy, xz * xz, yz * yz
    sa, sb, sc = s * xy, s * xz, s * yz
    bc, ac, ab = xz * yz, xy * yz, xy * xz
    c0 = [s2 - a2 - b2 + c2, -two * (bc + sa), two * (ac - sb)]
    c1 = [two * (sa - bc), s2 - a2 + b2 - c2, -two * (sc + ab)]
    c2_ = [two * (sb + ac), two * (sc - ab), s2 + a2 - b2 - c2]
    return np.array([[c0[i], c1[i], c2_[i]] for i in range(3)], F32)


def is_rotated(R):
    return bool(F32(0.5) * ((R[0, 0] + R[1, 1] + R[2, 2]) - F32(1.0)) < F32(0.999))


def world64(R, rotated, pos, p):
    """float(((R0 x + R1 y) + R2 z) + position) per component, float64 from the float32 rows; no rotation where the walks do none"""
    p = [float(F32(v)) for v in p]
    Rd = R.astype(np.float64)
    w = [((Rd[c, 0] * p[0] + Rd[c, 1] * p[1]) + Rd[c, 2] * p[2]) if rotated else p[c] for c in range(3)]
    return np.array([w[c] + float(F32(pos[c])) for c in range(3)]).astype(F32)


def records_ref(scene):
    """(records (N, 16) float32, codes (N, 2) uint32) of a Python Scene: entries, areas and weights as emitters_ref.entries gives them,
    the geometry of everything but spheres and rectangles restated in float64 and rounded once (spheres and rectangles: zeros here,
    they are compared with fw_selftest_lights)"""
    ent = ER.entries(scene)
    n = ent["obj"].size
    rec, codes = np.zeros((n, 16), F32), np.zeros((n, 2), np.uint32)
    for e in range(n):
        i, k, kind = int(ent["obj"][e]), int(ent["prim"][e]), int(ent["kind"][e])
        ro = scene.render_objects[i]
        s = ro.obj
        R = rows32(ro.rotation)
        rot = is_rotated(R)
        pos = [float(v) for v in np.asarray(ro._position, F32)]
        rec[e, 0], rec[e, 1], rec[e, 14], rec[e, 15] = i, kind, ent["area"][e], ent["weight"][e]
        codes[e] = (i, k)
        g = rec[e, 2:14]
        if kind == A.FW_SHAPE_RECT3D:
            lo = np.asarray(s.pos, F32)
            hi = lo + np.asarray(s.size, F32)                                                # float32 sums, as the walks form them
            ax = k >> 1
            ia, ib, ik = (0, 1, 2) if ax == 0 else ((0, 2, 1) if ax == 1 else (1, 2, 0))
            kk = lo[ik] if k & 1 else hi[ik]
            for c, (a, b) in enumerate([(lo[ia], lo[ib]), (hi[ia], lo[ib]), (hi[ia], hi[ib]), (lo[ia], hi[ib])]):
                p = [0.0, 0.0, 0.0]
                p[ia], p[ib], p[ik] = a, b, kk
                g[3 * c:3 * c + 3] = world64(R, rot, pos, p)
        elif kind == A.FW_SHAPE_TRIANGLE_MESH:
            tri = s.verts.astype(F32)[s.indicies.reshape(-1, 3)[k]]
            for c in range(3):
                g[3 * c:3 * c + 3] = world64(R, rot, pos, tri[c])
        elif kind == A.FW_SHAPE_DISK:
            g[0:3] = np.asarray(pos, F32)
            g[3:6] = R[:, 0] if rot else (1, 0, 0)
            g[6:9] = R[:, 2] if rot else (0, 0, 1)
            g[9:12] = (F32(s.radius), F32(s.inner_radius), F32(s.phi_max))
    return rec, codes


# ---- records made by hand -------------------------------------------------------------------------------------------------------------
def _finish(r, area, power):
    r[14] = area
    w = float(F32(area)) * power
    r[15] = w if np.isfinite(w) and w > 0 else 0.0
    return r


def sphere_record(obj, centre, radius, power=1.0):
    return _finish(AR.sphere_record(obj, centre, radius), 4.0 * np.pi * radius * radius, power)


def rect_record(obj, c0, c1, c2, c3, kind=A.FW_SHAPE_XZRECT, power=1.0):
    r = AR.rect_record(obj, c0, c1, c2, c3, kind)
    return _finish(r, float(r[14]), power)


def tri_record(obj, v0, v1, v2, power=1.0):
    r = np.zeros(16, F32)
    r[0], r[1] = obj, A.FW_SHAPE_TRIANGLE_MESH
    r[2:11] = np.concatenate([v0, v1, v2])
    v = r[2:11].astype(np.float64).reshape(3, 3)
    return _finish(r, 0.5 * np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])), power)


def disk_record(obj, centre, ax, az, radius, inner=0.0, phi_max=2 * np.pi, power=1.0):
    r = np.zeros(16, F32)
    r[0], r[1] = obj, A.FW_SHAPE_DISK
    r[2:5], r[5:8], r[8:11], r[11:14] = centre, ax, az, (radius, inner, phi_max)
    return _finish(r, 0.5 * float(F32(phi_max)) * (float(F32(radius)) ** 2 - float(F32(inner)) ** 2), power)


def mixed_records(n, rng):
    """(records, codes) of n entries cycling through sphere, rectangle, Rect3d face, triangle and disk, of any orientation, a few units
    above the origin, with powers that differ; one entry in seven has weight 0 (never picked)"""
    out, codes = [], []
    for i in range(n):
        c = rng.uniform(-2.0, 2.0, 3) + (0.0, 3.0, 0.0)
        e1 = rng.normal(size=3)
        e2 = np.cross(e1, rng.normal(size=3))
        e1, e2 = e1 / np.linalg.norm(e1) * rng.uniform(0.3, 1.5), e2 / np.linalg.norm(e2) * rng.uniform(0.3, 1.5)
        power = 0.0 if i % 7 == 3 else float(rng.uniform(0.2, 5.0))
        obj, k = 3 * (i // 2) + 1, i % 5
        if k == 0:
            out.append(sphere_record(obj, c, rng.uniform(0.1, 0.6), power))
        elif k == 1:
            out.append(rect_record(obj, c, c + e1, c + e1 + e2, c + e2, 1 + i % 3, power))
        elif k == 2:
            out.append(rect_record(obj, c, c + e1, c + e1 + e2, c + e2, A.FW_SHAPE_RECT3D, power))
        elif k == 3:
            out.append(tri_record(obj, c, c + e1, c + e2, power))
        else:
            out.append(disk_record(obj, c, e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2), rng.uniform(0.4, 1.2), rng.uniform(0.0, 0.3),
                                   rng.uniform(1.0, 2 * np.pi), power))
        codes.append((obj, i % 6 if k in (2, 3) else 0))
    return np.array(out, F32), np.array(codes, np.uint32)


def liveness_margins(em, records, cdf, positions, normals, round=0):
    """(M, S) float64: how far each entry of every point is from the boundary of its liveness tests in the statement's own float64
    arithmetic (the statement's internal entries: the tests choose their points with it, so that no last bit of sin, cos or sqrt
    decides a case)"""
    return api._emitters_entries(em, records, cdf, positions, normals, None, round)[4].reshape(-1, int(em.samples))


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
def disk_axis_irradiance(h, radius, L, inner=0.0, phi_max=2 * np.pi):
    """pi L r^2 / (h^2 + r^2) on the axis of a full disk facing the receiver, times phi_max / 2 pi for a sector, less the inner disk's"""
    full = lambda r: np.pi * r * r / (h * h + r * r)
    return (full(radius) - full(inner)) * (phi_max / (2 * np.pi)) * np.asarray(L, np.float64)


# ---- the known-answer cases -----------------------------------------------------------------------------------------------------------
# Every case: emitters of constant radiance and one receiver that every emitter sees unoccluded except by itself (a box's far faces).
S, ROUNDS, SEED = 64, 4, 11
L_A, L_B = (4.0, 3.0, 2.0), (1.0, 2.5, 0.5)
TRI = [(-0.5, 1.0, -0.4), (0.6, 1.0, -0.3), (0.1, 1.2, 0.7)]
FACE_P = (0.2, 0.0, 0.1)
DISK_H, DISK_R, DISK_IN, SECTOR_DEG = 1.2, 0.8, 0.3, 200.0
BOX_LO, BOX_SIZE = (-0.3, 0.8, 1.4), (0.6, 0.1, 0.6)
QUAD5 = [(-2.0, 0.8, -0.3), (-1.4, 0.8, -0.3), (-1.4, 0.8, 0.3), (-2.0, 0.8, 0.3)]
RING_H, RING_R, RING_IN = 2.0, 2.0, 1.6
SPHERE5_C, SPHERE5_R = (1.5, 1.0, 1.5), 0.3
# The statement's own relative error against the closed form at (S, ROUNDS, SEED), measured with tests/test_emitters_surface_cpu.py's
# test_known_answers (which prints it) on the host: the largest over the channels.  The tests allow four times as much, because the
# lattice's error moves with the jitter seed (DESIGN.md §9zc records both numbers).
MEASURED = {"triangle": 5.006e-04, "quad": 4.747e-04, "face": 7.940e-03, "rect": 1.032e-02, "disk": 2.183e-03, "sector": 2.183e-03,
            "annulus": 1.811e-03, "sphere": 4.137e-05, "five": 2.128e-02}
# ... and at S = 16 384, one round: what the statement reaches there (measured the same way; the convergence test allows four times it)
CONVERGED = {"triangle": 3.810e-07, "quad": 6.907e-05, "face": 2.498e-05, "rect": 6.545e-06, "disk": 1.630e-05, "sector": 1.637e-05,
             "annulus": 1.358e-05, "sphere": 4.403e-07, "five": 2.388e-05}
MARGIN = 4.0


def _mesh(corners, tris, material):
    return TriangleMesh(np.array(corners, F32), np.array(tris, np.uint32).reshape(-1), material=material)


def case_scene(name, emitter=None):
    """the scene of a case; emitter: the first lamp's material (default: EmissiveMat of L_A)"""
    scene = Scene.new()
    m = scene.add_material(emitter if emitter is not None else EmissiveMat.with_color(L_A))
    lamp = lambda mat: RenderObject.new(XZRect.new(AR.LAMP["x0"], AR.LAMP["x1"], AR.LAMP["z0"], AR.LAMP["z1"], AR.LAMP["y"], mat))
    if name == "triangle":
        scene.add_object(RenderObject.new(_mesh(TRI, [0, 1, 2], m)))
    elif name == "quad":
        scene.add_object(RenderObject.new(_mesh(AR.LAMP_CORNERS, [0, 1, 2, 0, 2, 3], m)))
    elif name == "face":
        scene.add_object(RenderObject.new(Rect3d.with_size((1.0, 0.2, 1.0), m)).position(-0.5, 1.0, -0.5))
    elif name == "rect":
        scene.add_object(lamp(m))
    elif name == "disk":
        scene.add_object(RenderObject.new(Disk.new(DISK_R, m)).position(0.0, DISK_H, 0.0))
    elif name == "sector":
        scene.add_object(RenderObject.new(Disk.partial(DISK_R, SECTOR_DEG, 0.0, m)).position(0.0, DISK_H, 0.0))
    elif name == "annulus":
        scene.add_object(RenderObject.new(Disk.partial(DISK_R, 360.0, DISK_IN, m)).position(0.0, DISK_H, 0.0))
    elif name == "sphere":
        scene.add_object(RenderObject.new(Sphere.new(AR.SPHERE_R, m)).position(*AR.SPHERE_C))
    elif name == "five":
        m2 = scene.add_material(EmissiveMat.with_color(L_B))
        scene.add_object(lamp(m))
        scene.add_object(RenderObject.new(Sphere.new(SPHERE5_R, m2)).position(*SPHERE5_C))
        scene.add_object(RenderObject.new(Disk.partial(RING_R, 360.0, RING_IN, m)).position(0.0, RING_H, 0.0))
        scene.add_object(RenderObject.new(_mesh(QUAD5, [0, 1, 2, 0, 2, 3], m2)))
        scene.add_object(RenderObject.new(Rect3d.with_size(BOX_SIZE, m)).position(*BOX_LO))
    else:
        raise KeyError(name)
    return scene


def _box_faces(lo, size):
    """the corners of the faces -y and -z of a box: the two that face a receiver below and in front of it"""
    (x0, y0, z0), (x1, y1, z1) = lo, np.add(lo, size)
    return [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)]


def cases():
    """name -> (point, normal, the closed form's E (3,) float64)"""
    up, o = (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)
    LA, LB = np.asarray(L_A, np.float64), np.asarray(L_B, np.float64)
    ph = float(F32(SECTOR_DEG) * F32(np.pi / 180.0))
    face = [(-0.5, 1.0, -0.5), (0.5, 1.0, -0.5), (0.5, 1.0, 0.5), (-0.5, 1.0, 0.5)]
    bottom, front = _box_faces(BOX_LO, BOX_SIZE)
    five = (AR.polygon_irradiance(o, up, AR.LAMP_CORNERS, LA) + AR.sphere_irradiance(o, up, SPHERE5_C, SPHERE5_R, LB)
            + disk_axis_irradiance(RING_H, RING_R, LA, RING_IN) + AR.polygon_irradiance(o, up, QUAD5, LB)
            + AR.polygon_irradiance(o, up, bottom, LA) + AR.polygon_irradiance(o, up, front, LA))
    return {
        "triangle": (o, up, AR.polygon_irradiance(o, up, TRI, LA)),
        "quad": ((0.7, 0.0, 0.3), (0.2, 1.0, 0.1), AR.polygon_irradiance((0.7, 0, 0.3), (0.2, 1, 0.1), AR.LAMP_CORNERS, LA)),
        "face": (FACE_P, up, AR.polygon_irradiance(FACE_P, up, face, LA)),
        "rect": ((0.7, 0.0, 0.3), (0.2, 1.0, 0.1), AR.polygon_irradiance((0.7, 0, 0.3), (0.2, 1, 0.1), AR.LAMP_CORNERS, LA)),
        "disk": (o, up, disk_axis_irradiance(DISK_H, DISK_R, LA)),
        "sector": (o, up, disk_axis_irradiance(DISK_H, DISK_R, LA, 0.0, ph)),
        "annulus": (o, up, disk_axis_irradiance(DISK_H, DISK_R, LA, DISK_IN)),
        "sphere": (o, up, AR.sphere_irradiance(o, up, AR.SPHERE_C, AR.SPHERE_R, LA)),
        "five": (o, up, five),
    }


_FACE_NORMAL = np.array([(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)], np.float64)


def facing(records, codes, point):
    """(N,) bool: False for the faces of an (unrotated) Rect3d whose outward normal points away from `point` — the box itself hides
    them; True for every other entry"""
    rec = np.asarray(records, F32).reshape(-1, 16)
    out = np.ones(rec.shape[0], bool)
    for e in np.nonzero(rec[:, 1] == A.FW_SHAPE_RECT3D)[0]:
        out[e] = _FACE_NORMAL[int(codes[e][1])] @ (np.asarray(point, np.float64) - rec[e, 2:5].astype(np.float64)) > 0
    return out


def statement_estimate(scene, point, normal, samples=S, rounds=ROUNDS, seed=SEED):
    """(E (3,), vis) float32 as the device would resolve them: the scene's records (fw_selftest_emitters_records) and their cdf,
    api.emitters_rays' picks and weights of `rounds` rounds, every live ray arriving at its entry — except on a box's faces that look
    away from the receiver — with the entry's constant emission, through api.emitters_reduce, float32 sums and api.emitters_resolve"""
    rec, codes = _lib.emitters_records(scene.to_desc())
    cdf, total = api.emitters_cdf(rec[:, 15])
    assert total > 0
    em = EmitterLights(samples, 0.0).seed(seed)                               # (the receivers float free of any surface: no bias)
    emission = np.array([scene.materials[scene.render_objects[int(o)].obj.material].albedo.color for o in codes[:, 0]], F32)
    seen = facing(rec, codes, point)
    sums = np.zeros((1, 4), F32)
    P, N = np.array([point], F32), np.array([normal], F32)
    for r in range(rounds):
        _rays, w, picks = api.emitters_rays(em, rec, cdf, P, N, round=r)
        at = np.where(picks == DEAD, 0, picks).astype(np.int64)
        surface = np.zeros((w.size, 16), F32)
        surface[:, 3], surface[:, 12:15] = 3.0, emission[at]
        hobj = np.where(seen[at], codes[at, 0], np.uint32(0x7FFFFFF0)).astype(np.uint32)
        sums = sums + api.emitters_reduce(picks, w, hobj, codes[at, 1], surface, codes, samples).astype(F32)
    out = api.emitters_resolve(sums, rounds)[0]
    return out[0:3], out[3]


# ---- a plain loop written from the header's statement of the reduction ----------------------------------------------------------------
def reduce_loop(picks, weights, hits_object, hits_prim, surface, codes, samples):
    S_ = int(samples)
    w = np.asarray(weights, F32).reshape(-1, S_)
    pk = np.asarray(picks).astype(np.uint32).reshape(-1, S_)
    ho, hp = np.asarray(hits_object).astype(np.uint32).reshape(-1, S_), np.asarray(hits_prim).astype(np.uint32).reshape(-1, S_)
    s = np.asarray(surface, F32).reshape(-1, S_, 16)
    G = 1
    while G < min(S_, 64):
        G *= 2
    out = np.zeros((w.shape[0], 4))
    for q in range(w.shape[0]):
        part = [[0.0, 0.0, 0.0, 0.0] for _ in range(G)]
        for m in range(S_):
            i = int(pk[q, m])
            if not (w[q, m] > 0) or i >= len(codes) or s[q, m, 3] != 3.0 or int(ho[q, m]) != int(codes[i][0]) or int(hp[q, m]) != int(codes[i][1]):
                continue
            p = part[m % G]
            for c in range(3):
                p[c] = p[c] + float(s[q, m, 12 + c]) * float(w[q, m])
            p[3] = p[3] + 1.0
        d = G // 2
        while d >= 1:
            part = [[part[l][c] + part[l ^ d][c] for c in range(4)] for l in range(G)]
            d //= 2
        out[q] = [(1.0 / S_) * part[0][c] for c in range(4)]
    return out


def synthetic_entries(n, samples, rng, n_entries=9):
    """(picks, weights, hits (n S, 12) float32 as the device holds them, surface, codes) covering every outcome: visible, the right object
    with the wrong prim, another object, a kind other than 3, a weight of 0 (a dead entry), a miss"""
    total = n * samples
    codes = np.stack([np.repeat(np.sort(rng.choice(1000, (n_entries + 1) // 2, replace=False)), 2)[:n_entries],
                      rng.integers(0, 40, n_entries)], axis=1).astype(np.uint32)
    picks = rng.integers(0, n_entries, total).astype(np.uint32)
    w = rng.uniform(0.01, 2.0, total).astype(F32)
    hits = rng.normal(size=(total, 12)).astype(F32)
    hobj, hprim = codes[picks, 0].copy(), codes[picks, 1].copy()
    surface = rng.uniform(0.0, 9.0, (total, 16)).astype(F32)
    surface[:, 3] = 3.0
    what = rng.integers(0, 7, total)
    hprim = np.where(what == 1, hprim + 1, hprim)
    hobj = np.where(what == 2, hobj + 1, hobj)
    surface[what == 3, 3] = rng.choice([-2.0, -1.0, 0.0, 1.0, 5.0], int((what == 3).sum()))
    w[what == 4] = 0.0
    picks[what == 4] = DEAD
    hobj = np.where(what == 5, NO_HIT, hobj)
    hits.view(np.uint32)[:, 10] = hobj.astype(np.uint32)
    hits.view(np.uint32)[:, 11] = hprim.astype(np.uint32)
    return picks, w, hits, surface, codes


# ---- scenes of the device tests -------------------------------------------------------------------------------------------------------
def grid_mesh(n, size, material, y=0.0):
    s = np.linspace(-size, size, n + 1)
    X, Z = np.meshgrid(s, s, indexing="ij")
    verts = np.stack([X, np.full_like(X, y), Z], -1).reshape(-1, 3).astype(F32)
    idx = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            idx += [a, b, c, a, c, d]
    return TriangleMesh(verts, np.array(idx, np.uint32), material=material)


def lit_room(mesh_material=None):
    """area_ref.lit_room — a floor, a rectangle lamp (object 1), a grey ball, an emissive sphere (3) and an emissive Rect3d (4) — plus
    a mesh lamp of 8 triangles (5; its material may be given) and an emissive partial disk (6), tilted, over the floor; sized for the
    CLI's fixed view from (0, 30, 50)"""
    from firework_amd.api import Rotor3
    scene = AR.lit_room()
    mm = scene.add_material(mesh_material if mesh_material is not None else EmissiveMat.with_color((6.0, 2.0, 7.0)))
    scene.add_object(RenderObject.new(grid_mesh(2, 1.5, mm)).rotate(Rotor3.from_rotation_yz(0.5)).position(-3.0, 6.0, -6.0))
    scene.add_object(RenderObject.new(Disk.partial(1.5, 250.0, 0.4, scene.add_material(EmissiveMat.with_color((1.0, 6.0, 2.0)))))
                     .rotate(Rotor3.from_rotation_xy(0.3)).position(6.0, 5.0, 4.0))
    return scene


def floor_points(n, rng, extent=12.0):
    """n points on lit_room's floor with its normal"""
    P = np.zeros((n, 3), F32)
    P[:, 0], P[:, 2] = rng.uniform(-extent, extent, n), rng.uniform(-extent, extent, n)
    N = np.tile(np.array([0.0, 1.0, 0.0], F32), (n, 1))
    return P, N
