"""Float64 restatement of FW_FLAG_ALL_EMITTERS's entries from a Python Scene, and the quadrature the GPU tests compare with.

An entry is one emitting primitive of an object whose material is an EmissiveMat of positive power: a sphere, an axis-aligned rectangle,
a disk (one each), a Rect3d (six faces, +z -z +y -y +x -x), a TriangleMesh (one per triangle).  weight = object-space area x power, power = max(r, g, b) of a
ConstantTexture (negative and non-finite channels counted as 0), 1 for any other texture.  Shape parameters are taken as the float32 values
the description carries."""
import numpy as np

from firework_amd import _abi as A
from firework_amd.api import ConstantTexture, Disk, EmissiveMat, Rect3d, Sphere, TriangleMesh, XYRect, XZRect, YZRect

f32 = lambda v: float(np.float32(v))


def power(mat):
    t = mat.albedo
    if not isinstance(t, ConstantTexture):
        return 1.0
    c = np.asarray(t.color, np.float32).astype(np.float64)
    c = np.where(np.isfinite(c) & (c > 0), c, 0.0)
    return float(c.max())


def tri_areas(mesh):
    v = mesh.verts.astype(np.float64)[mesh.indicies.reshape(-1, 3)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def areas(shape):
    """object-space areas of a shape's entries; None: not an entry kind"""
    if isinstance(shape, Sphere):
        return np.array([4 * np.pi * f32(shape.radius) ** 2]), A.FW_SHAPE_SPHERE
    if isinstance(shape, (XYRect, XZRect, YZRect)):
        return np.array([abs((f32(shape.a_max) - f32(shape.a_min)) * (f32(shape.b_max) - f32(shape.b_min)))]), shape.KIND
    if isinstance(shape, Rect3d):
        sx, sy, sz = (float(x) for x in np.asarray(shape.size, np.float32))
        return np.abs(np.array([sx * sy, sx * sy, sx * sz, sx * sz, sy * sz, sy * sz])), A.FW_SHAPE_RECT3D
    if isinstance(shape, Disk):
        r, ri, ph = f32(shape.radius), f32(shape.inner_radius), f32(shape.phi_max)
        return np.array([0.5 * ph * (r * r - ri * ri)]), A.FW_SHAPE_DISK
    if isinstance(shape, TriangleMesh):
        return tri_areas(shape), A.FW_SHAPE_TRIANGLE_MESH
    return None, None


def entries(scene):
    """-> dict of arrays obj, prim, kind, area, weight: one element per entry, in object order"""
    out = dict(obj=[], prim=[], kind=[], area=[], weight=[])
    for i, ro in enumerate(scene.render_objects):
        s = ro.obj
        m = getattr(s, "material", None)
        if m is None or not isinstance(scene.materials[m], EmissiveMat):
            continue
        a, kind = areas(s)
        pw = power(scene.materials[m])
        if a is None or not pw > 0:          # not an entry kind, or a black emitter: no entries
            continue
        w = a * pw
        w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
        out["obj"] += [i] * len(a); out["prim"] += list(range(len(a))); out["kind"] += [kind] * len(a)
        out["area"] += list(a); out["weight"] += list(w)
    return {k: np.asarray(v, np.float64 if k in ("area", "weight") else np.int64) for k, v in out.items()}


def rotation(rotor):
    """the rotation matrix of a Rotor3 (the reference's rotor to Mat3, scene.rs), in float64"""
    s, a, b, c = (float(np.float32(v)) for v in (rotor.s, rotor.xy, rotor.xz, rotor.yz))
    c0 = [s * s - a * a - b * b + c * c, -2 * (b * c + s * a), 2 * (a * c - s * b)]
    c1 = [2 * (s * a - b * c), s * s - a * a + b * b - c * c, -2 * (s * c + a * b)]
    c2 = [2 * (s * b + a * c), 2 * (s * c - a * b), s * s + a * a - b * b - c * c]
    return np.array([c0, c1, c2]).T


def flat_integral(points, normal, dA, P):
    """int 2 cos^3(theta) / pi dw over a flat emitter seen from floor point P (normal +y): points (n, 3) of the emitter in the world, its
    normal, the area each point stands for"""
    X = points - np.asarray(P, np.float64)
    d2 = (X ** 2).sum(-1)
    d = np.sqrt(d2)
    cos_t = np.clip(X[:, 1] / d, 0, None)
    cos_l = np.abs(X @ normal) / d
    return float((2 * cos_t ** 3 / np.pi * cos_l / d2 * dA).sum())


def grid(n):
    s = (np.arange(n) + 0.5) / n
    S, T = np.meshgrid(s, s, indexing="ij")
    return S.ravel(), T.ravel()
