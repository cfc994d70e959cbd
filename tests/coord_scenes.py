"""Scenes far from the origin and at extreme scales, and rays that graze triangle edges and box corners (helper module, not a test file).

The walks cull with boxes grown by margins relative to the items' own sizes (fw_runtime.cpp: grown_by) while the rounding of a plane's
distance (fw_kernels.hip: wide_step, FW_WIDE_FMA) grows with the ray origin's coordinate.  The scenes here move that ratio: small
triangles whose vertex data lies far off (a), the same mesh placed by a transform (b), a cluster of small objects far off (c), and
exact power-of-two rescalings of the baseline scenes (d), where only the absolute constants (t_min, tmax, the SOFT class's -1/16) see
a difference.  Every generator is deterministic and returns (scene, renderer)."""
import copy

import numpy as np

from firework_amd import scenes
from firework_amd.api import (CameraSettings, Cone, ConstantMedium, ConstantTexture, Cylinder, DielectricMat, Disk, EmissiveMat,
                              LambertianMat, MetalMat, Rect3d, RenderObject, Renderer, Rotor3, Scene, SkyEnv, Sphere, TriangleMesh,
                              XYRect, XZRect, YZRect, _AARect)

F32 = np.float32

# (a) / (b): (name, offset O, triangle size h).  |O| / h runs from 2^10 to past 2^20.
MESH_CASES = [
    ("origin", (0.0, 0.0, 0.0), 0.03),
    ("o1e3_h1", (1e3, 0.0, 0.0), 1.0),                       # 2^10
    ("o1e3", (1e3, -1e3, 1e3), 0.03),                        # 2^15
    ("o2p14", (-2.0 ** 14 + 0.37, 1e3, 0.0), 0.06),          # 2^18
    ("o1e4", (1e4, 1e4, -1e4), 0.03),                        # 2^18.3
    ("o3e4", (3e4, -3e4, 3e4), 0.03),                        # 2^19.9
    ("o3e4_fine", (0.0, 3e4, -3e4), 0.02),                   # 2^20.5
]
GRID = 37            # GRID x GRID vertices: 2 x 36^2 = 2592 triangles
SCALES = (-10, -6, 6, 12)
BASES = ("C1", "C2", "C3", "R2")


def mesh_ratio(offset, h):
    return max(abs(float(F32(c))) for c in offset) / h


def _patch(h, seed, n=GRID):
    """A bumpy n x n patch in the xy plane (facing -z) centred at 0, triangle legs h: local coordinates, float64."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = (i - (n - 1) / 2) * h + rng.uniform(-0.15, 0.15, i.shape) * h
    y = (j - (n - 1) / 2) * h + rng.uniform(-0.15, 0.15, i.shape) * h
    r = (n - 1) * h / 2
    z = 0.25 * r * np.cos(2.1 * x / r) * np.cos(1.7 * y / r) + rng.uniform(-0.1, 0.1, i.shape) * h
    verts = np.stack([x, y, z], -1).reshape(-1, 3)
    q = (i[:-1, :-1] * n + j[:-1, :-1]).ravel()
    flip = (i[:-1, :-1] + j[:-1, :-1]).ravel() % 2 == 1            # alternate diagonals: vertices shared by 4 and by 8 triangles
    a, b, c, d = q, q + n, q + n + 1, q + 1
    t1 = np.where(flip[:, None], np.stack([a, b, d], 1), np.stack([a, b, c], 1))
    t2 = np.where(flip[:, None], np.stack([b, c, d], 1), np.stack([a, c, d], 1))
    return verts, np.concatenate([t1, t2]).ravel().astype(np.uint32)


def _mesh_camera(centre, h, seed):
    rng = np.random.default_rng(seed + 100)
    r = (GRID - 1) * h / 2
    back = float(np.clip(2.2 * r, 1.0, 4.0))
    eye = np.asarray(centre, np.float64) + np.array([rng.uniform(-0.3, 0.3) * r, rng.uniform(-0.3, 0.3) * r, -back])
    cam = CameraSettings.default().cam_pos(tuple(eye)).look_at(tuple(np.asarray(centre, np.float64))).field_of_view(50.0)
    return cam


def _mesh_scene(verts, idx, obj_fn):
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.7, 0.5, 0.3)))
    light = sc.add_material(EmissiveMat.with_color((4.0, 4.0, 4.0)))
    sc.add_object(obj_fn(RenderObject.new(TriangleMesh.new(verts.astype(F32), idx, None, None, m))))
    sc.set_environment(SkyEnv.default())
    return sc, light


def far_mesh(case, w=48, h=32, spp=4):
    """(a): the patch's vertex data at the offset O, no object transform."""
    name, off, tri = next(c for c in MESH_CASES if c[0] == case)
    local, idx = _patch(tri, len(name))
    verts = (local + np.asarray(off, np.float64)).astype(F32)
    sc, _ = _mesh_scene(verts, idx, lambda o: o)
    centre = np.asarray(off, np.float64)
    r = Renderer.default().width(w).height(h).samples(spp).use_bvh(True).camera(_mesh_camera(centre, tri, len(name))).seed(17)
    return sc, r


def placed_mesh(case, rotated, w=48, h=32, spp=4):
    """(b): the same patch centred at zero, placed at O by RenderObject.position (and a rotation)."""
    name, off, tri = next(c for c in MESH_CASES if c[0] == case)
    local, idx = _patch(tri, len(name))
    rot = Rotor3.from_euler_angles(0.4, -0.3, 0.2) if rotated else None

    def place(o):
        o = o.position(*off)
        return o.rotate(rot) if rotated else o
    sc, _ = _mesh_scene(local.astype(F32), idx, place)
    centre = np.asarray([float(F32(c)) for c in off], np.float64)
    cam = _mesh_camera(centre, tri, len(name))       # the rotation turns the patch by ~30 degrees: still seen from the front
    r = Renderer.default().width(w).height(h).samples(spp).use_bvh(True).camera(cam).seed(19)
    return sc, r


CLUSTER_CASES = [("c_origin", (0.0, 0.0, 0.0)), ("c_far", (1e4, -3e3, 2e4)), ("c_far3e4", (-3e4, 3e4, 2.0 ** 14 + 0.37))]


def far_cluster(case, use_bvh=True, w=48, h=32, spp=4):
    """(c): ~450 small spheres, boxes and rects, one cone, cylinder and disk, two media, around a far centre O; the camera inside."""
    off = np.asarray(dict(CLUSTER_CASES)[case], np.float64)
    rng = np.random.default_rng(31)
    u = lambda a, b: float(rng.uniform(a, b))
    sc = Scene.new()
    mats = [sc.add_material(LambertianMat.with_color((u(0.2, 0.9), u(0.2, 0.9), u(0.2, 0.9)))) for _ in range(4)]
    mats += [sc.add_material(MetalMat.new((0.8, 0.8, 0.9), 0.2)), sc.add_material(DielectricMat.new(1.5)),
             sc.add_material(EmissiveMat.with_color((5.0, 5.0, 5.0)))]
    pick = lambda: mats[int(rng.integers(len(mats)))]
    at = lambda p: tuple(off + np.asarray(p, np.float64))
    for k in range(450):
        p = (u(-6, 6), u(-3, 3), u(-2, 10))
        kind = k % 5
        if kind < 2:
            o = RenderObject.new(Sphere.new(u(0.05, 0.25), pick()))
        elif kind < 4:
            o = RenderObject.new(Rect3d.with_size((u(0.05, 0.4), u(0.05, 0.4), u(0.05, 0.4)), pick()))
            if k % 3 == 0:
                o = o.rotate(Rotor3.from_rotation_xz(u(-3, 3)))
        else:
            rect = (XYRect, XZRect, YZRect)[k % 3]
            a, b = u(-0.3, 0.0), u(-0.3, 0.0)
            o = RenderObject.new(rect.new(a, a + u(0.05, 0.4), b, b + u(0.05, 0.4), 0.0, pick()))
        sc.add_object(o.position(*at(p)))
    sc.add_object(RenderObject.new(Cone.new(0.2, 0.4, mats[0])).position(*at((1.0, -1.0, 3.0))))
    sc.add_object(RenderObject.new(Cylinder.new(0.15, 0.5, mats[1])).position(*at((-1.0, -1.0, 3.5))))
    sc.add_object(RenderObject.new(Disk.new(0.3, mats[2])).rotate(Rotor3.from_rotation_yz(0.7)).position(*at((0.0, 1.0, 4.0))))
    sc.add_volume(RenderObject.new(Sphere.new(0.3, mats[0])).position(*at((0.5, 0.2, 2.0))), 2.0, ConstantTexture.from_rgb(0.9, 0.9, 0.9))
    sc.add_volume(RenderObject.new(Rect3d.with_size((0.3, 0.3, 0.3), mats[0])).position(*at((-0.6, 0.0, 2.5))), 3.0,
                  ConstantTexture.from_rgb(0.8, 0.8, 0.9))
    sc.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 20.0, 0.0, mats[3])).position(*at((0.0, -3.5, 0.0))))
    sc.set_environment(SkyEnv.default())
    cam = CameraSettings.default().cam_pos(at((0.2, 0.3, -1.5))).look_at(at((0.0, 0.0, 4.0))).field_of_view(60.0)
    return sc, Renderer.default().width(w).height(h).samples(spp).use_bvh(use_bvh).camera(cam).seed(23)


def spread_mesh(w=48, h=32, spp=4):
    """A mesh of 0.03-triangles at the origin among 200 small spheres spread over +-1e4: the spheres join the far rule's cluster, so
    far_r = 2 x its radius ~ 2e4 and rays that start on a sphere 1e4 away reach the mesh unflagged, with |o| ~ 1e4 in its frame (the mesh's
    own coordinates are ~0.5).  far_origin_set aims such rays at its vertices."""
    local, idx = _patch(0.03, 7)
    sc, _ = _mesh_scene(local.astype(F32), idx, lambda o: o)
    rng = np.random.default_rng(41)
    m = sc.add_material(LambertianMat.with_color((0.5, 0.6, 0.7)))
    for _ in range(200):
        sc.add_object(RenderObject.new(Sphere.new(float(rng.uniform(0.05, 0.1)), m)).position(*rng.uniform(-1e4, 1e4, 3)))
    r = Renderer.default().width(w).height(h).samples(spp).use_bvh(True).camera(_mesh_camera(np.zeros(3), 0.03, 7)).seed(29)
    return sc, r


def far_origin_set(scene, n=64, seed=5):
    """Rays from points beside far objects (not meshes) to nudged vertices of the scene's unplaced meshes: the rays with a large |o| in the
    mesh's frame that still reach it unflagged.  Rows (o, d)."""
    rng = np.random.default_rng(seed)
    meshes = [o.obj for o in scene.render_objects if isinstance(o.obj, TriangleMesh)]
    others = [o for o in scene.render_objects if isinstance(o.obj, Sphere)]
    if not meshes or not others:
        return np.zeros((0, 6), F32)
    v = meshes[0].verts
    rays = []
    for o in rng.choice(len(others), min(n, len(others)), replace=False):
        ob = others[o]
        p = v[int(rng.integers(v.shape[0]))]
        c = ob._position.astype(np.float64)
        u = (p - c) / np.linalg.norm(p - c)
        org = (c + u * 1.5 * ob.obj.radius).astype(F32)          # just outside the sphere, on the side facing the mesh
        for k in NUDGES:
            for sgn in (1, -1):
                q = nudged(p, sgn * rng.choice([-1.0, 1.0], 3), k)
                rays.append(np.concatenate([org, (q.astype(np.float64) - org).astype(F32)]))
    return np.asarray(rays, F32)


def inplane_set(scene, n=512, seed=9):
    """Rays that start exactly ON an axis-aligned rect of the scene (unrotated, unplaced objects) and run inside its plane (the direction's
    component along the normal is +-0): the reference meets that plane at t = 0/0 = NaN, a hit it keeps or replaces by the order of its
    tests.  Directions in steps of 1/16, as scattered directions far from the origin are quantised."""
    rng = np.random.default_rng(seed)
    axes = {XYRect: (0, 1, 2), XZRect: (0, 2, 1), YZRect: (1, 2, 0)}
    rects = [o for o in scene.render_objects if type(o.obj) in axes and o.rotation.s == 1.0 and not np.any(o._position != 0)]
    rays = []
    for k in range(n if rects else 0):
        rc = rects[k % len(rects)].obj
        a, b, c = axes[type(rc)]
        p = np.zeros(3, F32)
        p[a], p[b], p[c] = F32(rng.uniform(rc.a_min, rc.a_max)), F32(rng.uniform(rc.b_min, rc.b_max)), F32(rc.k)
        d = (np.round(rng.normal(size=3) * 16) / 16).astype(F32)
        d[c] = F32(-0.0) if k % 2 else F32(0.0)
        if not d.any():
            d[a] = F32(1.0)
        rays.append(np.concatenate([p, d]))
    return np.asarray(rays, F32).reshape(-1, 6)


# ------------------------------------------------------------------------------------------------ (d) exact rescalings
def base_scene(name, w=48, h=32, spp=4):
    if name == "R2":
        import test_gpu_parity as P
        sc, cam = P._random_scene(2)
        return sc, Renderer.default().width(w).height(h).samples(spp).use_bvh(True).camera(cam).seed(2000006)
    cfg = {"C1": "C1_random_spheres", "C2": "C2_cornell_box", "C3": "C3_suzanne"}[name]
    return scenes.config(cfg, w, h, spp)


def _scale_shape(s, f):
    if isinstance(s, Sphere):
        s.radius = float(F32(s.radius) * f)
    elif isinstance(s, (Cone, Cylinder)):
        s.radius, s.height = float(F32(s.radius) * f), float(F32(s.height) * f)
    elif isinstance(s, Disk):
        s.radius, s.inner_radius = float(F32(s.radius) * f), float(F32(s.inner_radius) * f)
    elif isinstance(s, _AARect):
        for k in ("a_min", "a_max", "b_min", "b_max", "k"):
            setattr(s, k, float(F32(getattr(s, k)) * f))
    elif isinstance(s, Rect3d):
        s.pos, s.size = (s.pos * f).astype(F32), (s.size * f).astype(F32)
    elif isinstance(s, TriangleMesh):
        s.verts = (s.verts * f).astype(F32)
    elif isinstance(s, ConstantMedium):
        _scale_shape(s.obj, f)
        s.density = float(F32(s.density) / f)       # per unit length: the same medium, seen at the new scale
    else:
        raise TypeError(type(s))


def rescaled(name, k, w=48, h=32, spp=4):
    """(d): the base scene with every coordinate, size, position and the camera multiplied by 2^k (exact in float32)."""
    sc, r = base_scene(name, w, h, spp)
    if k == 0:
        return sc, r
    f = F32(2.0 ** k)
    sc, r = copy.deepcopy(sc), copy.deepcopy(r)
    for o in sc.render_objects:
        o._position = (o._position * f).astype(F32)
        _scale_shape(o.obj, f)
    c = r._camera
    c._cam_pos, c._look_at = (c._cam_pos * f).astype(F32), (c._look_at * f).astype(F32)
    c._aperture, c._focus_dist = float(F32(c._aperture) * f), float(F32(c._focus_dist) * f)
    return sc, r


def geometric_floats(sc, r):
    """(kind, value) of every float a rescaling multiplies: 'L' lengths, 'D' densities (per length); the rest of the description as
    'X' (must not change)."""
    out = []

    def shape(s):
        if isinstance(s, Sphere):
            out.append(("L", [s.radius])); out.append(("X", [s.material]))
        elif isinstance(s, (Cone, Cylinder)):
            out.append(("L", [s.radius, s.height])); out.append(("X", [s.material, getattr(s, "max_phi", 0.0)]))
        elif isinstance(s, Disk):
            out.append(("L", [s.radius, s.inner_radius])); out.append(("X", [s.material, s.phi_max]))
        elif isinstance(s, _AARect):
            out.append(("L", [s.a_min, s.a_max, s.b_min, s.b_max, s.k])); out.append(("X", [s.material, float(s.flip_normal)]))
        elif isinstance(s, Rect3d):
            out.append(("L", list(s.pos) + list(s.size))); out.append(("X", [s.material]))
        elif isinstance(s, TriangleMesh):
            out.append(("L", list(s.verts.ravel())))
            out.append(("X", list(s.indicies.astype(np.float64)) + ([] if s.normals is None else list(s.normals.ravel())) + [s.material]))
        elif isinstance(s, ConstantMedium):
            shape(s.obj); out.append(("D", [s.density])); out.append(("X", [s.material]))
    for o in sc.render_objects:
        out.append(("L", list(o._position)))
        out.append(("X", [o.rotation.s, o.rotation.xy, o.rotation.xz, o.rotation.yz, float(o._flip_normals)]))
        shape(o.obj)
    c = r._camera
    out.append(("L", list(c._cam_pos) + list(c._look_at) + [c._aperture, c._focus_dist]))
    out.append(("X", [c._vfov] + [float(v) for k, v in sorted(r.settings.items()) if isinstance(v, (int, float))]))
    return [(kind, np.asarray(v, np.float64)) for kind, v in out]


# ------------------------------------------------------------------------------------------------ the family
def family():
    """(id, builder, modes): every scene of the family with the use_bvh modes its traces run in."""
    out = []
    for c in MESH_CASES:
        out.append((f"a_{c[0]}", lambda c=c: far_mesh(c[0]), (1,)))
    for c in ("origin", "o1e4", "o3e4"):
        out.append((f"b_{c}", lambda c=c: placed_mesh(c, False), (1,)))
        out.append((f"b_{c}_rot", lambda c=c: placed_mesh(c, True), (1,)))
    for c, _ in CLUSTER_CASES:
        out.append((c, lambda c=c: far_cluster(c), (0, 1)))
    out.append(("spread_mesh", spread_mesh, (1,)))
    for b in BASES:
        for k in SCALES:
            out.append((f"d_{b}_2^{k}", lambda b=b, k=k: rescaled(b, k), (0, 1)))
    return out


# ------------------------------------------------------------------------------------------------ rays
def nudged(p, toward, n):
    """p moved n ulps per coordinate in the direction of `toward`'s sign (np.nextafter, coordinate by coordinate; 0 stays)."""
    p = np.asarray(p, F32).copy()
    for _ in range(n):
        p = np.where(toward > 0, np.nextafter(p, F32(np.inf)), np.where(toward < 0, np.nextafter(p, F32(-np.inf)), p)).astype(F32)
    return p


NUDGES = (1, 2, 4, 16)


def grazing_set(scene, renderer, oracle, n_targets=96, seed=3):
    """Rays from origins near the camera aimed at triangle vertices and edge points (and at object box corners), each nudged by
    +-1, 2, 4, 16 ulps across the edge (or in and out of the box's corner).  Rows: (ox, oy, oz, dx, dy, dz); returns (rays, ulps)
    with ulps the signed nudge of each ray (consecutive rows +n, -n)."""
    rng = np.random.default_rng(seed)
    eye = np.asarray(renderer._camera._cam_pos, F32)
    span = max(float(np.abs(np.asarray(renderer._camera._look_at, np.float64) - eye).max()), 1e-30)
    targets, across = [], []
    for o in scene.render_objects:
        s = o.obj
        if not isinstance(s, TriangleMesh):
            continue
        m = np.asarray(oracle.rotor_into_matrix(o.rotation), np.float64)
        world = (s.verts.astype(np.float64) @ m.T + o._position.astype(np.float64)).astype(F32)
        tri = world[s.indicies.reshape(-1, 3)]
        for t in rng.choice(tri.shape[0], min(n_targets, tri.shape[0]), replace=False):
            v = tri[t].astype(np.float64)
            e = int(rng.integers(3))
            a, b, c = v[e], v[(e + 1) % 3], v[(e + 2) % 3]
            nrm = np.cross(b - a, c - a)
            out = np.cross(b - a, nrm)                       # in the plane, perpendicular to the edge a-b, away from c
            if np.dot(out, c - a) > 0:
                out = -out
            sfrac = (0.0, 1.0, float(rng.uniform(0.1, 0.9)))[int(rng.integers(3))]
            targets.append(F32(a + sfrac * (b - a)) if sfrac not in (0.0, 1.0) else (a if sfrac == 0.0 else b).astype(F32))
            across.append(out)
    boxes = oracle.object_aabbs(scene)
    fin = np.isfinite(boxes).all(axis=1) & ((boxes[:, 3:] - boxes[:, :3]).max(axis=1) < 1e3 * max(span, 1.0))
    for i in rng.choice(np.nonzero(fin)[0], min(n_targets, int(fin.sum())), replace=False) if fin.any() else []:
        lo, hi = boxes[i, :3], boxes[i, 3:]
        corner = rng.integers(2, size=3)
        targets.append(np.where(corner == 1, hi, lo).astype(F32))
        across.append(np.where(corner == 1, 1.0, -1.0))
    rays, ulps = [], []
    for p, a in zip(targets, across):
        for n in NUDGES:
            for sgn in (1, -1):
                q = nudged(p, sgn * np.asarray(a), n)
                o = (eye + rng.uniform(-0.02, 0.02, 3) * span).astype(F32)
                d = (q.astype(np.float64) - o.astype(np.float64)).astype(F32)
                rays.append(np.concatenate([o, d]))
                ulps.append(sgn * n)
    rays, ulps = np.asarray(rays, F32), np.asarray(ulps, np.int32)
    keep = (rays[:, 3:] != 0).any(axis=1)
    return rays[keep], ulps[keep]


def camera_ray_set(renderer, oracle, n=1500):
    """Pinhole rays through a lattice of pixel centres (camera.rs: lower_left + s horizontal + t vertical - position), for the guards
    (the GPU tests take the renders' own camera rays from DeviceScene.camera_rays)."""
    w, h = renderer.settings["width"], renderer.settings["height"]
    c = oracle.camera(renderer._camera, w, h)
    ids = np.unique(np.linspace(0, w * h - 1, min(n, w * h)).astype(np.int64))
    s, t = ((ids % w) + 0.5) / w, 1.0 - ((ids // w) + 0.5) / h
    d = c["lower_left"][None] + s[:, None] * c["horizontal"][None] + t[:, None] * c["vertical"][None] - c["position"][None]
    return np.hstack([np.broadcast_to(c["position"], d.shape), d]).astype(F32)


def far_rule(oracle, scene):
    """(far_c, far_r) of the exact walk's flag rule, restated in numpy from the oracle's object boxes (fw_runtime.cpp, DExact): the
    smallest item size (a mesh's: its box extent / sqrt(triangles)), the box of every item up to 16 x that size, far_r = max(256 x
    the smallest size, 2 x the box's half-extent)."""
    boxes = oracle.object_aabbs(scene).astype(F32)
    size = np.zeros(len(scene.render_objects), F32)
    for i, o in enumerate(scene.render_objects):
        b = boxes[i]
        if not np.isfinite(b).all():
            continue
        size[i] = np.abs(b[3:] - b[:3]).max()
        s = o.obj.obj if isinstance(o.obj, ConstantMedium) else o.obj
        if isinstance(s, TriangleMesh):
            size[i] = F32(size[i] / np.sqrt(F32(max(1, s.num_tris()))))
        elif isinstance(s, Disk):                    # its reference box is degenerate: the rule takes the box that encloses it
            size[i] = F32(2.0) * F32(s.radius)
    ok = size > 0
    m = size[ok].min()
    sel = ok & (size <= 16 * m)
    lo = np.minimum(boxes[sel, :3], boxes[sel, 3:]).min(0)
    hi = np.maximum(boxes[sel, :3], boxes[sel, 3:]).max(0)
    c = (lo + hi) * F32(0.5)
    return c.astype(np.float64), float(max(256.0 * m, 2.0 * (hi - c).max()))


def shear(d):
    """max|d| / |d_kz| with kz the SIGNED largest component (fw_kernels.hip: ill_direction)."""
    d = np.asarray(d, np.float64)
    dk = d[np.arange(d.shape[0]), np.argmax(d, axis=1)]
    return np.abs(d).max(axis=1) / np.maximum(np.abs(dk), 1e-300)
