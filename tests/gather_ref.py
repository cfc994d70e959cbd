"""What the final-gather tests share: the scene that holds every material and texture kind, the rays aimed at it, the
reference of a surface record — the CPU oracle's texture and environment lookups at the hit's own (u, v, point) and the float32
statement of normal, distance and kind — a plain-loop restatement of fw_gather_reduce, and synthetic records and probes."""
import numpy as np

from firework_amd import _abi as A
from firework_amd import api
from firework_amd.api import (CheckerTexture, ColorEnv, ConstantTexture, DielectricMat, EmissiveMat, GgxMat, ImageTexture, LambertianMat,
                              MarbleTexture, MetalMat, PerlinNoiseTexture, RenderObject, Scene, SkyEnv, Sphere, TriangleMesh, TurbulenceTexture,
                              XYRect, XZRect)

F32 = np.float32
NO_HIT = A.FW_NO_HIT
TEXTURE_KINDS = ("constant", "checker", "perlin", "turbulence", "marble", "image")


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """bit-equal float32 arrays, any NaN equal to any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (u32(a) == u32(b)) | (np.isnan(a) & np.isnan(b))


# ---- the scene of the surface tests -------------------------------------------------------------------------------------------------
def surface_scene(env, perlin=True, ggx=True):
    """(scene, targets): a row of spheres, one per material and texture kind, a ConstantMedium, a floor, a wall and a tilted quad of two
    triangles without vertex normals (its geometric normal is unnormalised).  targets: (centre, radius to aim within, label).  With
    perlin=False the three Perlin-family textures are constants: the scene stages no permutation table.  ggx=False: the scene's twin
    for the CPU oracle, which has no GgxMat: a MetalMat in its place, so every shape, material index and texture index is the same."""
    rng = np.random.default_rng(3)
    image = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    tex = dict(constant=ConstantTexture.new((0.7, 0.2, 0.1)),
               checker=CheckerTexture.with_colors((0.9, 0.9, 0.1), (0.1, 0.2, 0.8), 3.0),
               perlin=PerlinNoiseTexture.new(2.5) if perlin else ConstantTexture.new((0.3, 0.3, 0.3)),
               turbulence=TurbulenceTexture.new(5, 1.5) if perlin else ConstantTexture.new((0.4, 0.4, 0.4)),
               marble=MarbleTexture.new(4, 2.0) if perlin else ConstantTexture.new((0.5, 0.5, 0.5)),
               image=ImageTexture.new(image))
    scene = Scene.new()
    mats = [(k, LambertianMat.new(tex[k])) for k in TEXTURE_KINDS]
    mats += [("metal", MetalMat.new((0.8, 0.6, 0.2), 0.1)), ("ggx", GgxMat.new((0.95, 0.64, 0.54), 0.3) if ggx else MetalMat.new((0.95, 0.64, 0.54), 0.3)), ("dielectric", DielectricMat.new(1.5)),
             ("emissive", EmissiveMat.with_color((15.0, 12.0, 9.0))),
             ("emissive-checker", EmissiveMat.new(CheckerTexture.with_colors((4.0, 0.5, 0.0), (0.0, 2.5, 7.0), 2.0)))]
    targets = []
    for i, (label, m) in enumerate(mats):
        c = (2.5 * (i - 5), 0.0, 0.0)
        scene.add_object(RenderObject.new(Sphere.new(1.0, scene.add_material(m))).position(*c))
        targets.append((c, 0.8, label))
    grey = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    c = (2.5 * 6, 0.0, 0.0)
    scene.add_volume(RenderObject.new(Sphere.new(1.0, grey)).position(*c), 40.0, tex["checker"])
    targets.append((c, 0.5, "isotropic"))
    scene.add_object(RenderObject.new(XZRect.new(-30.0, 30.0, -8.0, 8.0, -2.0, grey)))                      # a floor
    scene.add_object(RenderObject.new(XYRect.new(-30.0, 30.0, 3.0, 8.0, -4.0, scene.add_material(LambertianMat.new(tex["image"])))))   # a wall
    quad = TriangleMesh.new([[-3.0, 3.0, -2.0], [3.0, 3.0, -2.0], [3.0, 6.5, 0.5], [-3.0, 6.5, 0.5]], [0, 1, 2, 0, 2, 3], None, None, grey)
    scene.add_object(RenderObject.new(quad))
    targets += [((0.0, 4.75, -0.75), 2.0, "mesh"), ((0.0, 5.5, -4.0), 2.0, "wall")]
    scene.set_environment(env)
    return scene, targets


def environments():
    return dict(color=ColorEnv((0.25, 0.5, 3.0)), sky=SkyEnv.new((0.1, 0.3, 2.5), (1.5, 1.0, 0.5)))


def surface_rays(targets, per=7, seed=1):
    """(n, 6) float32: `per` rays at every target from in front (z > 0) and from behind and below (where the rectangles' and the quad's
    stored normals face away from the ray), directions of every length; rays that leave the scene; and rays that are never traced"""
    rng = np.random.default_rng(seed)
    rays = []
    for c, rad, _ in targets:
        c = np.asarray(c)
        for side in (1.0, -1.0):
            for _ in range(per):
                o = c + np.array([rng.uniform(-2, 2), rng.uniform(-1, 3), side * rng.uniform(9, 12)])
                d = (c + rad * rng.uniform(-1, 1, 3) / np.sqrt(3.0) - o) * rng.uniform(0.05, 3.0)
                rays.append(np.concatenate([o, d]))
    for _ in range(2 * per):                                                                   # at the floor from above and from below
        o = np.array([rng.uniform(-20, 20), rng.choice([6.0, -9.0]), rng.uniform(-6, 6)])
        d = np.array([rng.uniform(-0.3, 0.3), -np.sign(o[1] + 2.0), rng.uniform(-0.3, 0.3)]) * rng.uniform(0.5, 2.0)
        rays.append(np.concatenate([o, d]))
    for _ in range(2 * per):                                                                   # away from everything
        rays.append(np.concatenate([rng.uniform(-5, 5, 3) + (0, 20, 0), rng.normal(size=3) * (1, 0.2, 1) + (0, 1.5, 0)]))
    rays = np.array(rays, F32)
    odd = np.array([[0, 0, 5, 0, 0, 0], [0, 0, 5, np.nan, 0, -1], [np.inf, 0, 5, 0, 0, -1], [0, 0, 5, 0, -np.inf, 0], [1, 2, 3, -0.0, 0.0, -0.0]], F32)
    return np.concatenate([rays, odd, rays[:3]])


def traced(rays):
    """the rays fw_trace_rays traces: every component finite and a direction other than (0, 0, 0)"""
    return np.all(np.isfinite(rays), axis=1) & np.any(rays[:, 3:] != 0, axis=1)


def length32(v):
    """sqrt((x x + y y) + z z), every operation rounded to float32"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2], dtype=F32)


def surface_reference(oracle, scene, twin, rays, hits):
    """(n, 16) float32: fw_hit_surface's statement for host rays and the HIT_DTYPE records fw_trace_rays wrote for them on `scene`.
    Texture and environment values are the CPU oracle's, on the scene's twin, at the hit's own (u, v, point) and at d / len(d)."""
    sd, td = scene.to_desc(), twin.to_desc()
    n = rays.shape[0]
    out = np.zeros((n, 16), F32)
    out[:, 3] = -2.0
    ok = traced(rays)
    d = rays[:, 3:]
    dl = length32(d)
    facing = api.surface_facing(hits["normal"], d)
    for i in np.nonzero(ok)[0]:
        h = hits[i]
        if h["object"] == NO_HIT:
            with np.errstate(all="ignore"):
                out[i, 3] = -1.0
                out[i, 12:15] = oracle.env_sample(twin, (d[i] / dl[i]).astype(F32))
            continue
        m = sd.desc.materials[int(h["material"])]
        kind = int(m.kind)
        tex = lambda: oracle.texture_sample(td, int(m.texture), float(h["u"]), float(h["v"]), h["point"])
        if kind in (A.FW_MAT_METAL, A.FW_MAT_GGX):
            out[i, 0:3] = (m.albedo.x, m.albedo.y, m.albedo.z)
        elif kind == A.FW_MAT_DIELECTRIC:
            out[i, 0:3] = 1.0
        elif kind == A.FW_MAT_EMISSIVE:
            out[i, 12:15] = tex()
        else:
            out[i, 0:3] = tex()
        out[i, 3] = kind
        out[i, 4:7] = facing[i]
        out[i, 7] = h["t"] * dl[i]
        out[i, 8:11] = h["point"]
    return out


def texture_kind_of(scene, material):
    """the label of the texture a hit on `material` samples, or None for a material without one"""
    m = scene.materials[material]
    t = getattr(m, "albedo", None) if not hasattr(m, "texture") else m.texture
    names = {ConstantTexture: "constant", CheckerTexture: "checker", PerlinNoiseTexture: "perlin", TurbulenceTexture: "turbulence",
             MarbleTexture: "marble", ImageTexture: "image"}
    return names.get(type(t))


# ---- fw_gather_reduce ---------------------------------------------------------------------------------------------------------------
def reduce_loop(surface, irradiance, D, direct=None):
    """fw_gather_reduce's statement as a plain loop over Python floats (IEEE float64): (n, 4), before the one rounding to float32"""
    s = np.asarray(surface, F32).reshape(-1, D, 16)
    E = np.asarray(irradiance, F32).reshape(-1, D, 3)
    Ed = None if direct is None else np.asarray(direct, F32).reshape(-1, D, 8)
    G = 1
    while G < min(D, 64):
        G *= 2
    inv_pi = 1.0 / 3.141592653589793
    out = np.zeros((s.shape[0], 4))
    for q in range(s.shape[0]):
        part = [[0.0, 0.0, 0.0, 0.0] for _ in range(G)]
        for l in range(G):
            for j in range(l, D, G):
                kind = float(s[q, j, 3])
                if kind == -2.0:
                    continue
                if kind == -1.0 or kind == 3.0:
                    L = [float(s[q, j, 12 + c]) for c in range(3)]
                    if kind == -1.0:
                        part[l][3] = part[l][3] + 1.0
                else:
                    L = []
                    for c in range(3):
                        e = float(E[q, j, c])
                        t = e if e > 0.0 else 0.0
                        if Ed is not None:
                            t = t + float(Ed[q, j, c])
                        L.append((float(s[q, j, c]) * t) * inv_pi)
                for c in range(3):
                    part[l][c] = part[l][c] + L[c]
        m = G // 2
        while m >= 1:
            part = [[part[l][c] + part[l ^ m][c] for c in range(4)] for l in range(G)]
            m //= 2
        out[q] = [(3.141592653589793 / D) * part[0][0], (3.141592653589793 / D) * part[0][1], (3.141592653589793 / D) * part[0][2],
                  (1.0 / D) * part[0][3]]
    return out


def synthetic_records(n, D, rng, unusable=3):
    """(surface (n D, 16), irradiance (n D, 3), direct (n D, 8)) float32: records of every kind mixed, irradiances of both signs (the
    negative ones are clamped), NaN where nothing may be read; the last `unusable` points hold only kind -2 records"""
    total = n * D
    s = rng.uniform(0.0, 1.0, size=(total, 16)).astype(F32)
    kinds = rng.choice(np.array([-2, -1, 0, 1, 2, 3, 4, 5], F32), size=total, p=[0.1, 0.15, 0.25, 0.1, 0.05, 0.15, 0.1, 0.1])
    s[:, 3] = kinds
    s[:, 12:15] = rng.uniform(0.0, 20.0, size=(total, 3)).astype(F32)
    s.reshape(n, D, 16)[n - unusable:, :, 3] = -2.0
    E = rng.uniform(-1.0, 4.0, size=(total, 3)).astype(F32)
    Ed = rng.uniform(0.0, 6.0, size=(total, 8)).astype(F32)
    Ed[:, 3:] = np.nan
    return s, E, Ed


def add_to(prior, acc):
    """sums after one round: float32(prior + float32(acc)), one float32 addition"""
    return (np.asarray(prior, F32) + np.asarray(acc, np.float64).astype(F32)).astype(F32)


# ---- probes -------------------------------------------------------------------------------------------------------------------------
def one_probe(sh0, band1=None):
    """(grid, sh): one probe whose irradiance depends on the normal alone: band 0 = sh0 per channel, optionally the three band-1 terms"""
    grid = api.ProbeGrid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (1, 1, 1))
    sh = np.zeros((1, 9, 3), F32)
    sh[0, 0] = sh0
    if band1 is not None:
        sh[0, 1:4] = band1
    return grid, sh


def random_probes(counts, rng, lo=(-6.0, -3.0, -6.0), hi=(6.0, 7.0, 6.0)):
    grid = api.ProbeGrid(lo, hi, counts)
    sh = rng.uniform(-0.3, 0.3, size=(grid.n_probes, 9, 3)).astype(F32)
    sh[:, 0] = rng.uniform(0.5, 2.0, size=(grid.n_probes, 3)).astype(F32)
    return grid, sh
