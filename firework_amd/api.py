"""Host-side mirror of the reference's scene/renderer API for the render path.

Same names, argument order and error behaviour as the Rust builders so that code written
against ritobanrc/firework reads the same here:

    reference                                         this module
    ------------------------------------------------  ------------------------------------
    Scene::new / add_material / add_object /          Scene (src/scene.rs:19-91)
      add_volume / set_environment
    RenderObject::new(..).position().rotate()         RenderObject (src/scene.rs:270-334)
      .flip_normals()
    Sphere / XYRect / XZRect / YZRect / Rect3d /      src/objects/*.rs
      TriangleMesh / ConstantMedium
    LambertianMat / MetalMat / DielectricMat /        src/material.rs
      EmissiveMat / IsotropicMat
    ConstantTexture / CheckerTexture / Perlin.. /     src/texture.rs
      Turbulence.. / Marble.. / ImageTexture
    ColorEnv / SkyEnv / HdrEnvironment                src/environment.rs, examples/hdri_test.rs:22-82
    CameraSettings                                    src/camera.rs:18-71
    Renderer::default().width()..render(scene)        src/render.rs:59-218

`Renderer.render` flattens the scene into the C ABI of include/firework_hip.h and calls the HIP
library; there is no CPU fallback (a missing library or GPU raises).
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _abi as A

F32 = np.float32


def _v3(v) -> np.ndarray:
    a = np.asarray(v, dtype=F32).reshape(3)
    return a


# --------------------------------------------------------------------------- Rotor3 (ultraviolet)
@dataclass
class Rotor3:
    """ultraviolet::Rotor3 as serialised by src/serde_compat.rs:6-20 (`{s, bv: {xy, xz, yz}}`).

    Pinned by scenes/*.yml: from_rotation_P(t) = {s: cos(t/2), P: -sin(t/2)};
    from_euler_angles(roll, pitch, yaw) = R_xz(yaw) * R_yz(pitch) * R_xy(roll) (geometric product).
    Angles are radians; the reference's examples pass e.g. `-30.` (radians, an example bug kept as written).
    """
    s: float = 1.0
    xy: float = 0.0
    xz: float = 0.0
    yz: float = 0.0

    @staticmethod
    def identity() -> "Rotor3":
        return Rotor3()

    @staticmethod
    def _plane(angle, which) -> "Rotor3":
        # ultraviolet: Rotor3::new(cos(a/2), unit_plane * -sin(a/2)); the products with the two zero
        # plane components keep their sign (teapot.yml holds `xy: -0.0` for from_rotation_xz(90.)).
        half = F32(angle) / F32(2.0)
        ms, c = -F32(math.sin(float(half))), F32(math.cos(float(half)))
        comps = {k: float(F32(1.0 if k == which else 0.0) * ms) for k in ("xy", "xz", "yz")}
        return Rotor3(float(c), comps["xy"], comps["xz"], comps["yz"])

    @staticmethod
    def from_rotation_xy(angle) -> "Rotor3":
        return Rotor3._plane(angle, "xy")

    @staticmethod
    def from_rotation_xz(angle) -> "Rotor3":
        return Rotor3._plane(angle, "xz")

    @staticmethod
    def from_rotation_yz(angle) -> "Rotor3":
        return Rotor3._plane(angle, "yz")

    def __mul__(self, q: "Rotor3") -> "Rotor3":
        """Geometric product of two rotors on the basis (1, e12, e13, e23), in f32 with every sum a fused
        multiply-add chain (ultraviolet builds its products from `mul_add`): the association that reproduces the
        rotor serialised in the reference's scenes/conics.yml BIT FOR BIT (plain f32 sums in any order miss `s` and
        `xz` by one ulp; tests/test_oracle_known_answers.py::test_rotor_constructors_match_reference_yaml)."""
        a, b = self, q

        def fma32(x, y, c):
            """f32 fma(x, y, c) with ONE rounding (std::fma in include/firework.hpp): the product of two f32 is exact in f64, the
            f64 sum is made round-to-odd with the error term of TwoSum, and an odd-rounded f64 rounds to the correct f32."""
            p = float(x) * float(y)
            s_ = p + float(c)
            bb = s_ - p
            err = (p - (s_ - bb)) + (float(c) - bb)
            if err != 0.0 and math.isfinite(s_):
                m = struct.unpack("<q", struct.pack("<d", s_))[0]
                if (m & 1) == 0:                                   # even mantissa and inexact: step to the odd neighbour on the error's side
                    s_ = math.nextafter(s_, math.inf if err > 0 else -math.inf)
            return F32(s_)

        def chain(t0, t1, t2, t3):          # fma(t0, fma(t3, fma(t2, round(t1)))): one rounding per step
            acc = F32(t1[0] * t1[1])
            for x, y in (t2, t3, t0):
                acc = fma32(x, y, acc)
            return float(acc)
        f = lambda x: float(F32(x))
        a_s, a_xy, a_xz, a_yz, b_s, b_xy, b_xz, b_yz = (f(x) for x in (a.s, a.xy, a.xz, a.yz, b.s, b.xy, b.xz, b.yz))
        return Rotor3(
            s=chain((a_s, b_s), (-a_xy, b_xy), (-a_xz, b_xz), (-a_yz, b_yz)),
            xy=chain((a_xy, b_s), (a_s, b_xy), (a_yz, b_xz), (-a_xz, b_yz)),
            xz=chain((a_xz, b_s), (a_s, b_xz), (-a_yz, b_xy), (a_xy, b_yz)),
            yz=chain((a_yz, b_s), (a_s, b_yz), (a_xz, b_xy), (-a_xy, b_xz)),
        )

    @staticmethod
    def from_euler_angles(roll, pitch, yaw) -> "Rotor3":
        return Rotor3.from_rotation_xz(yaw) * Rotor3.from_rotation_yz(pitch) * Rotor3.from_rotation_xy(roll)

    def reversed(self) -> "Rotor3":
        return Rotor3(self.s, -self.xy, -self.xz, -self.yz)

    def to_abi(self) -> A.fw_rotor3:
        return A.fw_rotor3(self.s, self.xy, self.xz, self.yz)


# --------------------------------------------------------------------------- textures
class Texture:
    pass


@dataclass
class ConstantTexture(Texture):
    color: np.ndarray

    def __init__(self, color):
        self.color = _v3(color)

    @staticmethod
    def new(color):
        return ConstantTexture(color)

    @staticmethod
    def from_rgb(r, g, b):
        return ConstantTexture((r, g, b))


@dataclass
class CheckerTexture(Texture):
    odd: Texture
    even: Texture
    scale: float

    @staticmethod
    def new(odd, even, scale):
        return CheckerTexture(odd, even, scale)

    @staticmethod
    def with_colors(odd, even, scale):
        return CheckerTexture(ConstantTexture(odd), ConstantTexture(even), scale)


@dataclass
class PerlinNoiseTexture(Texture):
    scale: float

    @staticmethod
    def new(scale):
        return PerlinNoiseTexture(scale)


@dataclass
class TurbulenceTexture(Texture):
    depth: int
    scale: float

    @staticmethod
    def new(depth, scale):
        return TurbulenceTexture(depth, scale)


@dataclass
class MarbleTexture(Texture):
    depth: int
    scale: float

    @staticmethod
    def new(depth, scale):
        return MarbleTexture(depth, scale)


class ImageTexture(Texture):
    """src/texture.rs:270-310.  `image`: HxWx3 uint8 array, row 0 = top."""

    def __init__(self, image, path: Optional[str] = None):
        img = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
        if img.ndim != 3 or img.shape[2] < 3:
            raise ValueError("ImageTexture expects an HxWx3 uint8 array")
        self.image = np.ascontiguousarray(img[:, :, :3])
        self.path = path

    @staticmethod
    def new(image):
        return ImageTexture(image)

    @staticmethod
    def from_path(path):
        from PIL import Image  # host-side decode only (the reference uses the `image` crate)
        with Image.open(path) as im:
            return ImageTexture(np.asarray(im.convert("RGB")), path=str(path))


# --------------------------------------------------------------------------- materials
class Material:
    pass


@dataclass
class LambertianMat(Material):
    albedo: Texture

    @staticmethod
    def new(albedo: Texture):
        return LambertianMat(albedo)

    @staticmethod
    def with_color(albedo):
        return LambertianMat(ConstantTexture(albedo))


@dataclass
class MetalMat(Material):
    albedo: np.ndarray
    roughness: float

    def __init__(self, albedo, roughness):
        self.albedo = _v3(albedo)
        self.roughness = float(roughness)

    @staticmethod
    def new(albedo, roughness):
        return MetalMat(albedo, roughness)


@dataclass
class GgxMat(Material):
    """An isotropic GGX microfacet conductor (FW_MAT_GGX): albedo = the normal-incidence reflectance F0, every component in
    [0, 1]; roughness in [0.03, 1] (alpha = roughness^2).  Unlike MetalMat its lobe has a density, so point, spot and directional lights
    and, under FW_FLAG_LIGHT_SAMPLING, sphere and rectangle emitters highlight it.  Scene.to_desc checks the ranges."""
    albedo: np.ndarray
    roughness: float

    def __init__(self, albedo, roughness):
        self.albedo = _v3(albedo)
        self.roughness = float(roughness)

    @staticmethod
    def new(albedo, roughness):
        return GgxMat(albedo, roughness)


@dataclass
class DielectricMat(Material):
    ref_idx: float

    @staticmethod
    def new(ref_idx):
        return DielectricMat(ref_idx)


@dataclass
class EmissiveMat(Material):
    albedo: Texture

    @staticmethod
    def new(albedo: Texture):
        return EmissiveMat(albedo)

    @staticmethod
    def with_color(albedo):
        return EmissiveMat(ConstantTexture(albedo))


@dataclass
class IsotropicMat(Material):
    texture: Texture

    @staticmethod
    def new(texture: Texture):
        return IsotropicMat(texture)


# --------------------------------------------------------------------------- shapes
class Shape:
    pass


@dataclass
class Sphere(Shape):
    radius: float
    material: int

    @staticmethod
    def new(radius, material):
        return Sphere(radius, material)


_RADS_PER_DEG = F32(F32(math.pi) / F32(180.0))     # f32::to_radians: self * (PI / 180)


def to_radians(deg) -> float:
    """Rust `f32::to_radians` (the examples write `18_f32.to_radians()`): one f32 multiply by PI/180."""
    return float(F32(deg) * _RADS_PER_DEG)


@dataclass
class Cone(Shape):
    """src/objects/cone.rs:9-25"""
    radius: float
    height: float
    material: int

    @staticmethod
    def new(radius, height, material):
        return Cone(radius, height, material)


@dataclass
class Cylinder(Shape):
    """src/objects/cylinder.rs:10-38 (max_phi in radians)"""
    radius: float
    height: float
    material: int
    max_phi: float = float(F32(360.0) * _RADS_PER_DEG)

    @staticmethod
    def new(radius, height, material):
        return Cylinder(radius, height, material)

    @staticmethod
    def partial(radius, height, phi, material):
        return Cylinder(radius, height, material, float(F32(phi) * _RADS_PER_DEG))


@dataclass
class Disk(Shape):
    """src/objects/disk.rs:10-37 (phi_max in radians)"""
    radius: float
    material: int
    phi_max: float = float(F32(2.0) * F32(math.pi))
    inner_radius: float = 0.0

    @staticmethod
    def new(radius, material):
        return Disk(radius, material)

    @staticmethod
    def partial(radius, phi, inner_radius, material):
        return Disk(radius, material, float(F32(phi) * _RADS_PER_DEG), float(inner_radius))


@dataclass
class _AARect(Shape):
    """AARect<A1,A2>::new(a1_min, a1_max, a2_min, a2_max, k, material) (src/objects/rect.rs:24-39)."""
    a_min: float
    a_max: float
    b_min: float
    b_max: float
    k: float
    material: int
    flip_normal: bool = False
    KIND = -1

    @classmethod
    def new(cls, a_min, a_max, b_min, b_max, k, material):
        return cls(a_min, a_max, b_min, b_max, k, material)


class XYRect(_AARect):
    KIND = A.FW_SHAPE_XYRECT


class XZRect(_AARect):
    KIND = A.FW_SHAPE_XZRECT


class YZRect(_AARect):
    KIND = A.FW_SHAPE_YZRECT


@dataclass
class Rect3d(Shape):
    pos: np.ndarray
    size: np.ndarray
    material: int

    @staticmethod
    def with_size(size, material):
        """src/objects/rect3d.rs:83-85"""
        return Rect3d(np.zeros(3, F32), _v3(size), material)


class TriangleMesh(Shape):
    """src/objects/mesh.rs:12-72"""

    def __init__(self, verts, indicies, normals=None, uvs=None, material=0):
        self.verts = np.ascontiguousarray(np.asarray(verts, dtype=F32).reshape(-1, 3))
        self.indicies = np.ascontiguousarray(np.asarray(indicies, dtype=np.uint32).reshape(-1))
        n = self.verts.shape[0]
        self.normals = None if normals is None else np.ascontiguousarray(np.asarray(normals, dtype=F32).reshape(-1, 3))
        self.uvs = None if uvs is None else np.ascontiguousarray(np.asarray(uvs, dtype=F32).reshape(-1, 2))
        if self.normals is not None and self.normals.shape[0] != n:
            raise ValueError("TriangleMesh::new() -- normals.len() must equal verts.len()")
        if self.uvs is not None and self.uvs.shape[0] != n:
            raise ValueError("TriangleMesh::new() -- uvs.len() must equal verts.len()")
        self.material = int(material)

    @staticmethod
    def new(verts, indicies, normals, uvs, material):
        return TriangleMesh(verts, indicies, normals, uvs, material)

    def translate(self, pos):
        self.verts = self.verts + _v3(pos)[None, :]
        return self

    def num_verts(self):
        return int(self.verts.shape[0])

    def num_tris(self):
        return int(self.indicies.shape[0] // 3)


@dataclass
class ConstantMedium(Shape):
    """src/objects/volume.rs:10-41; built by Scene.add_volume (src/scene.rs:47-62)."""
    obj: Shape
    density: float
    material: int


# --------------------------------------------------------------------------- environments
class Environment:
    pass


@dataclass
class ColorEnv(Environment):
    color: np.ndarray = field(default_factory=lambda: np.zeros(3, F32))

    def __init__(self, color=(0.0, 0.0, 0.0)):
        self.color = _v3(color)

    @staticmethod
    def new(color):
        return ColorEnv(color)


@dataclass
class SkyEnv(Environment):
    zenith_color: np.ndarray
    horizon_color: np.ndarray

    def __init__(self, zenith_color=(0.5, 0.7, 1.0), horizon_color=(1.0, 1.0, 1.0)):
        self.zenith_color = _v3(zenith_color)
        self.horizon_color = _v3(horizon_color)

    @staticmethod
    def new(zenith_color, horizon_color):
        return SkyEnv(zenith_color, horizon_color)

    @staticmethod
    def default():
        return SkyEnv()


class HdrEnvironment(Environment):
    """examples/hdri_test.rs:22-82 (equirect, nearest lookup).  `pixels`: HxWx3 float32, row 0 = top."""

    def __init__(self, pixels):
        p = np.ascontiguousarray(np.asarray(pixels, dtype=F32))
        if p.ndim != 3 or p.shape[2] != 3:
            raise ValueError("HdrEnvironment expects an HxWx3 float32 array")
        self.pixels = p


# --------------------------------------------------------------------------- SunSky
SKY_RG, SKY_RT, SKY_HR, SKY_HM, SKY_G = 6360000.0, 6420000.0, 7994.0, 1200.0, 0.76
SKY_BETA_R = np.array([5.8e-6, 13.5e-6, 33.1e-6])


class SunSky:
    """An analytic sun and sky (fw_sky; include/firework_hip.h has the statement): the sun at `elevation_deg` above the horizon and
    azimuth `azimuth_deg` (panorama_rays' phi), an atmosphere of `turbidity` times the clear Mie load, `sun_irradiance` (rgb) above the
    atmosphere on a plane facing the sun — a linear scale of everything: the exposure — seen from `altitude` metres over ground of
    `ground_albedo`.  view_steps / light_steps / sun_samples are the quadrature's NV, NL and S."""

    def __init__(self, elevation_deg, azimuth_deg, turbidity=1.0, sun_irradiance=(5.0, 5.0, 5.0), sun_radius=0.00465, altitude=1.0,
                 ground_albedo=(0.3, 0.3, 0.3), view_steps=32, light_steps=16, sun_samples=8):
        self.elevation_deg, self.azimuth_deg, self.turbidity = float(elevation_deg), float(azimuth_deg), float(turbidity)
        self.sun_irradiance, self.sun_radius, self.altitude = _v3(sun_irradiance), float(sun_radius), float(altitude)
        self.ground_albedo = _v3(ground_albedo)
        self.view_steps, self.light_steps, self.sun_samples = int(view_steps), int(light_steps), int(sun_samples)

    def check(self):
        """what fw_check_sky rejects in a description, as a ValueError, in its order"""
        f = np.float32
        if not -f(np.pi / 2) <= f(np.radians(self.elevation_deg)) <= f(np.pi / 2):
            raise ValueError("elevation_deg must be in [-90, 90]")
        if not np.isfinite(f(np.radians(self.azimuth_deg))):
            raise ValueError("azimuth_deg must be finite")
        if not 0.0 <= f(self.turbidity) <= 64.0:
            raise ValueError("turbidity must be in [0, 64]")
        if not (np.all(np.isfinite(self.sun_irradiance)) and np.all(self.sun_irradiance >= 0)):
            raise ValueError("sun_irradiance must be finite and >= 0")
        if not 0.0 < f(self.sun_radius) <= f(0.1):
            raise ValueError("sun_radius must be in (0, 0.1]")
        if not 1.0 <= f(self.altitude) <= 50000.0:
            raise ValueError("altitude must be in [1, 50000]")
        if not (np.all(self.ground_albedo >= 0) and np.all(self.ground_albedo <= 1)):
            raise ValueError("ground_albedo must be in [0, 1]")
        if not 1 <= self.view_steps <= 64:
            raise ValueError("view_steps must be in 1..64")
        if not 1 <= self.light_steps <= 32:
            raise ValueError("light_steps must be in 1..32")
        if not 1 <= self.sun_samples <= 16:
            raise ValueError("sun_samples must be in 1..16")
        return self

    def to_abi(self, disc: bool = False) -> A.fw_sky:
        self.check()
        s = A.fw_sky()
        s.sun_elevation, s.sun_azimuth, s.turbidity = np.radians(self.elevation_deg), np.radians(self.azimuth_deg), self.turbidity
        s.sun_irradiance, s.sun_radius, s.altitude, s.ground_albedo = A.vec3(self.sun_irradiance), self.sun_radius, self.altitude, A.vec3(self.ground_albedo)
        s.view_steps, s.light_steps, s.sun_samples, s.flags = self.view_steps, self.light_steps, self.sun_samples, A.FW_SKY_DISC if disc else 0
        return s

    def sun_direction(self) -> np.ndarray:
        """s, the unit direction towards the sun, float64 from the float32 angles"""
        return _sky_constants(self)["s"]

    def sun_light(self) -> "DirectionalLight":
        """the sun as a DirectionalLight of the disc's energy: direction -s, irradiance E0 T(O) (api.sky_sun)"""
        direction, irradiance = sky_sun(self)
        return DirectionalLight(direction, irradiance)


def _sky_constants(sky) -> dict:
    """fw_sky's fields widened to float64 and what the host derives from them (fw_runtime.cpp: sky_device)"""
    a = sky if isinstance(sky, A.fw_sky) else sky.to_abi()
    el, az = np.float64(a.sun_elevation), np.float64(a.sun_azimuth)
    ce = np.cos(el)
    k = dict(s=np.array([ce * np.cos(az), np.sin(el), ce * np.sin(az)]), oy=SKY_RG + np.float64(a.altitude), beta_m=21e-6 * np.float64(a.turbidity),
             e0=np.array([a.sun_irradiance.x, a.sun_irradiance.y, a.sun_irradiance.z], np.float64),
             albedo_pi=np.array([a.ground_albedo.x, a.ground_albedo.y, a.ground_albedo.z], np.float64) / np.pi,
             cos_sr=np.cos(np.float64(a.sun_radius)), radius=np.float64(a.sun_radius), el=el, nv=int(a.view_steps), nl=int(a.light_steps),
             ss=int(a.sun_samples), flags=int(a.flags))
    k["beta_me"] = 1.1 * k["beta_m"]
    k["O"] = np.array([0.0, k["oy"], 0.0])
    return k


def _sky_ground(P, w):
    """(meets the ground, b, disc, |disc| / P.P where b < 0 else inf: how far the decision is from its threshold)"""
    b = _dot3(P, w)
    pp = _dot3(P, P)
    disc = b * b - (pp - SKY_RG * SKY_RG)
    return (b < 0.0) & (disc > 0.0), b, disc, np.where(b < 0.0, np.abs(disc) / pp, np.inf)


def _sky_depth(P, w, n: int):
    """D(P, w, N): (dR, dM), P (..., 3), w (3,)"""
    b = _dot3(P, w)
    tl = -b + np.sqrt(b * b - (_dot3(P, P) - SKY_RT * SKY_RT))
    dr, dm = np.zeros_like(tl), np.zeros_like(tl)
    nd, nn = np.float64(n), np.float64(n * n)
    for k in range(n):
        f = (np.float64(k) + 0.5) / nd
        t, wd = tl * (f * f), tl * (np.float64(2 * k + 1) / nn)
        Q = P + t[..., None] * w
        h = np.sqrt(_dot3(Q, Q)) - SKY_RG
        dr = dr + np.exp(-h / SKY_HR) * wd
        dm = dm + np.exp(-h / SKY_HM) * wd
    return dr, dm


def _sky_transmittance(k, P):
    """T(P) (..., 3) and the ground decision's margin"""
    shadow, _, _, margin = _sky_ground(P, k["s"])
    lr, lm = _sky_depth(P, k["s"], k["nl"])
    T = np.exp(-(SKY_BETA_R * lr[..., None] + (k["beta_me"] * lm)[..., None]))
    return np.where(shadow[..., None], 0.0, T), margin


def _sky_along(k, d, terms=None):
    """the radiance (n, 3) float64 along unit directions d (n, 3) float64, without the disc.  terms: a dict that receives `margin` (the
    smallest |disc| / P.P of the ground decisions made with b < 0), `tau_max` (the largest optical depth of an unshadowed sample) and,
    per direction, `scatter` (n, 3), `ground_nocos` (n, 3: the ground's term without its cosine) and `t_max` (n,): what
    tests/sky_ref.py's bound is made of"""
    O, s, nv = k["O"], k["s"], k["nv"]
    n = d.shape[0]
    Ob = np.broadcast_to(O, d.shape)
    hit, bo, dg, margin = _sky_ground(Ob, d) if n else (np.zeros(0, bool), np.zeros(0), np.zeros(0), np.zeros(0))
    tmax = -bo + np.sqrt(bo * bo - (_dot3(O, O) - SKY_RT * SKY_RT))
    with np.errstate(invalid="ignore"):
        tmax = np.where(hit, -bo - np.sqrt(dg), tmax)
    nd, nn = np.float64(nv), np.float64(nv * nv)
    o_r, o_m = np.zeros(n), np.zeros(n)
    sr, sm = np.zeros((n, 3)), np.zeros((n, 3))
    low, tau_max = (np.min(margin) if n else np.inf), 0.0
    for i in range(nv):
        f = (np.float64(i) + 0.5) / nd
        t, wd = tmax * (f * f), tmax * (np.float64(2 * i + 1) / nn)
        P = O + t[:, None] * d
        h = np.sqrt(_dot3(P, P)) - SKY_RG
        hr, hm = np.exp(-h / SKY_HR) * wd, np.exp(-h / SKY_HM) * wd
        shadow, _, _, m = _sky_ground(P, s)
        lr, lm = _sky_depth(P, s, k["nl"])
        ar, am = (o_r + 0.5 * hr) + lr, (o_m + 0.5 * hm) + lm
        tau = SKY_BETA_R * ar[:, None] + (k["beta_me"] * am)[:, None]
        att = np.where(shadow[:, None], 0.0, np.exp(-tau))
        sr, sm = sr + att * hr[:, None], sm + att * hm[:, None]
        o_r, o_m = o_r + hr, o_m + hm
        if n:
            low = min(low, np.min(m))
            if not np.all(shadow):
                tau_max = max(tau_max, float(np.max(tau[~shadow])))
    mu = _dot3(d, s)
    m1 = 1.0 + mu * mu
    p_r = (3.0 / (16.0 * np.pi)) * m1
    x = (1.0 + SKY_G * SKY_G) - (2.0 * SKY_G) * mu
    p_m = ((3.0 / (8.0 * np.pi)) * ((1.0 - SKY_G * SKY_G) * m1)) / ((2.0 + SKY_G * SKY_G) * (x * np.sqrt(x)))
    L = k["e0"] * ((sr * SKY_BETA_R) * p_r[:, None] + (sm * k["beta_m"]) * p_m[:, None])
    scatter, ground_nocos = L.copy(), np.zeros((n, 3))
    if np.any(hit):
        q = np.nonzero(hit)[0]
        G = O + tmax[q, None] * d[q]
        gl = np.sqrt(_dot3(G, G))
        cg = np.maximum(_dot3(G / gl[:, None], s), 0.0)
        T, _ = _sky_transmittance(k, G)
        through = np.exp(-(SKY_BETA_R * o_r[q, None] + (k["beta_me"] * o_m[q])[:, None]))
        L[q] = L[q] + (((through * k["albedo_pi"]) * k["e0"]) * T) * cg[:, None]
        ground_nocos[q] = np.where(cg[:, None] > 0.0, ((through * k["albedo_pi"]) * k["e0"]) * T, 0.0)
        if q.size:
            tau_max = max(tau_max, float(np.max(SKY_BETA_R * o_r[q, None] + (k["beta_me"] * o_m[q])[:, None])))
    if terms is not None:
        terms["margin"] = min(terms.get("margin", np.inf), float(low))
        terms["tau_max"] = max(terms.get("tau_max", 0.0), tau_max)
        terms["scatter"], terms["ground_nocos"], terms["t_max"] = scatter, ground_nocos, tmax
    return L


def sky_sun(sky):
    """The numpy statement of fw_sky_sun: (direction -s, irradiance E0 T(O)) of the sun as a directional light, float32 (3,) each"""
    k = _sky_constants(sky)
    T, _ = _sky_transmittance(k, k["O"])
    return (-k["s"]).astype(np.float32), (k["e0"] * T).astype(np.float32)


def sky_radiance(sky, dirs, disc: bool = None, terms: dict = None) -> np.ndarray:
    """The numpy statement of fw_sky_radiance: (n, 3) float32 along directions of any length (n, 3); zeros for a zero or non-finite
    direction.  disc: draw the sun (None: as the fw_sky's flags say, False for an api.SunSky).  terms as _sky_along's, plus `edge`: the
    smallest |d . s - cos(sun_radius)|."""
    k = _sky_constants(sky)
    disc = bool(k["flags"] & A.FW_SKY_DISC) if disc is None else disc
    r = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l2 = _dot3(r, r)
        ok = (l2 > 0.0) & np.isfinite(l2)
        d = r[ok] / np.sqrt(l2[ok])[:, None]
    L = _sky_along(k, d, terms)
    if terms is not None:
        terms["ok"] = ok
    if disc:
        T, _ = _sky_transmittance(k, k["O"])
        mu = _dot3(d, k["s"])
        L = L + np.where((mu >= k["cos_sr"])[:, None], (k["e0"] * T) / ((2.0 * np.pi) * (1.0 - k["cos_sr"])), 0.0)
        if terms is not None and mu.size:
            terms["edge"] = min(terms.get("edge", np.inf), float(np.min(np.abs(mu - k["cos_sr"]))))
    out = np.zeros((r.shape[0], 3), np.float32)
    out[ok] = L.astype(np.float32)
    return out


def _sky_map_dirs(xf, jf, w: int, h: int) -> np.ndarray:
    """panorama_rays' direction of the map points (x + fx, j + fy), float64"""
    u, v = xf / np.float64(w), 1.0 - jf / np.float64(h)
    phi, theta = np.pi - (2.0 * np.pi) * u, np.pi * v - np.pi / 2.0
    ct = np.cos(theta)
    return np.stack([ct * np.cos(phi), np.sin(theta), ct * np.sin(phi)], axis=-1)


def sky_omega_row(w: int, h: int) -> np.ndarray:
    """Omega_j: the solid angle of one texel of each row (h,)"""
    y = np.arange(h, dtype=np.float64)
    return ((2.0 * np.pi) / np.float64(w)) * (np.cos((y * np.pi) / np.float64(h)) - np.cos(((y + 1.0) * np.pi) / np.float64(h)))


def sky_env_texel(s, w: int, h: int) -> int:
    """the texel the FW_ENV_HDR lookup reads for the direction s: env_sample's float32 arithmetic"""
    f = np.float32
    d = np.asarray(s, np.float64).astype(f)
    phi, theta = np.arctan2(d[2], d[0]).astype(f), np.arcsin(np.clip(d[1], f(-1), f(1))).astype(f)
    u = f(1) - (phi + f(np.pi)) / f(2 * np.pi)
    v = (theta + f(np.pi / 2)) / f(np.pi)
    x, y = np.floor(np.maximum(u * f(w), f(0))), np.floor(np.maximum((f(1) - v) * f(h), f(0)))
    idx = np.floor(np.float64(f(y) * f(w))) + np.float64(x)
    return int(min(idx, w * h - 1))


def sky_disc(sky, width: int, height: int, terms: dict = None):
    """The disc's share of a map: (ids, gain) — the flat texel ids it covers and E0 T(O) c_t / A (n, 3) float64 for each — and A.  Empty
    where the sun is below the observer's horizon.  terms receives `edge`: the smallest |d . s - cos(sun_radius)| of a sample."""
    k = _sky_constants(sky)
    w, h, S = int(width), int(height), k["ss"]
    T, _ = _sky_transmittance(k, k["O"])
    if _sky_ground(k["O"], k["s"])[0]:
        return np.zeros(0, np.int64), np.zeros((0, 3)), 0.0
    et = k["e0"] * T
    # rows farther than sun_radius from the sun's latitude hold no sample (a latitude difference is at most the angle): their n_t is 0
    theta_edge = np.pi * (1.0 - np.arange(h + 1) / h) - np.pi / 2
    rows = np.nonzero((theta_edge[:-1] >= k["el"] - k["radius"] - 1e-9) & (theta_edge[1:] <= k["el"] + k["radius"] + 1e-9))[0]
    off = (np.arange(S, dtype=np.float64) + 0.5) / np.float64(S)
    x = np.arange(w, dtype=np.float64)
    counts = np.zeros((h, w), np.int64)
    for j in rows:
        xf = (x[:, None, None] + off[None, None, :]) + np.zeros((1, S, 1))
        jf = (np.float64(j) + off[None, :, None]) + np.zeros((w, 1, S))
        mu = _dot3(_sky_map_dirs(xf, jf, w, h), k["s"])
        counts[j] = np.sum(mu >= k["cos_sr"], axis=(1, 2))
        if terms is not None:
            terms["edge"] = min(terms.get("edge", np.inf), float(np.min(np.abs(mu - k["cos_sr"]))))
    omega = sky_omega_row(w, h)
    s2 = np.float64(S * S)
    A_ = np.float64(0.0)
    for j in range(h):
        A_ = A_ + (np.float64(counts[j].sum()) / s2) * omega[j]
    if A_ == 0.0:
        t = sky_env_texel(k["s"], w, h)
        return np.array([t], np.int64), ((et * 1.0) / omega[t // w])[None, :], float(omega[t // w])
    ids = np.nonzero(counts.reshape(-1))[0]
    c = counts.reshape(-1)[ids] / s2
    return ids, (et[None, :] * c[:, None]) / A_, float(A_)


def sky_map(sky, width: int, height: int, disc: bool = None, texels=None, terms: dict = None) -> np.ndarray:
    """The numpy statement of fw_sky_map: (height, width, 3) float32, row 0 at the top.  disc as sky_radiance's.  texels: flat texel
    ids to evaluate instead of the whole map -> (n, 3).  terms as _sky_along's and sky_disc's."""
    k = _sky_constants(sky)
    w, h = int(width), int(height)
    if w < 2 or h < 2:
        raise ValueError("width and height must be >= 2")
    disc = bool(k["flags"] & A.FW_SKY_DISC) if disc is None else disc
    ids = np.arange(w * h, dtype=np.int64) if texels is None else np.asarray(texels, np.int64).reshape(-1)
    j, x = np.divmod(ids, w)
    L = _sky_along(k, _sky_map_dirs(x + 0.5, j + 0.5, w, h), terms)
    if terms is not None:
        terms["radiance"] = L.copy()                            # float64, before the disc
    if disc:
        covered, gain, _ = sky_disc(sky, w, h, terms)
        pos = {int(t): i for i, t in enumerate(ids)}
        for t, g in zip(covered, gain):
            if int(t) in pos:
                L[pos[int(t)]] = L[pos[int(t)]] + g
    out = L.astype(np.float32)
    return out.reshape(h, w, 3) if texels is None else out


class SunSkyEnv(Environment):
    """A SunSky as a scene's environment: its width x height map, baked on the GPU (_lib.sky_map) when the scene's descriptor is built
    and passed as FW_ENV_HDR.  sun: "disc" draws the sun into the map (for FW_FLAG_ENV_SAMPLING to find), "light" leaves it out and adds
    sky.sun_light() to the scene's lights (a delta sun: sharp shadows through next-event estimation and fw_bake_direct), "none" neither."""
    SUNS = ("disc", "light", "none")

    def __init__(self, sky: SunSky, width: int = 2048, height: int = 1024, sun: str = "disc"):
        if sun not in self.SUNS:
            raise ValueError('sun must be "disc", "light" or "none"')
        if int(width) < 2 or int(height) < 2:
            raise ValueError("width and height must be >= 2")
        self.sky, self.width, self.height, self.sun = sky.check(), int(width), int(height), sun

    def bake(self, device: int = 0) -> np.ndarray:
        """the (height, width, 3) float32 map; raises _lib's no-device error without a GPU"""
        from . import _lib
        return _lib.sky_map(self.sky.to_abi(disc=self.sun == "disc"), self.width, self.height, device=device)


# --------------------------------------------------------------------------- RenderObject / Scene
class RenderObject:
    """src/scene.rs:270-334"""

    def __init__(self, obj: Shape):
        self.obj = obj
        self._position = np.zeros(3, F32)
        self.rotation = Rotor3.identity()
        self._flip_normals = False

    @staticmethod
    def new(obj: Shape):
        return RenderObject(obj)

    def position(self, x, y, z):
        self._position = _v3((x, y, z))
        return self

    def position_vec(self, pos):
        self._position = _v3(pos)
        return self

    def rotate(self, rotor: Rotor3):
        self.rotation = rotor
        return self

    def flip_normals(self):
        self._flip_normals = not self._flip_normals
        return self


# --------------------------------------------------------------------------- lights without area
class Light:
    """A point, spot or directional light: found by next-event estimation alone (no path can hit it), so it lights Lambertian and
    Isotropic surfaces of a resident scene and nothing else.  The reference has none."""


class PointLight(Light):
    """Radiant intensity `intensity` (rgb, per steradian) from `position`, the same in every direction."""

    def __init__(self, position, intensity):
        self.position, self.intensity = _v3(position), _v3(intensity)

    def to_abi(self) -> A.fw_light:
        return A.fw_light(A.FW_LIGHT_POINT, A.vec3(self.position), A.vec3((0, 0, 0)), A.vec3(self.intensity), 0.0, 0.0)


class SpotLight(Light):
    """A point light that shines along `direction`: full intensity within `inner_deg` of the axis, none beyond `outer_deg`, a
    smoothstep of the cosine between (0 <= inner_deg <= outer_deg <= 180)."""

    def __init__(self, position, direction, intensity, inner_deg, outer_deg):
        self.position, self.direction, self.intensity = _v3(position), _v3(direction), _v3(intensity)
        self.inner_deg, self.outer_deg = float(inner_deg), float(outer_deg)

    def to_abi(self) -> A.fw_light:
        ci, co = np.cos(np.radians(self.inner_deg)), np.cos(np.radians(self.outer_deg))
        return A.fw_light(A.FW_LIGHT_SPOT, A.vec3(self.position), A.vec3(self.direction), A.vec3(self.intensity), float(ci), float(co))


class DirectionalLight(Light):
    """Parallel light travelling along `direction` (any length), `irradiance` (rgb) on a plane that faces it."""

    def __init__(self, direction, irradiance):
        self.direction, self.irradiance = _v3(direction), _v3(irradiance)

    def to_abi(self) -> A.fw_light:
        return A.fw_light(A.FW_LIGHT_DIRECTIONAL, A.vec3((0, 0, 0)), A.vec3(self.direction), A.vec3(self.irradiance), 0.0, 0.0)


class Scene:
    """src/scene.rs:19-91"""

    def __init__(self):
        self.render_objects: List[RenderObject] = []
        self.materials: List[Material] = []
        self.lights: List[Light] = []               # point, spot and directional lights: not part of fw_scene_desc
        self.environment: Environment = ColorEnv()  # Scene::new(): black ColorEnv (scene.rs:36)

    @staticmethod
    def new():
        return Scene()

    def add_object(self, obj: RenderObject) -> int:
        self.render_objects.append(obj)
        return len(self.render_objects) - 1

    def add_volume(self, obj: RenderObject, density, texture: Texture) -> int:
        mat = self.add_material(IsotropicMat(texture))
        obj.obj = ConstantMedium(obj.obj, float(density), mat)
        return self.add_object(obj)

    def get_object(self, idx):
        return self.render_objects[idx]

    def add_material(self, mat: Material) -> int:
        self.materials.append(mat)
        return len(self.materials) - 1

    def add_light(self, light: Light) -> int:
        """Adds a PointLight, SpotLight or DirectionalLight.  Resident scenes (DeviceScene and every Renderer call that makes one, render
        and render_full of a lit scene included) render with them; the tiled multi-GPU path, which passes a bare description, does not."""
        if not isinstance(light, Light):
            raise TypeError(f"not a light: {type(light).__name__}")
        self.lights.append(light)
        return len(self.lights) - 1

    def get_material(self, idx):
        return self.materials[idx]

    def set_environment(self, env: Environment):
        """A SunSkyEnv with sun="light" brings its sun: sky.sun_light() joins self.lights, and leaves with the environment that brought it."""
        brought = getattr(self, "_sky_light", None)
        self.lights = [l for l in self.lights if l is not brought]
        self._sky_light = None
        if isinstance(env, SunSkyEnv) and env.sun == "light":
            self._sky_light = env.sky.sun_light()
            self.lights.append(self._sky_light)
        self.environment = env

    # ---- flatten to the C ABI -------------------------------------------------
    def to_desc(self) -> "SceneDesc":
        return SceneDesc(self)


def _object_record(fo, ro: RenderObject, shape: int):
    """Fills the fw_object `fo` with RenderObject `ro`'s placement and shape index `shape`; returns it."""
    fo.shape = shape
    fo.position = A.vec3(ro._position)
    fo.rotation = ro.rotation.to_abi()
    fo.flip_normals = int(ro._flip_normals)
    return fo


class SceneDesc:
    """Owns the ctypes arrays (and the numpy buffers they point into) of one fw_scene_desc."""

    def __init__(self, scene: Scene):
        self._keep = []
        texs: List[A.fw_texture] = []

        def add_tex(t: Texture) -> int:
            ft = A.fw_texture()
            if isinstance(t, ConstantTexture):
                ft.kind = A.FW_TEX_CONSTANT
                ft.color = A.vec3(t.color)
            elif isinstance(t, CheckerTexture):
                ft.kind = A.FW_TEX_CHECKER
                ft.scale = t.scale
                ft.odd = add_tex(t.odd)
                ft.even = add_tex(t.even)
            elif isinstance(t, PerlinNoiseTexture):
                ft.kind = A.FW_TEX_PERLIN
                ft.scale = t.scale
            elif isinstance(t, TurbulenceTexture):
                ft.kind = A.FW_TEX_TURBULENCE
                ft.scale = t.scale
                ft.depth = t.depth
            elif isinstance(t, MarbleTexture):
                ft.kind = A.FW_TEX_MARBLE
                ft.scale = t.scale
                ft.depth = t.depth
            elif isinstance(t, ImageTexture):
                ft.kind = A.FW_TEX_IMAGE
                ft.img_h, ft.img_w = t.image.shape[0], t.image.shape[1]
                ft.img_rgb8 = t.image.ctypes.data_as(C.POINTER(C.c_uint8))
                self._keep.append(t.image)
            else:
                raise TypeError(f"unknown texture {type(t).__name__}")
            texs.append(ft)
            return len(texs) - 1

        mats = []
        for m in scene.materials:
            fm = A.fw_material()
            fm.texture = -1
            if isinstance(m, LambertianMat):
                fm.kind = A.FW_MAT_LAMBERTIAN
                fm.texture = add_tex(m.albedo)
            elif isinstance(m, MetalMat):
                fm.kind = A.FW_MAT_METAL
                fm.albedo = A.vec3(m.albedo)
                fm.roughness = m.roughness
            elif isinstance(m, GgxMat):
                i = len(mats)          # (the library's checks and wording: fw_scene_create would refuse the same)
                if not (np.float32(0.03) <= np.float32(m.roughness) <= np.float32(1.0)):
                    raise ValueError(f"material {i}: GgxMat roughness must be in [0.03, 1]")
                if not all(0.0 <= float(c) <= 1.0 for c in np.asarray(m.albedo, dtype=np.float32)):
                    raise ValueError(f"material {i}: GgxMat albedo components must be in [0, 1]")
                fm.kind = A.FW_MAT_GGX
                fm.albedo = A.vec3(m.albedo)
                fm.roughness = m.roughness
            elif isinstance(m, DielectricMat):
                fm.kind = A.FW_MAT_DIELECTRIC
                fm.ref_idx = m.ref_idx
            elif isinstance(m, EmissiveMat):
                fm.kind = A.FW_MAT_EMISSIVE
                fm.texture = add_tex(m.albedo)
            elif isinstance(m, IsotropicMat):
                fm.kind = A.FW_MAT_ISOTROPIC
                fm.texture = add_tex(m.texture)
            else:
                raise TypeError(f"unknown material {type(m).__name__}")
            mats.append(fm)

        shapes: List[A.fw_shape] = []
        self._shape_objs = []  # the Python shape object of each fw_shape (kept: placements() maps objects to shapes by identity)

        shape_index = {}      # one fw_shape per Python shape object: objects that share a TriangleMesh share its BLAS

        def add_shape(s: Shape) -> int:
            if id(s) in shape_index:
                return shape_index[id(s)]
            fs = A.fw_shape()
            fs.inner = -1
            if isinstance(s, Sphere):
                fs.kind, fs.radius, fs.material = A.FW_SHAPE_SPHERE, s.radius, s.material
            elif isinstance(s, Cone):
                fs.kind, fs.material, fs.radius, fs.height = A.FW_SHAPE_CONE, s.material, s.radius, s.height
            elif isinstance(s, Cylinder):
                fs.kind, fs.material, fs.radius, fs.height, fs.phi_max = A.FW_SHAPE_CYLINDER, s.material, s.radius, s.height, s.max_phi
            elif isinstance(s, Disk):
                fs.kind, fs.material, fs.radius, fs.phi_max, fs.inner_radius = A.FW_SHAPE_DISK, s.material, s.radius, s.phi_max, s.inner_radius
            elif isinstance(s, _AARect):
                fs.kind, fs.material = s.KIND, s.material
                fs.a_min, fs.a_max, fs.b_min, fs.b_max, fs.k = s.a_min, s.a_max, s.b_min, s.b_max, s.k
                fs.flip_normal = int(bool(s.flip_normal))
            elif isinstance(s, Rect3d):
                fs.kind, fs.material = A.FW_SHAPE_RECT3D, s.material
                fs.pos, fs.size = A.vec3(s.pos), A.vec3(s.size)
            elif isinstance(s, TriangleMesh):
                fs.kind, fs.material = A.FW_SHAPE_TRIANGLE_MESH, s.material
                fs.verts = s.verts.ctypes.data_as(C.POINTER(C.c_float))
                fs.n_verts = s.verts.shape[0]
                fs.indices = s.indicies.ctypes.data_as(C.POINTER(C.c_uint32))
                fs.n_indices = s.indicies.shape[0]
                self._keep += [s.verts, s.indicies]
                if s.normals is not None:
                    fs.normals = s.normals.ctypes.data_as(C.POINTER(C.c_float))
                    self._keep.append(s.normals)
                if s.uvs is not None:
                    fs.uvs = s.uvs.ctypes.data_as(C.POINTER(C.c_float))
                    self._keep.append(s.uvs)
            elif isinstance(s, ConstantMedium):
                fs.kind, fs.material, fs.density = A.FW_SHAPE_CONSTANT_MEDIUM, s.material, s.density
                fs.inner = add_shape(s.obj)
            else:
                raise TypeError(f"unknown shape {type(s).__name__}")
            shapes.append(fs)
            self._shape_objs.append(s)
            shape_index[id(s)] = len(shapes) - 1
            return len(shapes) - 1

        objs = [_object_record(A.fw_object(), ro, add_shape(ro.obj)) for ro in scene.render_objects]

        env = A.fw_environment()
        e = scene.environment
        if isinstance(e, ColorEnv):
            env.kind, env.color = A.FW_ENV_COLOR, A.vec3(e.color)
        elif isinstance(e, SkyEnv):
            env.kind, env.zenith, env.horizon = A.FW_ENV_SKY, A.vec3(e.zenith_color), A.vec3(e.horizon_color)
        elif isinstance(e, HdrEnvironment):
            env.kind = A.FW_ENV_HDR
            env.hdr_h, env.hdr_w = e.pixels.shape[0], e.pixels.shape[1]
            env.hdr_rgb = e.pixels.ctypes.data_as(C.POINTER(C.c_float))
            self._keep.append(e.pixels)
        elif isinstance(e, SunSkyEnv):
            pixels = e.bake()                                   # on the GPU, once per description; no device: _lib's error
            env.kind = A.FW_ENV_HDR
            env.hdr_h, env.hdr_w = pixels.shape[0], pixels.shape[1]
            env.hdr_rgb = pixels.ctypes.data_as(C.POINTER(C.c_float))
            self._keep.append(pixels)
        else:
            raise TypeError(f"unknown environment {type(e).__name__}")

        def arr(ctype, items):
            a = (ctype * max(1, len(items)))(*items)
            self._keep.append(a)
            return a

        self.objects, self.shapes = arr(A.fw_object, objs), arr(A.fw_shape, shapes)
        self.materials, self.textures = arr(A.fw_material, mats), arr(A.fw_texture, texs)
        d = A.fw_scene_desc()
        d.objects, d.n_objects = self.objects, len(objs)
        d.shapes, d.n_shapes = self.shapes, len(shapes)
        d.materials, d.n_materials = self.materials, len(mats)
        d.textures, d.n_textures = self.textures, len(texs)
        d.environment = env
        self.desc = d
        # the lights travel beside the description (fw_scene_set_lights): DeviceScene sets them after it created the scene
        self.lights = [l.to_abi() for l in getattr(scene, "lights", [])]

    def ptr(self):
        return C.byref(self.desc)

    def placements(self, scene: Scene) -> "SceneDesc":
        """The description of `scene`, the Scene this one was made from, after its RenderObjects were moved (position, rotation,
        flip_normals): a new fw_object array, and this description's shape, material and texture arrays and environment as they are
        (what DeviceScene.update passes to fw_scene_update).  ValueError if the scene's objects no longer map to the same shapes, by
        identity as SceneDesc maps them."""
        ros = scene.render_objects
        if len(ros) != self.desc.n_objects:
            raise ValueError(f"the scene has {len(ros)} objects, its description {self.desc.n_objects}")
        index = {id(s): i for i, s in enumerate(self._shape_objs)}
        objs = (A.fw_object * max(1, len(ros)))()
        for i, ro in enumerate(ros):
            si = index.get(id(ro.obj))
            if si is None or si != self.objects[i].shape:
                raise ValueError(f"object {i} no longer uses the shape it was created with (only placements may change)")
            _object_record(objs[i], ro, si)
        # the buffers of the description the chain started from, and this object array: a placements() of a placements() holds the
        # same number of buffers, however long the chain (DeviceScene.update keeps the latest description)
        base_keep = getattr(self, "_base_keep", self._keep)
        out = SceneDesc.__new__(SceneDesc)
        out._base_keep = base_keep
        out._keep = base_keep + [objs]
        out._shape_objs = self._shape_objs
        out.objects, out.shapes, out.materials, out.textures = objs, self.shapes, self.materials, self.textures
        d = A.fw_scene_desc()
        d.objects, d.n_objects = objs, len(ros)
        d.shapes, d.n_shapes = self.shapes, self.desc.n_shapes
        d.materials, d.n_materials = self.materials, self.desc.n_materials
        d.textures, d.n_textures = self.textures, self.desc.n_textures
        d.environment = self.desc.environment
        out.desc = d
        out.lights = [l.to_abi() for l in getattr(scene, "lights", [])]
        return out

    def content_hash(self) -> str:
        """sha256 over everything a render depends on: every struct field that is not a pointer, and the arrays the
        pointers name (vertices, indices, normals, uvs, image and HDR pixels).  Identifies a scene in a checkpoint."""
        import hashlib
        h = hashlib.sha256()

        def feed(obj):
            for name, _ in obj._fields_:
                v = getattr(obj, name)
                if isinstance(v, C.Structure):
                    feed(v)
                elif isinstance(v, C._Pointer):
                    if v:                                     # the array it names is hashed below: it must be one of the kept ones
                        addr = C.cast(v, C.c_void_p).value
                        assert any(isinstance(a, np.ndarray) and a.ctypes.data == addr for a in self._keep), f"{name}: pointer without a kept array"
                    continue
                elif isinstance(v, C.Array):
                    h.update(bytes(v))
                else:
                    h.update(repr(v).encode())
        d = self.desc
        for arr, n in ((self.objects, d.n_objects), (self.shapes, d.n_shapes), (self.materials, d.n_materials), (self.textures, d.n_textures)):
            for i in range(n):
                feed(arr[i])
        feed(d.environment)
        for l in getattr(self, "lights", []):           # (nothing where there are none: such a scene keeps its hash)
            h.update(b"light")
            feed(l)
        for a in self._keep:
            if isinstance(a, np.ndarray):
                h.update(str(a.shape).encode())
                h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()


# --------------------------------------------------------------------------- camera / renderer
class CameraSettings:
    """src/camera.rs:18-71"""

    def __init__(self):
        self._cam_pos = _v3((0.0, 0.0, -10.0))
        self._look_at = _v3((0.0, 0.0, 0.0))
        self._vfov = 30.0
        self._aperture = 0.0
        self._focus_dist = 10.0

    @staticmethod
    def default():
        return CameraSettings()

    def cam_pos(self, v):
        self._cam_pos = _v3(v)
        return self

    def look_at(self, v):
        self._look_at = _v3(v)
        return self

    def field_of_view(self, vfov):
        self._vfov = float(vfov)
        return self

    def aperture(self, a):
        self._aperture = float(a)
        return self

    def focus_dist(self, d):
        self._focus_dist = float(d)
        return self

    def to_abi(self) -> A.fw_camera_settings:
        return A.fw_camera_settings(A.vec3(self._cam_pos), A.vec3(self._look_at), self._vfov, self._aperture,
                                    self._focus_dist)


@dataclass
class RenderResult:
    rgb8: np.ndarray       # (N,3) uint8  — `Vec<Color>` (render.rs:109)
    gamma: np.ndarray      # (N,3) float32 post-gamma clamped (render.rs:185-187)
    linear: np.ndarray     # (N,3) float32 pre-gamma mean (render.rs:184)
    stats: dict
    width: int
    height: int
    raw: Optional["RenderResult"] = None   # render_denoised: the frame before filtering

    def image(self) -> np.ndarray:
        return self.rgb8.reshape(self.height, self.width, 3)


@dataclass
class AdaptiveResult:
    """fw_render_adaptive's outputs (numpy arrays, or the caller's device tensors): rgb8 / gamma / linear (N, 3) as RenderResult, each
    pixel resolved with its own sample count; accum (N, 4) sums as fw_render_progressive keeps them; moments (N, 4) sums of squares and
    .w = the pixel's sample count; round_pixels (32,) the active pixels of each round, then zeros."""
    rgb8: object
    gamma: object
    linear: object
    accum: object
    moments: object
    round_pixels: object
    stats: dict
    width: int
    height: int

    @property
    def counts(self):
        """(H, W) uint32: every pixel's final sample count"""
        m = self.moments
        if type(m).__module__.startswith("torch"):
            import torch
            return m[:, 3].to(torch.int64).reshape(self.height, self.width)
        return m[:, 3].astype(np.uint32).reshape(self.height, self.width)

    @property
    def rounds(self):
        """the active pixels of each round that ran"""
        r = [int(x) for x in (self.round_pixels.tolist() if self.round_pixels is not None else [])]
        return [x for x in r if x > 0]

    def image(self) -> np.ndarray:
        return self.rgb8.reshape(self.height, self.width, 3)


@dataclass
class ViewsResult:
    """fw_render_views' outputs: one view per camera, each as RenderResult's arrays.  rgb8 (V, H, W, 3) uint8 and gamma_rgb /
    linear_rgb (V, H, W, 3) float32 for whole frames; (V, N, 3) for a pixel subset."""
    rgb8: np.ndarray
    gamma_rgb: np.ndarray
    linear_rgb: np.ndarray
    stats: dict
    width: int
    height: int
    subset: bool = False

    def __post_init__(self):
        if not self.subset:
            v = self.rgb8.shape[0]
            self.rgb8 = self.rgb8.reshape(v, self.height, self.width, 3)
            self.gamma_rgb = self.gamma_rgb.reshape(v, self.height, self.width, 3)
            self.linear_rgb = self.linear_rgb.reshape(v, self.height, self.width, 3)


@dataclass
class RaysResult:
    """fw_render_rays' outputs, in ray order (numpy arrays, or device tensors for device rays): rgb8 (N, 3) uint8, gamma / linear (N, 3)
    float32 as RenderResult, accum (N, 4) float32 sums as fw_render_progressive keeps them."""
    rgb8: object
    gamma: object
    linear: object
    accum: object
    stats: dict

    def image(self, width: int, height: int) -> np.ndarray:
        rgb8 = self.rgb8.cpu().numpy() if type(self.rgb8).__module__.startswith("torch") else self.rgb8
        return np.asarray(rgb8).reshape(height, width, 3)


# --------------------------------------------------------------------------- camera models over fw_render_rays
def _hash32(x: np.ndarray) -> np.ndarray:
    """a 32-bit integer mix (uint32 arrays, wrapping arithmetic)"""
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def pixel_jitter(seed: int, sample: int, n: int) -> np.ndarray:
    """(n, 2) float64 in [0, 1): the sub-pixel offsets (x, y) of pixels 0..n-1 for one absolute sample, from a counter-based generator
    keyed by (seed, sample, pixel, axis): sample s's offsets do not depend on which other samples are made with them."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s32 = ((seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF
    key = _hash32(np.array([s32 ^ int(_hash32(np.array([(int(sample) + 0x9E3779B9) & 0xFFFFFFFF]))[0])], np.uint32))[0]
    ctr = np.arange(2 * n, dtype=np.uint64).astype(np.uint32)
    bits = _hash32(_hash32(ctr) ^ key) >> np.uint32(8)
    return (bits.astype(np.float64) * 2.0 ** -24).reshape(n, 2)


def _pixel_grid(width: int, height: int, sample: int, seed: int, jitter: bool):
    """x + xi_x and j + xi_y of every pixel, row-major with row 0 = image top, float64"""
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError("width and height must be >= 1")
    j, x = np.divmod(np.arange(w * h, dtype=np.int64), w)
    xi = pixel_jitter(seed, sample, w * h) if jitter else np.full((w * h, 2), 0.5)
    return x + xi[:, 0], j + xi[:, 1]


def _rays_out(o: np.ndarray, d: np.ndarray, device):
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(np.float32))
    if device is None:
        return rays
    import torch
    return torch.from_numpy(rays).to(torch.device("cuda", device) if isinstance(device, int) else device)


def panorama_rays(position, width: int, height: int, sample: int, seed: int = 0, jitter: bool = True, device=None):
    """Equirectangular panorama rays from `position`: (W*H, 6) float32 origin + direction, row-major, row 0 = image top, for absolute
    sample `sample` (jitter from pixel_jitter(seed, sample); jitter=False: pixel centres).  The exact inverse of the HDR environment
    lookup (sphere_uv, env_sample): for pixel (x, row j), u = (x + xi_x) / W, v = 1 - (j + xi_y) / H, phi = pi - 2 pi u,
    theta = pi v - pi / 2, d = (cos theta cos phi, sin theta, cos theta sin phi) — so a panorama rendered this way loads as an
    HdrEnvironment with the same orientation.  Computed in float64, rounded to float32.  device: a torch device (or index) to return a
    tensor on instead of a numpy array."""
    w, h = int(width), int(height)
    px, py = _pixel_grid(w, h, sample, seed, jitter)
    u, v = px / w, 1.0 - py / h
    phi, theta = np.pi - 2.0 * np.pi * u, np.pi * v - np.pi / 2.0
    d = np.stack([np.cos(theta) * np.cos(phi), np.sin(theta), np.cos(theta) * np.sin(phi)], axis=1)
    o = np.broadcast_to(np.asarray(position, np.float64).reshape(1, 3), d.shape)
    return _rays_out(o, d, device)


def orthographic_rays(camera: CameraSettings, view_height: float, width: int, height: int, sample: int, seed: int = 0, jitter: bool = True,
                      device=None):
    """Orthographic rays: (W*H, 6) float32, row-major, row 0 = image top, for absolute sample `sample` (jitter as panorama_rays).  The
    basis is camera.rs's: w = unit(cam_pos - look_at), u = unit(Y x w), v = w x u.  The view plane is view_height high and
    view_height * W / H wide, centred on cam_pos; pixel (x, row j) starts at cam_pos + (s - 1/2) view_width u + (t - 1/2) view_height v
    with s = (x + xi_x) / W, t = 1 - (j + xi_y) / H, and every ray's direction is look_at - cam_pos.  Computed in float64, rounded to
    float32.  The camera's field of view, aperture and focus distance are not used."""
    w_px, h_px = int(width), int(height)
    pos = np.asarray(camera._cam_pos, np.float64)
    at = np.asarray(camera._look_at, np.float64)
    w = pos - at
    w = w / np.linalg.norm(w)
    u = np.cross(np.array([0.0, 1.0, 0.0]), w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    vh = float(view_height)
    vw = vh * w_px / h_px
    px, py = _pixel_grid(w_px, h_px, sample, seed, jitter)
    s, t = px / w_px, 1.0 - py / h_px
    o = pos + ((s - 0.5) * vw)[:, None] * u + ((t - 0.5) * vh)[:, None] * v
    d = np.broadcast_to((at - pos).reshape(1, 3), o.shape)
    return _rays_out(o, d, device)


def fisheye_rays(camera: CameraSettings, fov: float, width: int, height: int, sample: int, seed: int = 0, jitter: bool = True, device=None):
    """Equidistant, full-frame fisheye rays: (W*H, 6) float32, row-major, row 0 = image top, for absolute sample `sample` (jitter as
    panorama_rays).  The basis is camera.rs's (see orthographic_rays).  `fov` is the full angle across the image diagonal in degrees, in
    (0, 360].  For pixel (x, row j): a = 2 (x + xi_x) - W, b = H - 2 (j + xi_y), rho = sqrt(a^2 + b^2), r = rho / sqrt(W^2 + H^2) (0 at
    the centre, 1 in the corners), theta = r * fov / 2 the angle to the view direction (equidistant: proportional to the distance from
    the centre), d = sin theta * (a u + b v) / rho - cos theta * w, and d = -w where rho = 0; the origin is cam_pos.  Computed in
    float64, rounded to float32.  The camera's field of view, aperture and focus distance are not used."""
    w_px, h_px = int(width), int(height)
    fov = float(fov)
    if not 0.0 < fov <= 360.0:
        raise ValueError("fov must be in (0, 360] degrees")
    pos = np.asarray(camera._cam_pos, np.float64)
    at = np.asarray(camera._look_at, np.float64)
    w = pos - at
    w = w / np.linalg.norm(w)
    u = np.cross(np.array([0.0, 1.0, 0.0]), w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    px, py = _pixel_grid(w_px, h_px, sample, seed, jitter)
    a, b = 2.0 * px - w_px, h_px - 2.0 * py
    rho = np.sqrt(a * a + b * b)
    theta = (rho / np.sqrt(float(w_px) * float(w_px) + float(h_px) * float(h_px))) * (fov * (np.pi / 180.0) / 2.0)
    safe = np.where(rho > 0.0, rho, 1.0)
    e = (a[:, None] * u + b[:, None] * v) / safe[:, None]
    d = np.sin(theta)[:, None] * e - np.cos(theta)[:, None] * w
    d = np.where((rho > 0.0)[:, None], d, -w)
    o = np.broadcast_to(pos.reshape(1, 3), d.shape)
    return _rays_out(o, d, device)


class CameraModel:
    """A non-pinhole camera whose rays are generated on the device (fw_camera_model): CameraModel.panorama(...),
    .orthographic(...) or .fisheye(...), then .seed(s) / .jitter(on) as builders.  .rays(sample) is the numpy float64 statement of what
    the device generates (panorama_rays, orthographic_rays, fisheye_rays); _lib.model_rays(model, ...) the device's own."""

    def __init__(self, kind: int, width: int, height: int, camera: CameraSettings, view_height: float = 0.0, fov: float = 0.0):
        self.kind, self.width, self.height, self.camera = int(kind), int(width), int(height), camera
        self.view_height, self.fov = float(view_height), float(fov)
        self._seed, self._jitter, self.chunk_samples = 0, True, 0

    @staticmethod
    def panorama(position, width: int, height: int) -> "CameraModel":
        """an equirectangular 360-degree image from `position` (panorama_rays)"""
        pos = _v3(position)
        return CameraModel(A.FW_MODEL_PANORAMA, width, height, CameraSettings.default().cam_pos(pos).look_at(pos + _v3((0.0, 0.0, -1.0))))

    @staticmethod
    def orthographic(camera: CameraSettings, view_height: float, width: int, height: int) -> "CameraModel":
        """parallel rays along the camera's view direction over a view plane `view_height` high (orthographic_rays)"""
        return CameraModel(A.FW_MODEL_ORTHOGRAPHIC, width, height, camera, view_height=view_height)

    @staticmethod
    def fisheye(camera: CameraSettings, fov: float, width: int, height: int) -> "CameraModel":
        """an equidistant full-frame fisheye along the camera's view direction, `fov` degrees across the diagonal (fisheye_rays)"""
        return CameraModel(A.FW_MODEL_FISHEYE, width, height, camera, fov=fov)

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def rays(self, sample: int, device=None):
        """the numpy statement of one absolute sample's rays: (W*H, 6) float32 (device: see panorama_rays)"""
        if self.kind == A.FW_MODEL_PANORAMA:
            return panorama_rays(self.camera._cam_pos, self.width, self.height, sample, self._seed, self._jitter, device)
        if self.kind == A.FW_MODEL_ORTHOGRAPHIC:
            return orthographic_rays(self.camera, self.view_height, self.width, self.height, sample, self._seed, self._jitter, device)
        return fisheye_rays(self.camera, self.fov, self.width, self.height, sample, self._seed, self._jitter, device)

    def to_abi(self) -> A.fw_camera_model:
        m = A.fw_camera_model()
        m.kind, m.width, m.height, m.camera = self.kind, self.width, self.height, self.camera.to_abi()
        m.view_height, m.fov, m.jitter = self.view_height, self.fov, int(self._jitter)
        m.seed, m.chunk_samples = self._seed & 0xFFFFFFFFFFFFFFFF, int(self.chunk_samples)
        return m


# --------------------------------------------------------------------------- irradiance probes (fw_bake_probes)
_SH_Y0 = 0.5 * np.sqrt(1.0 / np.pi)
_SH_C1 = np.sqrt(3.0 / (4.0 * np.pi))
_SH_C2 = 0.5 * np.sqrt(15.0 / np.pi)
_SH_C6 = 0.25 * np.sqrt(5.0 / np.pi)
_SH_C8 = 0.25 * np.sqrt(15.0 / np.pi)
# the Ramamoorthi-Hanrahan cosine-lobe factors of the bands l = 0, 1, 2, per coefficient
_SH_COSINE = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def sh_basis(dirs) -> np.ndarray:
    """(..., 9) float64: the real orthonormal spherical harmonics up to l = 2 of the unit directions dirs (..., 3), index k = l (l + 1) + m,
    polar axis as written (no renormalisation): Y0 = 1/2 sqrt(1/pi), Y1..3 = sqrt(3/4pi) (y, z, x), Y4 = 1/2 sqrt(15/pi) x y,
    Y5 = 1/2 sqrt(15/pi) y z, Y6 = 1/4 sqrt(5/pi) (3 z z - 1), Y7 = 1/2 sqrt(15/pi) x z, Y8 = 1/4 sqrt(15/pi) (x x - y y)."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full(x.shape, _SH_Y0), _SH_C1 * y, _SH_C1 * z, _SH_C1 * x, (_SH_C2 * x) * y, (_SH_C2 * y) * z,
                     _SH_C6 * (3.0 * (z * z) - 1.0), (_SH_C2 * x) * z, _SH_C8 * (x * x - y * y)], axis=-1)


def sh_project(rays, accum, samples: int, directions: int) -> np.ndarray:
    """The float64 statement of fw_probe_project: (N, 9, 3) with proj[p][k][c] = (4 pi / D) sum_j Y_k(d_pj) accum[p D + j][c] / samples,
    for rays (N * D, 6) (the directions as stored) and accum (N * D, 4) (r, g, b sums, then segments)."""
    D = int(directions)
    r = np.asarray(rays, np.float64).reshape(-1, D, 6)
    a = np.asarray(accum, np.float64).reshape(-1, D, 4)[..., :3] / float(samples)
    return (4.0 * np.pi / D) * np.einsum("pjk,pjc->pkc", sh_basis(r[..., 3:]), a)


def sh_radiance(sh, dirs) -> np.ndarray:
    """The radiance the coefficients sh (..., 9, 3) reconstruct along the unit directions dirs (M, 3): (..., M, 3) float64."""
    return np.einsum("mk,...kc->...mc", sh_basis(np.asarray(dirs, np.float64).reshape(-1, 3)), np.asarray(sh, np.float64))


def sh_irradiance(sh, normals) -> np.ndarray:
    """The irradiance on surfaces with the unit normals (M, 3) under the radiance sh (..., 9, 3) describes: (..., M, 3) float64, the
    Ramamoorthi-Hanrahan cosine convolution, band factors pi, 2 pi / 3 and pi / 4."""
    y = sh_basis(np.asarray(normals, np.float64).reshape(-1, 3)) * _SH_COSINE
    return np.einsum("mk,...kc->...mc", y, np.asarray(sh, np.float64))


class ProbeSet:
    """Irradiance probes (fw_probe_set): N positions with `directions` rays each, per round a spherical Fibonacci lattice
    with a Cranley-Patterson shift per (round, probe).  ProbeSet(positions, directions=256) or ProbeSet.grid(lo, hi, (nx, ny, nz)), then
    .seed(s) / .jitter(on) as builders.  .rays(round) is the numpy float64 statement of what the device generates; _lib.probe_rays(set,
    ...) the device's own."""

    def __init__(self, positions, directions: int = 256):
        self.positions = np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1, 3))
        self.directions = int(directions)
        self._seed, self._jitter, self.chunk_probes = 0, True, 0
        self.grid_lo = self.grid_hi = self.grid_counts = None      # set by ProbeSet.grid: what fw_probe_irradiance needs to read sh back

    @staticmethod
    def grid(lo, hi, counts, directions: int = 256) -> "ProbeSet":
        """nx x ny x nz probes on a regular grid from corner lo to corner hi, both included (a count of 1 sits at the middle), x
        fastest, then y, then z.  The set remembers the grid: .grid_lo and .grid_hi (float64 triples) and .grid_counts."""
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        if len(counts) != 3 or any(int(n) < 1 for n in counts):
            raise ValueError("counts must be three numbers >= 1")
        axes = [np.linspace(lo[k], hi[k], int(counts[k])) if int(counts[k]) > 1 else np.array([0.5 * (lo[k] + hi[k])]) for k in range(3)]
        z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        out = ProbeSet(np.stack([x, y, z], axis=-1).reshape(-1, 3), directions)
        out.grid_lo, out.grid_hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        out.grid_counts = tuple(int(n) for n in counts)
        return out

    @property
    def n_probes(self) -> int:
        return int(self.positions.shape[0])

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def shifts(self, round: int) -> np.ndarray:
        """(N, 2) float64: the shift (xi_u, xi_v) of every probe in `round` (pixel_jitter with sample -> round, pixel -> probe)"""
        n = self.n_probes
        return pixel_jitter(self._seed, round, n) if self._jitter else np.full((n, 2), 0.5)

    def rays(self, round: int, device=None):
        """the numpy statement of one round's rays: (N * D, 6) float32, entry p * D + j = direction j of probe p (device: see
        panorama_rays).  In float64, rounded once: u = (j + xi_u) / D, c = 1 - 2 u, rad = sqrt(max(0, 1 - c c)), t = j g + xi_v with
        g = (sqrt(5) - 1) / 2, v = t - floor(t), phi = 2 pi v, d = (rad cos phi, c, rad sin phi)."""
        n, D = self.n_probes, self.directions
        if D < 1:
            raise ValueError("directions must be >= 1")
        xi = self.shifts(round)
        j = np.arange(D, dtype=np.float64)[None, :]
        u = (j + xi[:, 0:1]) / float(D)
        c = 1.0 - 2.0 * u
        rad = np.sqrt(np.maximum(0.0, 1.0 - c * c))
        g = (np.sqrt(5.0) - 1.0) / 2.0
        t = j * g + xi[:, 1:2]
        v = t - np.floor(t)
        phi = (2.0 * np.pi) * v
        d = np.stack([rad * np.cos(phi), c, rad * np.sin(phi)], axis=-1).reshape(n * D, 3)
        o = np.repeat(self.positions.astype(np.float64), D, axis=0)
        return _rays_out(o, d, device)

    def moved(self, placement) -> "ProbeSet":
        """The set at the moved positions float32((double)position + (double)offset) of a placement (N, 4) (ox, oy, oz, a) — what
        fw_relocate_probes traces from, and where sh and depth maps are baked for the placed lookups.  Directions, seed, jitter, chunk and
        the grid are kept: the grid stays the nominal one."""
        pl = np.asarray(placement, np.float32).reshape(self.n_probes, 4)
        out = ProbeSet((self.positions.astype(np.float64) + pl[:, 0:3].astype(np.float64)).astype(np.float32), self.directions)
        out._seed, out._jitter, out.chunk_probes = self._seed, self._jitter, self.chunk_probes
        out.grid_lo, out.grid_hi, out.grid_counts = self.grid_lo, self.grid_hi, self.grid_counts
        return out

    def to_abi(self):
        """(fw_probe_set, the float32 positions it points into: keep them alive as long as the struct is used)"""
        s = A.fw_probe_set()
        s.n_probes, s.positions = self.n_probes, self.positions.ctypes.data_as(C.POINTER(C.c_float))
        s.directions, s.jitter = self.directions, int(self._jitter)
        s.seed, s.chunk_probes = self._seed & 0xFFFFFFFFFFFFFFFF, int(self.chunk_probes)
        return s, self.positions


# --------------------------------------------------------------------------- baked probes read back
class ProbeGrid:
    """A probe grid as fw_probe_irradiance and fw_probe_shade read it (fw_probe_grid): the corners and counts ProbeSet.grid was given,
    and wrap = FW_PROBE_WRAP.  ProbeGrid(lo, hi, counts, wrap=True), or ProbeGrid.of(probes, wrap=True) from a ProbeSet made by
    ProbeSet.grid (a free ProbeSet: ValueError)."""

    def __init__(self, lo, hi, counts, wrap: bool = True):
        self.lo, self.hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        self.counts = tuple(int(n) for n in counts)
        if len(self.lo) != 3 or len(self.hi) != 3 or len(self.counts) != 3 or min(self.counts) < 1:
            raise ValueError("a probe grid needs two corners of three numbers and three counts >= 1")
        self.wrap = bool(wrap)

    @staticmethod
    def of(grid, wrap: bool = True) -> "ProbeGrid":
        if isinstance(grid, ProbeGrid):
            return grid
        if getattr(grid, "grid_counts", None) is None:
            raise ValueError("the probes have no grid: only a ProbeSet made by ProbeSet.grid can be looked up")
        return ProbeGrid(grid.grid_lo, grid.grid_hi, grid.grid_counts, wrap)

    @property
    def n_probes(self) -> int:
        return self.counts[0] * self.counts[1] * self.counts[2]

    def to_abi(self) -> A.fw_probe_grid:
        g = A.fw_probe_grid()
        for k in range(3):
            g.lo[k], g.hi[k], g.counts[k] = self.lo[k], self.hi[k], self.counts[k]
        g.flags = A.FW_PROBE_WRAP if self.wrap else 0
        return g


def probe_lookup(grid, sh, positions, normals, terms: bool = False) -> np.ndarray:
    """The numpy float64 statement of fw_probe_irradiance (include/firework_hip.h): the irradiance (N, 3) float64 — before the device's
    one rounding to float32 — that the grid `grid` (a ProbeGrid, or a ProbeSet made by ProbeSet.grid: wrap on) with the coefficients sh
    (n, 9, 3) gives at the float32 points `positions` with the float32 normals `normals`, (N, 3) each.  Every operation is written in
    the header's order; only + - * /, floor, min, max and sqrt are used.  terms=True: returns (E, T) with T (N, 3) =
    sum over corners and k of |w B_k sh|, what a rounding-error bound of the sum scales with."""
    g = ProbeGrid.of(grid)
    sh = np.asarray(sh, np.float32).astype(np.float64).reshape(g.n_probes, 9, 3)
    p = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    n = p.shape[0]
    E, T = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        nl2 = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        ok = np.all(np.isfinite(p), axis=1) & np.all(np.isfinite(nr), axis=1) & (nl2 > 0.0)
        nl = np.sqrt(nl2)
        nh = nr / nl[:, None]
        x, y, z = nh[:, 0], nh[:, 1], nh[:, 2]
        idx, f, two = [], [], []
        for k in range(3):
            c = g.counts[k]
            two.append(c > 1)
            if c > 1:
                cm1 = float(c - 1)
                s = ((p[:, k] - g.lo[k]) / (g.hi[k] - g.lo[k])) * cm1
                s = np.fmin(np.fmax(s, 0.0), cm1)
                fl = np.fmin(np.floor(s), cm1 - 1.0)
                idx.append(np.where(ok, fl, 0.0).astype(np.int64))
                f.append(s - fl)
            else:
                idx.append(np.zeros(n, np.int64))
                f.append(np.zeros(n))
        corners = [(dx, dy, dz) for dz in range(2 if two[2] else 1) for dy in range(2 if two[1] else 1) for dx in range(2 if two[0] else 1)]
        w = []
        for d in corners:
            wk = [f[k] if d[k] else 1.0 - f[k] for k in range(3)]
            wd = (wk[0] * wk[1]) * wk[2]
            if g.wrap:
                r = []
                for k in range(3):
                    if two[k]:
                        pk = g.lo[k] + (idx[k] + d[k]).astype(np.float64) * ((g.hi[k] - g.lo[k]) / float(g.counts[k] - 1))
                    else:
                        pk = 0.5 * (g.lo[k] + g.hi[k])
                    r.append(pk - p[:, k])
                rl2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
                rl = np.sqrt(rl2)
                dot = (x * (r[0] / rl) + y * (r[1] / rl)) + z * (r[2] / rl)
                h = 0.5 * (dot + 1.0)
                wd = wd * np.where(rl2 > 0.0, h * h + 0.2, 1.2)
            w.append(wd)
        if g.wrap:
            wsum = np.zeros(n)
            for wd in w:
                wsum = wsum + wd
            w = [wd / wsum for wd in w]
        B = sh_basis(nh) * _SH_COSINE
        for d, wd in zip(corners, w):
            probe = ((idx[2] + d[2]) * g.counts[1] + (idx[1] + d[1])) * g.counts[0] + (idx[0] + d[0])
            c = sh[probe]                                                  # (N, 9, 3)
            e = B[:, 0, None] * c[:, 0]
            t = np.abs(e)
            for k in range(1, 9):
                term = B[:, k, None] * c[:, k]
                e = e + term
                t = t + np.abs(term)
            E = E + wd[:, None] * e
            T = T + np.abs(wd)[:, None] * t
    E[~ok] = 0.0
    T[~ok] = 0.0
    return (E, T) if terms else E


def probe_shade_ref(grid, sh, aov, irradiance=None) -> np.ndarray:
    """The float32 statement of fw_probe_shade's shade step, (N, 3) float32 linear colours (before resolve_pixel): with E = probe_lookup
    at the records' (position, normal) rounded to float32 — or `irradiance`, (N, 3) float32, when given — and clamped at 0,
    out_c = a_c (v (E_c float32(1 / pi)) + (1 - v)) for fw_render_aovs' records aov (N, 12)."""
    a = np.asarray(aov, np.float32).reshape(-1, 12)
    E = probe_lookup(grid, sh, a[:, 8:11], a[:, 4:7]).astype(np.float32) if irradiance is None else np.asarray(irradiance, np.float32).reshape(-1, 3)
    E = np.where(E > 0, E, np.float32(0.0)).astype(np.float32)
    v = a[:, 3:4]
    inv_pi = np.float32(1.0 / np.pi)
    return (a[:, 0:3] * (v * (E * inv_pi) + (np.float32(1.0) - v))).astype(np.float32)


# --------------------------------------------------------------------------- probe visibility
class ProbeDepth:
    """The depth maps of a probe set (fw_probe_depth): every probe has a resolution x resolution octahedral map of the first two moments
    of the distance to the nearest surface; a ray's weight in a texel is max(0, T.d)^(2^sharpness_log2); distances are clamped to
    max_distance, which a miss counts as."""

    def __init__(self, resolution: int = 8, sharpness_log2: int = 6, max_distance: float = 1.0e3):
        self.resolution, self.sharpness_log2, self.max_distance = int(resolution), int(sharpness_log2), float(np.float32(max_distance))

    def to_abi(self) -> A.fw_probe_depth:
        d = A.fw_probe_depth()
        d.resolution, d.sharpness_log2, d.max_distance = self.resolution, self.sharpness_log2, self.max_distance
        return d


def _sgn1(v):
    return np.where(v >= 0.0, 1.0, -1.0)


def probe_depth_dirs(R: int) -> np.ndarray:
    """(R, R, 3) float64, [b][a] = the unit direction of texel (column a, row b) of an R x R octahedral map, as the header states it"""
    R = int(R)
    e = ((np.arange(R, dtype=np.float64) + 0.5) * 2.0) / float(R) - 1.0
    ex, ey = np.broadcast_to(e[None, :], (R, R)), np.broadcast_to(e[:, None], (R, R))
    z = (1.0 - np.abs(ex)) - np.abs(ey)
    x = np.where(z < 0.0, (1.0 - np.abs(ey)) * _sgn1(ex), ex)
    y = np.where(z < 0.0, (1.0 - np.abs(ex)) * _sgn1(ey), ey)
    l = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / l, y / l, z / l], axis=-1)


def probe_depth_reduce(pd: "ProbeDepth", rays, hits_t, hits_object, directions: int, terms: bool = False) -> np.ndarray:
    """The numpy float64 statement of fw_probe_depth_reduce: (N, R, R, 3) float64, the accumulators (A, B, W) of one round before their
    one rounding to float32, for rays (N * D, 6) float32 (the directions as stored) and the hits' t (float32) and object (uint32,
    0xFFFFFFFF = miss) columns.  terms=True: returns (sums, G) with G (N, 3) = sum_j |d_j|^(2^k) dist_j^m for m = 1, 2, 0 (the order of
    A, B, W): what a rounding-error bound of the weights scales with."""
    D, R, k = int(directions), int(pd.resolution), int(pd.sharpness_log2)
    d = np.asarray(rays, np.float32).astype(np.float64).reshape(-1, D, 6)[..., 3:]
    t = np.asarray(hits_t, np.float32).astype(np.float64).reshape(-1, D)
    miss = np.asarray(hits_object).astype(np.uint32).reshape(-1, D) == np.uint32(0xFFFFFFFF)
    r_max = float(np.float32(pd.max_distance))
    T = probe_depth_dirs(R)
    n = d.shape[0]
    out = np.zeros((n, R, R, 3))
    with np.errstate(all="ignore"):
        length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        dist = np.where(miss, r_max, np.fmin(t * length, r_max))
        for j in range(D):
            dj = d[:, j, None, None, :]
            w = np.fmax(0.0, (T[None, ..., 0] * dj[..., 0] + T[None, ..., 1] * dj[..., 1]) + T[None, ..., 2] * dj[..., 2])
            for _ in range(k):
                w = w * w
            dd = dist[:, j, None, None]
            wd = w * dd
            out[..., 0] = out[..., 0] + wd
            out[..., 1] = out[..., 1] + wd * dd
            out[..., 2] = out[..., 2] + w
        lk = length ** float(2 ** k)
        G = np.stack([(lk * dist).sum(axis=1), (lk * dist * dist).sum(axis=1), lk.sum(axis=1)], axis=-1)
    return (out, G) if terms else out


def probe_depth_moments(pd: "ProbeDepth", sums) -> np.ndarray:
    """The statement of the moments: (N, R, R, 2) float32 (mu, mu2) = float32(sums.x / sums.z), float32(sums.y / sums.z) in float64 from
    the float32 running sums (N, R, R, 4); a texel with sums.z == 0 gets (r_max, float32(r_max r_max))."""
    s = np.asarray(sums, np.float32).astype(np.float64)
    r_max = float(np.float32(pd.max_distance))
    with np.errstate(all="ignore"):
        none = s[..., 2] == 0.0
        mu = np.where(none, r_max, s[..., 0] / s[..., 2])
        mu2 = np.where(none, float(np.float32(r_max * r_max)), s[..., 1] / s[..., 2])
        return np.stack([mu, mu2], axis=-1).astype(np.float32)


def probe_depth_fetch(R: int, maps, dirs):
    """(mu, mu2), float64 (M,) each: the bilinear fetch of the header along the unit directions dirs (M, 3) from the maps (M, R, R, 2) —
    one map per direction — edges clamped."""
    R = int(R)
    m = np.asarray(maps, np.float32).astype(np.float64).reshape(-1, R, R, 2)
    v = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    rows = np.arange(m.shape[0])
    with np.errstate(all="ignore"):
        s1 = (np.abs(x) + np.abs(y)) + np.abs(z)
        ox, oy = x / s1, y / s1
        fx, fy = (1.0 - np.abs(oy)) * _sgn1(ox), (1.0 - np.abs(ox)) * _sgn1(oy)
        ox, oy = np.where(z < 0.0, fx, ox), np.where(z < 0.0, fy, oy)
        top = float(R) - 1.0
        su = np.fmin(np.fmax(((ox + 1.0) * 0.5) * float(R) - 0.5, 0.0), top)
        sv = np.fmin(np.fmax(((oy + 1.0) * 0.5) * float(R) - 0.5, 0.0), top)
        iu, jv = np.fmin(np.floor(su), top - 1.0), np.fmin(np.floor(sv), top - 1.0)
        fu, fv = su - iu, sv - jv
        i, j = iu.astype(np.int64), jv.astype(np.int64)
        m00, m10, m01, m11 = m[rows, j, i], m[rows, j, i + 1], m[rows, j + 1, i], m[rows, j + 1, i + 1]
        gu, gv = (1.0 - fu)[:, None], (1.0 - fv)[:, None]
        out = ((m00 * gu + m10 * fu[:, None]) * gv) + ((m01 * gu + m11 * fu[:, None]) * fv[:, None])
    return out[:, 0], out[:, 1]


def probe_lookup_vis(grid, sh, pd: "ProbeDepth", moments, positions, normals, normal_bias: float = 0.0, terms: bool = False):
    """The numpy float64 statement of fw_probe_irradiance_vis (include/firework_hip.h): probe_lookup with every corner's weight multiplied
    by g — the wrap factor (1 without wrap) times the visibility of the corner's probe from p + normal_bias nh, floored at 1e-6 and
    crushed below 0.2 — and the weights always divided by their sum.  moments (n, R, R, 2) float32.  terms=True: returns (E, T, W) with T
    as probe_lookup's and X a dict of per-corner arrays (N, corners), in corner order: the normalised weights "w", and "fac", "v", "g",
    "dist", "mu", "mu2" and "m1", "m2" (the largest |mu| and |mu2| of the corner probe's map), which the error bound of the weights needs."""
    g = ProbeGrid.of(grid)
    R = int(pd.resolution)
    sh = np.asarray(sh, np.float32).astype(np.float64).reshape(g.n_probes, 9, 3)
    mom = np.asarray(moments, np.float32).reshape(g.n_probes, R, R, 2)
    p = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    bias = float(np.float32(normal_bias))
    n = p.shape[0]
    E, T = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        nl2 = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        ok = np.all(np.isfinite(p), axis=1) & np.all(np.isfinite(nr), axis=1) & (nl2 > 0.0)
        nl = np.sqrt(nl2)
        nh = nr / nl[:, None]
        nh = np.where(ok[:, None], nh, 0.0)
        p = np.where(ok[:, None], p, 0.0)
        x, y, z = nh[:, 0], nh[:, 1], nh[:, 2]
        q = p + bias * nh
        idx, f, two = [], [], []
        for k in range(3):
            c = g.counts[k]
            two.append(c > 1)
            if c > 1:
                cm1 = float(c - 1)
                s = ((p[:, k] - g.lo[k]) / (g.hi[k] - g.lo[k])) * cm1
                s = np.fmin(np.fmax(s, 0.0), cm1)
                fl = np.fmin(np.floor(s), cm1 - 1.0)
                idx.append(fl.astype(np.int64))
                f.append(s - fl)
            else:
                idx.append(np.zeros(n, np.int64))
                f.append(np.zeros(n))
        corners = [(dx, dy, dz) for dz in range(2 if two[2] else 1) for dy in range(2 if two[1] else 1) for dx in range(2 if two[0] else 1)]
        w, X = [], {k: [] for k in ("fac", "v", "g", "dist", "mu", "mu2", "m1", "m2")}
        for d in corners:
            wk = [f[k] if d[k] else 1.0 - f[k] for k in range(3)]
            P = []
            for k in range(3):
                if two[k]:
                    P.append(g.lo[k] + (idx[k] + d[k]).astype(np.float64) * ((g.hi[k] - g.lo[k]) / float(g.counts[k] - 1)))
                else:
                    P.append(np.full(n, 0.5 * (g.lo[k] + g.hi[k])))
            fac = np.ones(n)
            if g.wrap:
                r = [P[k] - p[:, k] for k in range(3)]
                rl2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
                rl = np.sqrt(rl2)
                dot = (x * (r[0] / rl) + y * (r[1] / rl)) + z * (r[2] / rl)
                h = 0.5 * (dot + 1.0)
                fac = np.where(rl2 > 0.0, h * h + 0.2, 1.2)
            rv = [q[:, k] - P[k] for k in range(3)]
            dist = np.sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2])
            probe = ((idx[2] + d[2]) * g.counts[1] + (idx[1] + d[1])) * g.counts[0] + (idx[0] + d[0])
            safe = np.where(dist != 0.0, dist, 1.0)
            dirs = np.stack([np.where(dist != 0.0, rv[k] / safe, (0.0, 0.0, 1.0)[k]) for k in range(3)], axis=-1)
            mu, mu2 = probe_depth_fetch(R, mom[probe], dirs)
            var = np.abs(mu * mu - mu2)
            t = dist - mu
            c = var / (var + t * t)
            v = np.where((dist == 0.0) | (dist <= mu), 1.0, (c * c) * c)
            gg = np.fmax(1e-6, fac * v)
            gg = np.where(gg < 0.2, (gg * (gg * gg)) * 25.0, gg)
            w.append(((wk[0] * wk[1]) * wk[2]) * gg)
            if terms:
                am = np.abs(mom.astype(np.float64)).reshape(g.n_probes, -1, 2).max(axis=1)
                for name, val in (("fac", fac), ("v", v), ("g", gg), ("dist", dist), ("mu", mu), ("mu2", mu2), ("m1", am[probe, 0]), ("m2", am[probe, 1])):
                    X[name].append(val)
        wsum = np.zeros(n)
        for wd in w:
            wsum = wsum + wd
        w = [wd / wsum for wd in w]
        B = sh_basis(nh) * _SH_COSINE
        for d, wd in zip(corners, w):
            probe = ((idx[2] + d[2]) * g.counts[1] + (idx[1] + d[1])) * g.counts[0] + (idx[0] + d[0])
            c = sh[probe]                                                  # (N, 9, 3)
            e = B[:, 0, None] * c[:, 0]
            t = np.abs(e)
            for k in range(1, 9):
                term = B[:, k, None] * c[:, k]
                e = e + term
                t = t + np.abs(term)
            E = E + wd[:, None] * e
            T = T + np.abs(wd)[:, None] * t
    E[~ok] = 0.0
    T[~ok] = 0.0
    if not terms:
        return E
    X = {k: np.stack(v, axis=-1) for k, v in X.items()}
    X["w"] = np.stack(w, axis=-1)
    return E, T, X


# --------------------------------------------------------------------------- probe relocation and classification
class ProbeRelocation:
    """How probes are moved out of geometry (fw_probe_relocate): a probe keeps at least min_front to the nearest front face; one that
    sees more than back_fraction of back faces is inside geometry and is moved through the nearest of them; no offset may exceed
    max_offset (three numbers, world units per axis; a move that would is rejected, and the probe ends inactive).  max_offset=None:
    0.45 x the grid's spacing per axis, on a flat axis the smallest spacing of the other axes — taken from the ProbeSet the relocation is
    used with.  steps: how many moving steps Renderer.relocate_probes runs before it classifies."""

    def __init__(self, min_front: float, back_fraction: float = 0.25, max_offset=None, steps: int = 4):
        self.min_front, self.back_fraction = float(np.float32(min_front)), float(np.float32(back_fraction))
        self.max_offset = None if max_offset is None else tuple(float(np.float32(v)) for v in (max_offset if np.ndim(max_offset) else (max_offset,) * 3))
        if self.max_offset is not None and len(self.max_offset) != 3:
            raise ValueError("max_offset must be one number or three")
        self.steps = int(steps)

    def resolved(self, probes=None) -> "ProbeRelocation":
        """this relocation with a max_offset of its own: None becomes 0.45 x the spacing of `probes`' grid (a ProbeSet made by
        ProbeSet.grid, or a ProbeGrid)"""
        if self.max_offset is not None:
            return self
        if probes is None:
            raise ValueError("max_offset=None needs the probes' grid")
        return ProbeRelocation(self.min_front, self.back_fraction, tuple(0.45 * v for v in probe_spacing(probes)), self.steps)

    def to_abi(self, probes=None) -> A.fw_probe_relocate:
        r = self.resolved(probes)
        a = A.fw_probe_relocate()
        a.min_front, a.back_fraction = r.min_front, r.back_fraction
        for k in range(3):
            a.max_offset[k] = r.max_offset[k]
        return a


def probe_spacing(grid) -> tuple:
    """the distance between neighbouring probes of a grid (a ProbeGrid, or a ProbeSet made by ProbeSet.grid) per axis; a flat axis takes
    the smallest spacing of the other axes.  A grid of one probe has none: ValueError."""
    g = ProbeGrid.of(grid)
    sp = [abs(g.hi[k] - g.lo[k]) / float(g.counts[k] - 1) if g.counts[k] > 1 else None for k in range(3)]
    known = [v for v in sp if v is not None]
    if not known:
        raise ValueError("a grid of one probe has no spacing: give max_offset")
    return tuple(v if v is not None else min(known) for v in sp)


def neutral_placement(n: int) -> np.ndarray:
    """(n, 4) float32 records (0, 0, 0, 1): every probe at its nominal position and active"""
    out = np.zeros((int(n), 4), np.float32)
    out[:, 3] = 1.0
    return out


def probe_survey(rays, hits_t, hits_normal, hits_object, directions: int, terms: bool = False):
    """The numpy float64 statement of fw_probe_survey: (N, 3, 4) float64 — (back.xyz, dist), (front.xyz, dist), (n_back, n_front, n_miss,
    0), the distances before their one rounding to float32 — for rays (N * D, 6) float32 (the directions as stored) and the hits' t
    (float32), normal (float32, (N * D, 3)) and object (uint32, 0xFFFFFFFF = miss) columns.  terms=True: returns (survey, J) with J (N, 2)
    int64 the winning ray of each class, -1 for none."""
    D = int(directions)
    d32 = np.asarray(rays, np.float32).reshape(-1, D, 6)[..., 3:]
    d = d32.astype(np.float64)
    t = np.asarray(hits_t, np.float32).astype(np.float64).reshape(-1, D)
    nr = np.asarray(hits_normal, np.float32).astype(np.float64).reshape(-1, D, 3)
    obj = np.asarray(hits_object).astype(np.uint32).reshape(-1, D)
    n = d.shape[0]
    rows = np.arange(n)
    out = np.zeros((n, 3, 4))
    J = np.full((n, 2), -1, np.int64)
    with np.errstate(all="ignore"):
        zero = np.all(d == 0.0, axis=2)
        miss = ~zero & (obj == np.uint32(0xFFFFFFFF))
        hit = ~zero & ~miss
        dist = t * np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        back = hit & (((nr[..., 0] * d[..., 0] + nr[..., 1] * d[..., 1]) + nr[..., 2] * d[..., 2]) > 0.0)
        front = hit & ~back
        for c, m in enumerate((back, front)):
            dd = np.where(m & ~np.isnan(dist), dist, np.inf)
            j = np.argmin(dd, axis=1)                      # the first of equal minima: the lowest j
            dm = dd[rows, j]
            has = dm < np.inf
            out[:, c, 0:3] = np.where(has[:, None], d[rows, j], 0.0)
            out[:, c, 3] = np.where(has, dm, np.inf)
            J[:, c] = np.where(has, j, -1)
        out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = back.sum(axis=1), front.sum(axis=1), miss.sum(axis=1)
    return (out, J) if terms else out


def probe_relocate_step(relocation: "ProbeRelocation", survey, placement, directions: int, move: bool = True) -> np.ndarray:
    """The numpy statement of fw_probe_relocate_step: the placement (N, 4) float32 after one step of `relocation` (with a max_offset of its
    own) over the float32 survey (N, 3, 4) and the placement (N, 4) before it, in float64, the candidate rounded to float32 once."""
    rl = relocation.resolved()
    sv = np.asarray(survey, np.float32).astype(np.float64).reshape(-1, 3, 4)
    pl = np.array(np.asarray(placement, np.float32).reshape(-1, 4), np.float32)
    o = pl[:, 0:3].astype(np.float64)
    mf = float(np.float32(rl.min_front))
    inside = sv[:, 2, 0] > float(np.float32(rl.back_fraction)) * float(int(directions))
    a = np.where(inside, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    if not move:
        pl[:, 3] = a
        return pl
    with np.errstate(all="ignore"):
        def unit(v):
            return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
        cb = o + unit(sv[:, 0, 0:3]) * (sv[:, 0, 3] + 0.5 * mf)[:, None]
        cf = o - unit(sv[:, 1, 0:3]) * (mf - sv[:, 1, 3])[:, None]
        near = ~inside & (sv[:, 2, 1] > 0.0) & (sv[:, 1, 3] < mf)
        c = np.where(inside[:, None], cb, np.where(near[:, None], cf, o)).astype(np.float32)
        lim = np.asarray([float(np.float32(v)) for v in rl.max_offset])
        ok = np.all(np.abs(c.astype(np.float64)) <= lim[None, :], axis=1)
    pl[:, 0:3] = np.where(ok[:, None], c, pl[:, 0:3])
    pl[:, 3] = a
    return pl


def probe_lookup_placed(grid, sh, placement, positions, normals, pd: "ProbeDepth" = None, moments=None, normal_bias: float = 0.0,
                        terms: bool = False):
    """The numpy float64 statement of fw_probe_irradiance_placed (include/firework_hip.h): probe_lookup — with pd and moments
    probe_lookup_vis — where a corner's probe stands at P + o, a corner whose a is 0 is skipped (nothing of it enters a sum) and the
    remaining weights are always divided by their sum; no active corner, or a sum of 0, gives zeros.  placement (n, 4) float32.
    terms=True: returns (E, T, X) as probe_lookup_vis does, X with "w" and "active" always and the visibility terms when pd is given;
    a skipped corner's entries are 0."""
    g = ProbeGrid.of(grid)
    vis = pd is not None
    if vis != (moments is not None):
        raise ValueError("pd and moments are given together or not at all")
    sh = np.asarray(sh, np.float32).astype(np.float64).reshape(g.n_probes, 9, 3)
    pl = np.asarray(placement, np.float32).reshape(g.n_probes, 4)
    off, state = pl[:, 0:3].astype(np.float64), pl[:, 3]
    if vis:
        R = int(pd.resolution)
        mom = np.asarray(moments, np.float32).reshape(g.n_probes, R, R, 2)
    p = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    bias = float(np.float32(normal_bias))
    n = p.shape[0]
    E, T = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        nl2 = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        ok = np.all(np.isfinite(p), axis=1) & np.all(np.isfinite(nr), axis=1) & (nl2 > 0.0)
        nl = np.sqrt(nl2)
        nh = np.where(ok[:, None], nr / nl[:, None], 0.0)
        p = np.where(ok[:, None], p, 0.0)
        x, y, z = nh[:, 0], nh[:, 1], nh[:, 2]
        q = p + bias * nh if vis else p
        idx, f, two = [], [], []
        for k in range(3):
            c = g.counts[k]
            two.append(c > 1)
            if c > 1:
                cm1 = float(c - 1)
                s = ((p[:, k] - g.lo[k]) / (g.hi[k] - g.lo[k])) * cm1
                s = np.fmin(np.fmax(s, 0.0), cm1)
                fl = np.fmin(np.floor(s), cm1 - 1.0)
                idx.append(fl.astype(np.int64))
                f.append(s - fl)
            else:
                idx.append(np.zeros(n, np.int64))
                f.append(np.zeros(n))
        corners = [(dx, dy, dz) for dz in range(2 if two[2] else 1) for dy in range(2 if two[1] else 1) for dx in range(2 if two[0] else 1)]
        w, act = [], []
        X = {k: [] for k in ("fac", "v", "g", "dist", "mu", "mu2", "m1", "m2")}
        wsum = np.zeros(n)
        for d in corners:
            probe = ((idx[2] + d[2]) * g.counts[1] + (idx[1] + d[1])) * g.counts[0] + (idx[0] + d[0])
            on = state[probe] != 0.0
            wk = [f[k] if d[k] else 1.0 - f[k] for k in range(3)]
            P = []
            for k in range(3):
                if two[k]:
                    nominal = g.lo[k] + (idx[k] + d[k]).astype(np.float64) * ((g.hi[k] - g.lo[k]) / float(g.counts[k] - 1))
                else:
                    nominal = np.full(n, 0.5 * (g.lo[k] + g.hi[k]))
                P.append(nominal + off[probe, k])
            fac = np.ones(n)
            if g.wrap:
                r = [P[k] - p[:, k] for k in range(3)]
                rl2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
                rl = np.sqrt(rl2)
                dot = (x * (r[0] / rl) + y * (r[1] / rl)) + z * (r[2] / rl)
                h = 0.5 * (dot + 1.0)
                fac = np.where(rl2 > 0.0, h * h + 0.2, 1.2)
            wd = (wk[0] * wk[1]) * wk[2]
            if vis:
                rv = [q[:, k] - P[k] for k in range(3)]
                dist = np.sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2])
                safe = np.where(dist != 0.0, dist, 1.0)
                dirs = np.stack([np.where(dist != 0.0, rv[k] / safe, (0.0, 0.0, 1.0)[k]) for k in range(3)], axis=-1)
                mu, mu2 = probe_depth_fetch(R, mom[probe], dirs)
                var = np.abs(mu * mu - mu2)
                t = dist - mu
                c = var / (var + t * t)
                v = np.where((dist == 0.0) | (dist <= mu), 1.0, (c * c) * c)
                gg = np.fmax(1e-6, fac * v)
                gg = np.where(gg < 0.2, (gg * (gg * gg)) * 25.0, gg)
                wd = wd * gg
                if terms:
                    am = np.abs(mom.astype(np.float64)).reshape(g.n_probes, -1, 2).max(axis=1)
                    for name, val in (("fac", fac), ("v", v), ("g", gg), ("dist", dist), ("mu", mu), ("mu2", mu2), ("m1", am[probe, 0]),
                                      ("m2", am[probe, 1])):
                        X[name].append(np.where(on, val, 0.0))
            elif g.wrap:
                wd = wd * fac
            wd = np.where(on, wd, 0.0)
            wsum = np.where(on, wsum + wd, wsum)
            w.append(wd)
            act.append(on)
        some = ok & (wsum != 0.0)
        w = [np.where(some, wd / np.where(some, wsum, 1.0), 0.0) for wd in w]
        B = sh_basis(nh) * _SH_COSINE
        for d, wd, on in zip(corners, w, act):
            probe = ((idx[2] + d[2]) * g.counts[1] + (idx[1] + d[1])) * g.counts[0] + (idx[0] + d[0])
            c = sh[probe]                                                  # (N, 9, 3)
            e = B[:, 0, None] * c[:, 0]
            t = np.abs(e)
            for k in range(1, 9):
                term = B[:, k, None] * c[:, k]
                e = e + term
                t = t + np.abs(term)
            E = np.where(on[:, None], E + wd[:, None] * e, E)
            T = np.where(on[:, None], T + np.abs(wd)[:, None] * t, T)
    E[~some] = 0.0
    T[~some] = 0.0
    if not terms:
        return E
    X = {k: np.stack(v, axis=-1) for k, v in X.items() if v}
    X["w"] = np.stack(w, axis=-1)
    X["active"] = np.stack(act, axis=-1)
    return E, T, X


# --------------------------------------------------------------------------- probe radiance maps
class ProbeRadiance:
    """The radiance maps of a probe set (fw_probe_radiance): every probe has a pyramid of octahedral maps, level l of resolution
    resolution >> l (at least 4) holding the radiance prefiltered for a GGX lobe of roughness[l]; level 0 is the raw map, a ray's weight
    in a texel max(0, T.d)^(2^sharpness_log2).  roughness None: linspace(0.1, 1, L) with as many levels as the floor of 4 allows.
    .levels, .resolutions, .offsets (the texel offset of every level in a probe's pyramid) and .texels (their total, M)."""

    def __init__(self, resolution: int = 8, sharpness_log2: int = 2, roughness=None):
        self.resolution, self.sharpness_log2 = int(resolution), int(sharpness_log2)
        if self.resolution not in (4, 8, 16, 32):
            raise ValueError("resolution must be 4, 8, 16 or 32")
        if not 0 <= self.sharpness_log2 <= 8:
            raise ValueError("sharpness_log2 must be in 0..8")
        most = min(A.FW_PROBE_RADIANCE_MAX_LEVELS, self.resolution.bit_length() - 2)          # R >> (L - 1) >= 4
        if roughness is None:
            roughness = np.linspace(0.1, 1.0, most)
        rho = np.asarray(roughness, np.float32).reshape(-1)
        if not 1 <= rho.size <= most:
            raise ValueError(f"resolution {self.resolution} allows 1..{most} levels")
        if not (np.all(rho >= 0.0) and np.all(rho <= 1.0) and np.all(np.diff(rho) > 0.0)):
            raise ValueError("roughness must lie in [0, 1] and ascend strictly")
        self.roughness = tuple(float(v) for v in rho)
        self.levels = int(rho.size)
        self.resolutions = tuple(self.resolution >> l for l in range(self.levels))
        self.offsets = tuple(int(sum(r * r for r in self.resolutions[:l])) for l in range(self.levels))
        self.texels = int(sum(r * r for r in self.resolutions))

    def to_abi(self) -> A.fw_probe_radiance:
        d = A.fw_probe_radiance()
        d.resolution, d.sharpness_log2, d.levels = self.resolution, self.sharpness_log2, self.levels
        for l, v in enumerate(self.roughness):
            d.roughness[l] = v
        return d


def probe_radiance_reduce(pr: "ProbeRadiance", rays, accum, samples: int, directions: int, terms: bool = False):
    """The numpy float64 statement of fw_probe_radiance_reduce: (N, R, R, 4) float64, the accumulators (A_r, A_g, A_b, W) of one round
    before their one rounding to float32, for rays (N * D, 6) float32 (the directions as stored) and accum (N * D, 4) float32.
    terms=True: returns (sums, G, B) with G (N, 4) = sum_j |d_j|^(2^k) |L_cj| (1 for W) and B (N, R, R, 4) the sums of the terms'
    magnitudes: what a rounding-error bound scales with."""
    D, R, k = int(directions), int(pr.resolution), int(pr.sharpness_log2)
    d = np.asarray(rays, np.float32).astype(np.float64).reshape(-1, D, 6)[..., 3:]
    a = np.asarray(accum, np.float32).astype(np.float64).reshape(-1, D, 4)
    T = probe_depth_dirs(R)
    n = d.shape[0]
    out, mag = np.zeros((n, R, R, 4)), np.zeros((n, R, R, 4))
    with np.errstate(all="ignore"):
        L = a[..., 0:3] / float(int(samples))
        for j in range(D):
            dj = d[:, j, None, None, :]
            w = np.fmax(0.0, (T[None, ..., 0] * dj[..., 0] + T[None, ..., 1] * dj[..., 1]) + T[None, ..., 2] * dj[..., 2])
            for _ in range(k):
                w = w * w
            on = w > 0.0
            for c in range(3):
                term = w * L[:, j, None, None, c]
                out[..., c] = np.where(on, out[..., c] + term, out[..., c])
                mag[..., c] = np.where(on, mag[..., c] + np.abs(term), mag[..., c])
            out[..., 3] = np.where(on, out[..., 3] + w, out[..., 3])
        mag[..., 3] = out[..., 3]
        length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        lk = length ** float(2 ** k)
        G = np.stack([(lk * np.abs(L[..., c])).sum(axis=1) for c in range(3)] + [lk.sum(axis=1)], axis=-1)
    return (out, G, mag) if terms else out


def probe_radiance_sources(R: int):
    """(S, omega): the unit directions (R * R, 3) of an R x R octahedral map's texels in ascending id, and their solid angles
    omega = (4 / (R R)) / ((len len) len), len the length of the texel's centre on the octahedron: the map's Jacobian at the centre"""
    R = int(R)
    e = ((np.arange(R, dtype=np.float64) + 0.5) * 2.0) / float(R) - 1.0
    ex, ey = np.broadcast_to(e[None, :], (R, R)), np.broadcast_to(e[:, None], (R, R))
    z = (1.0 - np.abs(ex)) - np.abs(ey)
    x = np.where(z < 0.0, (1.0 - np.abs(ey)) * _sgn1(ex), ex)
    y = np.where(z < 0.0, (1.0 - np.abs(ex)) * _sgn1(ey), ey)
    ln = np.sqrt((x * x + y * y) + z * z)
    S = np.stack([x / ln, y / ln, z / ln], axis=-1).reshape(R * R, 3)
    omega = ((4.0 / (float(R) * float(R))) / ((ln * ln) * ln)).reshape(R * R)
    return S, omega


def probe_radiance_weights(pr: "ProbeRadiance", level: int):
    """(w, c, den): the prefilter's weight of every source texel of level 0 in every output texel of `level` >= 1, (R_l^2, R^2) float64 —
    w = ((a2 / (den den)) c) omega with c = (Tx Sx + Ty Sy) + Tz Sz, h = (1 + c) 0.5, den = h (a2 - 1) + 1, a2 = (rho rho)(rho rho) —
    with w = 0 where !(c > 0): those sources are skipped"""
    S, omega = probe_radiance_sources(pr.resolution)
    T = probe_depth_dirs(pr.resolutions[level]).reshape(-1, 3)
    rho = float(np.float32(pr.roughness[level]))
    a = rho * rho
    a2 = a * a
    c = (T[:, None, 0] * S[None, :, 0] + T[:, None, 1] * S[None, :, 1]) + T[:, None, 2] * S[None, :, 2]
    h = (1.0 + c) * 0.5
    den = h * (a2 - 1.0) + 1.0
    w = ((a2 / (den * den)) * c) * omega[None, :]
    return np.where(c > 0.0, w, 0.0), c, den


def probe_radiance_prefilter(pr: "ProbeRadiance", sums, terms: bool = False):
    """The numpy statement of fw_probe_radiance_prefilter: maps (N, M, 4) float32 from the float32 running sums (N, R, R, 4).  Level 0 is
    float32((double)A_c / W) with flag 1, zeros where W == 0; a texel of a level >= 1 is float32(A_c / Wt) over the flagged source texels
    of level 0 in ascending id with probe_radiance_weights' weights, zeros where Wt == 0.  terms=True: returns (maps, X), X a list with one
    dict per level >= 1 of the float64 values before the rounding: "q" (N, R_l^2, 3), "Wt" (N, R_l^2), "B" (N, R_l^2, 3) = sum w |L|, and
    "on" (N, R^2), the sources' flags."""
    R, M = int(pr.resolution), int(pr.texels)
    s = np.asarray(sums, np.float32).astype(np.float64).reshape(-1, R * R, 4)
    n = s.shape[0]
    maps = np.zeros((n, M, 4), np.float32)
    X = []
    with np.errstate(all="ignore"):
        none = s[..., 3] == 0.0
        lv0 = np.where(none[..., None], 0.0, s[..., 0:3] / s[..., 3:4]).astype(np.float32)
        maps[:, :R * R, 0:3] = lv0
        maps[:, :R * R, 3] = np.where(none, 0.0, 1.0)
        L0 = lv0.astype(np.float64)
        for l in range(1, pr.levels):
            w, c, _den = probe_radiance_weights(pr, l)
            m = w.shape[0]
            A, B, Wt = np.zeros((n, m, 3)), np.zeros((n, m, 3)), np.zeros((n, m))
            for j in range(R * R):
                on = (~none[:, j])[:, None] & (c[None, :, j] > 0.0)                        # (n, m)
                term = w[None, :, j, None] * L0[:, None, j, :]
                Wt = np.where(on, Wt + w[None, :, j], Wt)
                A = np.where(on[..., None], A + term, A)
                B = np.where(on[..., None], B + np.abs(term), B)
            zero = Wt == 0.0
            q = np.where(zero[..., None], 0.0, A / np.where(zero, 1.0, Wt)[..., None])
            o = pr.offsets[l]
            maps[:, o:o + m, 0:3] = q.astype(np.float32)
            maps[:, o:o + m, 3] = np.where(zero, 0.0, 1.0)
            X.append({"q": q, "Wt": Wt, "B": B, "on": ~none})
    return (maps, X) if terms else maps


def probe_radiance_fetch(R: int, maps, dirs):
    """(M, 3) float64: the bilinear fetch of the header along the unit directions dirs (M, 3) from the level maps (M, R * R, 4) — one map
    per direction — edges clamped, the flags not read"""
    R = int(R)
    m = np.asarray(maps, np.float32).astype(np.float64).reshape(-1, R, R, 4)[..., 0:3]
    v = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    rows = np.arange(m.shape[0])
    with np.errstate(all="ignore"):
        s1 = (np.abs(x) + np.abs(y)) + np.abs(z)
        ox, oy = x / s1, y / s1
        fx, fy = (1.0 - np.abs(oy)) * _sgn1(ox), (1.0 - np.abs(ox)) * _sgn1(oy)
        ox, oy = np.where(z < 0.0, fx, ox), np.where(z < 0.0, fy, oy)
        top = float(R) - 1.0
        su = np.fmin(np.fmax(((ox + 1.0) * 0.5) * float(R) - 0.5, 0.0), top)
        sv = np.fmin(np.fmax(((oy + 1.0) * 0.5) * float(R) - 0.5, 0.0), top)
        iu, jv = np.fmin(np.floor(su), top - 1.0), np.fmin(np.floor(sv), top - 1.0)
        fu, fv = su - iu, sv - jv
        i, j = iu.astype(np.int64), jv.astype(np.int64)
        m00, m10, m01, m11 = m[rows, j, i], m[rows, j, i + 1], m[rows, j + 1, i], m[rows, j + 1, i + 1]
        gu, gv = (1.0 - fu)[:, None], (1.0 - fv)[:, None]
        return ((m00 * gu + m10 * fu[:, None]) * gv) + ((m01 * gu + m11 * fu[:, None]) * fv[:, None])


def probe_radiance_level(pr: "ProbeRadiance", roughness):
    """(l, t): the lower level of the pair a lookup at `roughness` (float64 array) blends, and the blend — rho clamped to the chain's
    range, l the largest level with rho_l <= rho capped at L - 2, t = (rho - rho_l) / (rho_(l+1) - rho_l); with one level (0, 0)"""
    rough = np.asarray(roughness, np.float64)
    rr = [float(np.float32(v)) for v in pr.roughness]
    if pr.levels == 1:
        return np.zeros(rough.shape, np.int64), np.zeros(rough.shape)
    rho = np.fmin(np.fmax(rough, rr[0]), rr[-1])
    l = np.zeros(rough.shape, np.int64)
    for k in range(1, pr.levels - 1):
        l = np.where(rr[k] <= rho, k, l)
    lo, hi = np.asarray(rr)[l], np.asarray(rr)[l + 1]
    return l, (rho - lo) / (hi - lo)


def probe_radiance_lookup(grid, pr: "ProbeRadiance", maps, positions, normals, dirs, roughness, pd: "ProbeDepth" = None, moments=None,
                          normal_bias: float = 0.0, placement=None, terms: bool = False):
    """The numpy float64 statement of fw_probe_radiance_lookup (include/firework_hip.h): the corner weights of probe_lookup_placed
    (placement None: every record (0, 0, 0, 1)), and per active corner the rgb of the level pair probe_radiance_level picks, each fetched
    bilinearly along r = dirs / |dirs| and blended m = m_l (1 - t) + m_(l+1) t (one level: m = m_0); Out_c = sum (w_d / wsum) m_c.  Zeros
    for a non-finite position, normal, dir or roughness, a zero normal or dir, no active corner or a zero weight sum.  maps (n, M, 4)
    float32.  terms=True: returns (E, T, X): T = sum |w_d| (|m_l| (1 - t) + |m_(l+1)| t) with the fetches taken of the texels'
    magnitudes, and X probe_lookup_placed's terms with "probe" (N, corners), "level" and "t" (N,)."""
    g = ProbeGrid.of(grid)
    M = int(pr.texels)
    mp = np.asarray(maps, np.float32).reshape(g.n_probes, M, 4)
    if placement is None:
        placement = np.tile(np.array([0.0, 0.0, 0.0, 1.0], np.float32), (g.n_probes, 1))
    p32 = np.asarray(positions, np.float32).reshape(-1, 3)
    n = p32.shape[0]
    _E, _T, X = probe_lookup_placed(g, np.zeros((g.n_probes, 9, 3), np.float32), placement, p32, normals, pd, moments, normal_bias, terms=True)
    dv = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    ro = np.asarray(roughness, np.float32).astype(np.float64).reshape(-1)
    p = p32.astype(np.float64)
    E, T = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        dl2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
        ok = np.all(np.isfinite(dv), axis=1) & np.isfinite(ro) & (dl2 > 0.0)
        r = dv / np.sqrt(dl2)[:, None]
        r = np.where(ok[:, None], r, (0.0, 0.0, 1.0))
        level, t = probe_radiance_level(pr, np.where(ok, ro, 0.0))
        pos = np.where(np.all(np.isfinite(p), axis=1)[:, None], p, 0.0)
        idx = []
        for k in range(3):
            c = g.counts[k]
            if c > 1:
                cm1 = float(c - 1)
                s = np.fmin(np.fmax(((pos[:, k] - g.lo[k]) / (g.hi[k] - g.lo[k])) * cm1, 0.0), cm1)
                idx.append(np.fmin(np.floor(s), cm1 - 1.0).astype(np.int64))
            else:
                idx.append(np.zeros(n, np.int64))
        two = [c > 1 for c in g.counts]
        corners = [(dx, dy, dz) for dz in range(2 if two[2] else 1) for dy in range(2 if two[1] else 1) for dx in range(2 if two[0] else 1)]
        probes = []
        for ci, d in enumerate(corners):
            probe = ((idx[2] + d[2]) * g.counts[1] + (idx[1] + d[1])) * g.counts[0] + (idx[0] + d[0])
            probes.append(probe)
            wd, on = X["w"][:, ci], X["active"][:, ci] & ok
            m, ma = np.zeros((n, 3)), np.zeros((n, 3))
            for l in range(pr.levels):
                Rl, o = pr.resolutions[l], pr.offsets[l]
                lower, upper = level == l, (level + 1 == l) & (pr.levels > 1)
                if not (lower.any() or upper.any()):
                    continue
                tex = mp[probe, o:o + Rl * Rl]
                f = probe_radiance_fetch(Rl, tex, r)
                fa = probe_radiance_fetch(Rl, np.abs(tex), r)
                if pr.levels == 1:
                    m, ma = f, fa
                else:
                    m = np.where(lower[:, None], f * (1.0 - t)[:, None], m)
                    ma = np.where(lower[:, None], fa * (1.0 - t)[:, None], ma)
                    m = np.where(upper[:, None], m + f * t[:, None], m)
                    ma = np.where(upper[:, None], ma + fa * t[:, None], ma)
            E = np.where(on[:, None], E + wd[:, None] * m, E)
            T = np.where(on[:, None], T + np.abs(wd)[:, None] * ma, T)
    some = ok & (np.abs(X["w"]).sum(axis=1) != 0.0)
    E[~some] = 0.0
    T[~some] = 0.0
    if not terms:
        return E
    X = dict(X)
    X["probe"], X["level"], X["t"] = np.stack(probes, axis=-1), level, t
    return E, T, X


def probe_glossy_ref(aov, spec, view, diffuse, radiance=None, *, grid=None, pr: "ProbeRadiance" = None, maps=None, pd: "ProbeDepth" = None,
                     moments=None, normal_bias: float = 0.0, placement=None):
    """The float32 statement of fw_probe_shade_glossy's linear output, (N, 3) float32: a pixel with !(rho > 0) takes `diffuse` (N, 3), the
    linear output of the placed shade of the same records; a glossy pixel is v (F Ls) + (1 - v) a with F_c = f0_c + (1 - f0_c) float32(S),
    S = ((m m)(m m)) m, m = 1 - min(1, max(0, -(nh.u))), u = view / |view|, and Ls = max(radiance, 0): the lookup along
    r = float32(u - (2 (nh.u)) nh) at rho, as probe_glossy_dirs returns it — `radiance` (N, 3) float32 when given (the device lookup's
    own output), else probe_radiance_lookup over grid, pr, maps and the optional terms.  Ls = 0 and S = 0 for an unusable view, normal
    or position."""
    a = np.asarray(aov, np.float32).reshape(-1, 12)
    sp = np.asarray(spec, np.float32).reshape(-1, 4)
    r, S, ok = probe_glossy_dirs(aov, view)
    if radiance is None:
        radiance = probe_radiance_lookup(grid, pr, maps, a[:, 8:11], a[:, 4:7], r, sp[:, 3], pd, moments, normal_bias, placement).astype(np.float32)
    with np.errstate(all="ignore"):
        Ls = np.asarray(radiance, np.float32).reshape(-1, 3)
        Ls = np.where(ok[:, None] & (Ls > 0), Ls, np.float32(0.0)).astype(np.float32)
        Sf = np.where(ok, S, 0.0).astype(np.float32)[:, None]
        f0, v, one = sp[:, 0:3], a[:, 3:4], np.float32(1.0)
        F = (f0 + (one - f0) * Sf).astype(np.float32)
        out = (v * (F * Ls) + (one - v) * a[:, 0:3]).astype(np.float32)
    glossy = sp[:, 3] > 0
    return np.where(glossy[:, None], out, np.asarray(diffuse, np.float32).reshape(-1, 3)).astype(np.float32)


def material_spec_table(desc: "SceneDesc") -> np.ndarray:
    """(n_materials + 1, 4) float32: fw_probe_shade_glossy's (F0.rgb, rho) of every material of a scene description — a GgxMat (albedo,
    roughness), a MetalMat (albedo, roughness clipped to [0.03, 1]), every other material zeros (rho = 0: diffuse) — and a last row of
    zeros for a miss"""
    n = int(desc.desc.n_materials)
    table = np.zeros((n + 1, 4), np.float32)
    for i in range(n):
        m = desc.materials[i]
        if m.kind in (A.FW_MAT_GGX, A.FW_MAT_METAL):
            rho = np.float32(m.roughness)
            if m.kind == A.FW_MAT_METAL:
                rho = np.float32(min(max(rho, np.float32(0.03)), np.float32(1.0)))
            table[i] = (m.albedo.x, m.albedo.y, m.albedo.z, rho)
    return table


def probe_glossy_dirs(aov, view):
    """(r, S, ok) of fw_probe_shade_glossy: r (N, 3) float32, the view direction mirrored about the record's unit normal; S (N,) float64,
    Schlick's weight; ok (N,), False where the view, the normal or the position is not finite or the view or the normal is zero (r is
    then (0, 0, 1) and S 0)"""
    a = np.asarray(aov, np.float32).reshape(-1, 12).astype(np.float64)
    vw = np.asarray(view, np.float32).astype(np.float64).reshape(-1, 3)
    nr = a[:, 4:7]
    with np.errstate(all="ignore"):
        nl2 = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        vl2 = (vw[:, 0] * vw[:, 0] + vw[:, 1] * vw[:, 1]) + vw[:, 2] * vw[:, 2]
        ok = (np.all(np.isfinite(a[:, 8:11]), axis=1) & np.all(np.isfinite(nr), axis=1) & np.all(np.isfinite(vw), axis=1) & (nl2 > 0.0)
              & (vl2 > 0.0))
        nh = nr / np.sqrt(nl2)[:, None]
        u = vw / np.sqrt(vl2)[:, None]
        c = (nh[:, 0] * u[:, 0] + nh[:, 1] * u[:, 1]) + nh[:, 2] * u[:, 2]
        r = (u - (2.0 * c)[:, None] * nh).astype(np.float32)
        m = 1.0 - np.fmin(1.0, np.fmax(0.0, -c))
        S = ((m * m) * (m * m)) * m
    return np.where(ok[:, None], r, np.float32([0.0, 0.0, 1.0])).astype(np.float32), np.where(ok, S, 0.0), ok


# --------------------------------------------------------------------------- the split sum's BRDF term: a GGX albedo table
class GgxTable:
    """The table of GgxMat's directional albedo that fw_probe_shade_split reads (fw_ggx_table): n_rho x n_mu texels of the two terms
    (A, B) of F0 A + B at the centres mu_i = (i + 0.5) / n_mu, rho_j = (j + 0.5) / n_rho, each integrated over m1 x m2 midpoints of the
    visible-normal square.  energy: shade with FW_SPLIT_ENERGY, the single-lobe energy compensation 1 + F0 (1 / (A + B) - 1)."""

    def __init__(self, n_mu: int = 64, n_rho: int = 64, m1: int = 128, m2: int = 128, energy: bool = False):
        self.n_mu, self.n_rho, self.m1, self.m2, self.energy = int(n_mu), int(n_rho), int(m1), int(m2), bool(energy)
        self.check()

    def check(self):
        if not (2 <= self.n_mu <= 256 and 2 <= self.n_rho <= 256):
            raise ValueError("n_mu and n_rho must be in 2..256")
        if not (1 <= self.m1 <= 1024 and 1 <= self.m2 <= 1024):
            raise ValueError("m1 and m2 must be in 1..1024")
        return self

    @property
    def flags(self) -> int:
        return A.FW_SPLIT_ENERGY if self.energy else 0

    def to_abi(self) -> A.fw_ggx_quad:
        return A.fw_ggx_quad(self.m1, self.m2)


def ggx_terms(mu, rho, m1: int = 128, m2: int = 128, terms: bool = False):
    """The numpy float64 statement of fw_ggx_terms: (n, 2) float32, the terms (A, B) of GgxMat's directional albedo F0 A + B at the
    float32 pairs (mu, rho), by the m1 x m2 midpoint rule over the visible-normal square in the kernel's order: lane l of 256 adds the
    samples l, l + 256, ... (id = a m2 + b), the partials go through the xor tree of each run of 64 and the four runs are added in
    order.  Zeros for a mu outside (0, 1], a rho outside [0, 1] or a NaN.  terms: also a dict with the float64 values before their one
    rounding ("AB", (n, 2)), the smallest |wi.z| over the samples ("min_wz", (n,)), the largest amplification of the one
    ill-conditioned step, 1 / (2 (1 - p1^2 - p2^2)) where the root's argument is positive ("amp", (n,)), and the number of samples
    whose argument is not positive ("clamped", (n,))."""
    m1, m2 = int(m1), int(m2)
    muf = np.asarray(mu, np.float32).reshape(-1)
    rhof = np.asarray(rho, np.float32).reshape(-1)
    n = muf.shape[0]
    with np.errstate(all="ignore"):
        ok = (muf > 0) & (muf <= 1) & (rhof >= 0) & (rhof <= 1)
        cm = np.where(ok, muf, np.float32(1.0)).astype(np.float64)[:, None]
        alpha = np.where(ok, rhof * rhof, np.float32(0.0)).astype(np.float64)[:, None]
        a2 = alpha * alpha
        sx = np.sqrt(np.fmax(1.0 - cm * cm, 0.0))
        vx = alpha * sx
        vl = np.sqrt(vx * vx + cm * cm)
        vhx, vhz = vx / vl, cm / vl
        s = 0.5 * (1.0 + vhz)
        s1 = 1.0 - s
        lo1 = 1.0 + 0.5 * (np.sqrt(1.0 + a2 * ((sx * sx) / (cm * cm))) - 1.0)
        sr = np.sqrt((np.arange(m1, dtype=np.float64) + 0.5) / float(m1))
        phi = (2.0 * np.pi) * ((np.arange(m2, dtype=np.float64) + 0.5) / float(m2))
        cphi, sphi = np.cos(phi), np.sin(phi)
        total = m1 * m2
        trips = (total + 255) // 256
        accA, accB = np.zeros((n, 256)), np.zeros((n, 256))
        min_wz, amp, clamped = np.full(n, np.inf), np.zeros(n), np.zeros(n, np.int64)
        for it in range(trips):
            raw = it * 256 + np.arange(256)
            valid = (raw < total)[None, :]
            ids = np.minimum(raw, total - 1)
            a, b = ids // m2, ids % m2
            r, cp, sp = sr[a][None, :], cphi[b][None, :], sphi[b][None, :]
            p1 = r * cp
            q1 = 1.0 - p1 * p1
            p2 = s1 * np.sqrt(np.fmax(q1, 0.0)) + s * (r * sp)
            arg = q1 - p2 * p2
            nz = np.sqrt(np.fmax(arg, 0.0))
            nhx, nhz = nz * vhx - p2 * vhz, p2 * vhx + nz * vhz
            gx, gy, gz = alpha * nhx, alpha * p1, np.fmax(nhz, 0.0)
            hl = np.sqrt((gx * gx + gy * gy) + gz * gz)
            hx, hy, hz = gx / hl, gy / hl, gz / hl
            oh = sx * hx + cm * hz
            t2 = 2.0 * oh
            wx, wy, wz = t2 * hx - sx, t2 * hy, t2 * hz - cm
            alive = wz > 0.0
            zz, xy = np.where(alive, wz, 1.0), np.where(alive, wx * wx + wy * wy, 0.0)
            li = 0.5 * (np.sqrt(1.0 + a2 * (xy / (zz * zz))) - 1.0)
            k = np.where(alive & valid, lo1 / (lo1 + li), 0.0)
            m = np.fmax(1.0 - oh, 0.0)
            fc = ((m * m) * (m * m)) * m
            accA = accA + k * (1.0 - fc)
            accB = accB + k * fc
            if terms:
                min_wz = np.minimum(min_wz, np.min(np.where(valid, np.abs(wz), np.inf), axis=1))
                amp = np.maximum(amp, np.max(np.where(valid & (arg > 0.0), 0.5 / np.where(arg > 0.0, arg, 1.0), 0.0), axis=1))
                clamped += np.sum(valid & ~(arg > 0.0), axis=1)

        def tree(v):
            v = v.reshape(n, 4, 64)
            lanes = np.arange(64)
            for d in (32, 16, 8, 4, 2, 1):
                v = v + v[:, :, lanes ^ d]
            w = v[:, :, 0]
            return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]

        count = float(m1) * float(m2)
        AB = np.stack([tree(accA) / count, tree(accB) / count], axis=1)
        AB = np.where(ok[:, None], AB, 0.0)
    out = AB.astype(np.float32)
    if terms:
        return out, {"AB": AB, "min_wz": np.where(ok, min_wz, np.inf), "amp": np.where(ok, amp, 0.0), "clamped": np.where(ok, clamped, 0), "ok": ok}
    return out


def ggx_table_centres(n_mu: int, n_rho: int):
    """(mu (n_rho, n_mu), rho (n_rho, n_mu)) float32: the texel centres of a GGX table, divided in float64 and rounded once"""
    mu = ((np.arange(int(n_mu), dtype=np.float64) + 0.5) / float(n_mu)).astype(np.float32)
    rho = ((np.arange(int(n_rho), dtype=np.float64) + 0.5) / float(n_rho)).astype(np.float32)
    return np.broadcast_to(mu[None, :], (int(n_rho), int(n_mu))).copy(), np.broadcast_to(rho[:, None], (int(n_rho), int(n_mu))).copy()


def ggx_table(n_mu: int = 64, n_rho: int = 64, m1: int = 128, m2: int = 128) -> np.ndarray:
    """The numpy statement of fw_ggx_table: (n_rho, n_mu, 2) float32, ggx_terms at the texel centres"""
    mu, rho = ggx_table_centres(n_mu, n_rho)
    return ggx_terms(mu.reshape(-1), rho.reshape(-1), m1, m2).reshape(int(n_rho), int(n_mu), 2)


def ggx_table_lookup(table, mu, rho) -> np.ndarray:
    """The numpy float64 statement of fw_ggx_table_lookup: (n, 2) float32, the bilinear lookup of an (n_rho, n_mu, 2) float32 table at
    the float32 pairs (mu, rho): x = min(max(mu n_mu - 0.5, 0), n_mu - 1), i0 = min(int(x), n_mu - 2), tx = x - i0, likewise y, and
    ((t00 (1 - tx) + t10 tx) (1 - ty)) + ((t01 (1 - tx) + t11 tx) ty), rounded once; zeros for a non-finite mu or rho"""
    t = np.asarray(table, np.float32)
    n_rho, n_mu = int(t.shape[0]), int(t.shape[1])
    t = t.astype(np.float64)
    muf = np.asarray(mu, np.float32).reshape(-1)
    rhof = np.asarray(rho, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(muf) & np.isfinite(rhof)
        x = np.fmin(np.fmax(np.where(ok, muf, 0).astype(np.float64) * float(n_mu) - 0.5, 0.0), float(n_mu) - 1.0)
        y = np.fmin(np.fmax(np.where(ok, rhof, 0).astype(np.float64) * float(n_rho) - 0.5, 0.0), float(n_rho) - 1.0)
        i0, j0 = np.minimum(x.astype(np.int64), n_mu - 2), np.minimum(y.astype(np.int64), n_rho - 2)
        tx, ty = (x - i0)[:, None], (y - j0)[:, None]
        ux, uy = 1.0 - tx, 1.0 - ty
        t00, t10, t01, t11 = t[j0, i0], t[j0, i0 + 1], t[j0 + 1, i0], t[j0 + 1, i0 + 1]
        out = ((t00 * ux + t10 * tx) * uy) + ((t01 * ux + t11 * tx) * ty)
        return np.where(ok[:, None], out, 0.0).astype(np.float32)


def probe_split_mu(aov, view) -> np.ndarray:
    """(N,) float32: fw_probe_shade_split's mu_f = float32(min(1, max(0, -(nh.u)))), and 0 for an unusable view, normal or position"""
    a = np.asarray(aov, np.float32).reshape(-1, 12).astype(np.float64)
    vw = np.asarray(view, np.float32).astype(np.float64).reshape(-1, 3)
    nr = a[:, 4:7]
    _r, _S, ok = probe_glossy_dirs(aov, view)
    with np.errstate(all="ignore"):
        nh = nr / np.sqrt((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2])[:, None]
        u = vw / np.sqrt((vw[:, 0] * vw[:, 0] + vw[:, 1] * vw[:, 1]) + vw[:, 2] * vw[:, 2])[:, None]
        c = (nh[:, 0] * u[:, 0] + nh[:, 1] * u[:, 1]) + nh[:, 2] * u[:, 2]
        return np.where(ok, np.fmin(1.0, np.fmax(0.0, -c)), 0.0).astype(np.float32)


def probe_split_ref(aov, spec, view, diffuse, radiance, terms=None, table=None, flags: int = 0) -> np.ndarray:
    """The float32 statement of fw_probe_shade_split's linear output, (N, 3) float32: a pixel with !(rho > 0) takes `diffuse` (N, 3), the
    linear output of the placed shade of the same records; a glossy pixel is v (spec Ls) + (1 - v) a with Ls = max(radiance, 0) — the
    lookup along probe_glossy_dirs' r at rho, (N, 3) float32, 0 for an unusable view, normal or position — spec_c = f0_c A + B and,
    with FW_SPLIT_ENERGY in flags, spec_c (1 + f0_c g), g = 1 / (A + B) - 1 where A + B > 0, else 0.  (A, B) = `terms` (N, 2) float32
    when given (the device lookup's own output), else ggx_table_lookup(table, probe_split_mu(aov, view), rho)."""
    a = np.asarray(aov, np.float32).reshape(-1, 12)
    sp = np.asarray(spec, np.float32).reshape(-1, 4)
    _r, _S, ok = probe_glossy_dirs(aov, view)
    if terms is None:
        terms = ggx_table_lookup(table, probe_split_mu(aov, view), sp[:, 3])
    ab = np.asarray(terms, np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        Ls = np.asarray(radiance, np.float32).reshape(-1, 3)
        Ls = np.where(ok[:, None] & (Ls > 0), Ls, np.float32(0.0)).astype(np.float32)
        f0, v, one = sp[:, 0:3], a[:, 3:4], np.float32(1.0)
        Af, Bf = ab[:, 0:1], ab[:, 1:2]
        s = (f0 * Af + Bf).astype(np.float32)
        if int(flags) & A.FW_SPLIT_ENERGY:
            e1 = (Af + Bf).astype(np.float32)
            g = np.where(e1 > 0, one / np.where(e1 > 0, e1, one) - one, np.float32(0.0)).astype(np.float32)
            s = (s * (one + f0 * g)).astype(np.float32)
        out = (v * (s * Ls) + (one - v) * a[:, 0:3]).astype(np.float32)
    glossy = sp[:, 3] > 0
    return np.where(glossy[:, None], out, np.asarray(diffuse, np.float32).reshape(-1, 3)).astype(np.float32)


# --------------------------------------------------------------------------- lightmaps (fw_bake_lightmap)
LIGHTMAP_NO_OWNER = 0xFFFFFFFF          # FW_NO_HIT in an owner map


def texel_jitter(seed: int, round: int, ids) -> np.ndarray:
    """(n, 2) float64 in [0, 1): pixel_jitter's hash with sample -> round and pixel -> the texel ids given (any subset, any order)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s32 = ((seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF
    key = _hash32(np.array([s32 ^ int(_hash32(np.array([(int(round) + 0x9E3779B9) & 0xFFFFFFFF], np.uint32))[0])], np.uint32))[0]
    ids = np.asarray(ids, np.uint64).reshape(-1)
    ctr = np.stack([2 * ids, 2 * ids + 1], axis=1).astype(np.uint32)
    bits = _hash32(_hash32(ctr) ^ key) >> np.uint32(8)
    return bits.astype(np.float64) * 2.0 ** -24


def rotor_rows(rot: "Rotor3") -> np.ndarray:
    """(3, 3) float32: the rotation matrix of a rotor as the tracer forms it (ultraviolet's Rotor3::into_matrix, float32, this order)"""
    s, xy, xz, yz = (F32(v) for v in (rot.s, rot.xy, rot.xz, rot.yz))
    two = F32(2.0)
    s2, bxy2, bxz2, byz2 = s * s, xy * xy, xz * xz, yz * yz
    s_bxy, s_bxz, s_byz = s * xy, s * xz, s * yz
    bxz_byz, bxy_byz, bxy_bxz = xz * yz, xy * yz, xy * xz
    c0 = [s2 - bxy2 - bxz2 + byz2, -two * (bxz_byz + s_bxy), two * (bxy_byz - s_bxz)]
    c1 = [two * (s_bxy - bxz_byz), s2 - bxy2 + bxz2 - byz2, -two * (s_byz + bxy_bxz)]
    c2 = [two * (s_bxz + bxy_byz), two * (s_byz - bxy_bxz), s2 + bxy2 - bxz2 - byz2]
    return np.array([[c0[i], c1[i], c2[i]] for i in range(3)], F32)


def _edge(au, av, bu, bv, pu, pv):
    return (bu - au) * (pv - av) - (bv - av) * (pu - au)


def lightmap_reduce(accum, samples: int, directions: int) -> np.ndarray:
    """The float64 statement of fw_lightmap_reduce's projection: (n, 3) with proj[q][c] = (pi / D) sum_j accum[q D + j][c] / samples, for
    accum (n * D, 4) (r, g, b sums, then segments).  The device rounds it to float32 once and adds it to the texel's running sum."""
    D = int(directions)
    a = np.asarray(accum, np.float64).reshape(-1, D, 4)[..., :3] / float(samples)
    return (np.pi / D) * a.sum(axis=1)


_DILATE_ORDER = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))      # (dy, dx)


def lightmap_dilate(image, passes: int) -> np.ndarray:
    """The float32 statement of fw_lightmap_dilate: image (H, W, 4) (rgb, a).  Per pass a texel with a > 0 is copied; a texel with a == 0
    whose in-image neighbours, in the order (dy, dx) = (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1), include n >= 1 with
    a > 0 takes their float32 sum in that order divided by float32(n), and a = 0.5; otherwise it is unchanged.  No wrap-around."""
    img = np.array(image, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image must have shape (H, W, 4)")
    h, w = img.shape[:2]
    for _ in range(int(passes)):
        pad = np.zeros((h + 2, w + 2, 4), np.float32)
        pad[1:-1, 1:-1] = img
        total = np.zeros((h, w, 3), np.float32)
        count = np.zeros((h, w), np.int64)
        for dy, dx in _DILATE_ORDER:
            v = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            on = v[..., 3] > 0
            total = np.where(on[..., None], total + v[..., :3], total)
            count += on
        fill = ~(img[..., 3] > 0) & (count > 0)
        out = img.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            out[..., :3] = np.where(fill[..., None], total / count.astype(np.float32)[..., None], img[..., :3])
        out[..., 3] = np.where(fill, np.float32(0.5), img[..., 3])
        img = out
    return img


class Lightmap:
    """A lightmap (fw_lightmap): irradiance over the UV texels of one placed TriangleMesh.  Lightmap(mesh, width, height,
    directions=64), then .placement(render_object) or Lightmap.of(scene, object_index, w, h), and .seed(s) / .jitter(on) / .bias(b) /
    .flip(on) as builders.  .texels(), .covered() and .rays(round) are the numpy float64 statements of what the device computes;
    _lib.lightmap_texels / _lib.lightmap_rays the device's own.  Texel (x, y), row 0 at the top, id = y W + x, has its centre at
    u = (x + 1/2) / W, v = 1 - (y + 1/2) / H: ImageTexture's lookup inverted."""

    def __init__(self, mesh: "TriangleMesh", width: int, height: int, directions: int = 64):
        if not isinstance(mesh, TriangleMesh):
            raise ValueError("a lightmap needs a TriangleMesh")
        if mesh.uvs is None:
            raise ValueError("a lightmap needs a mesh with uvs")
        self.mesh = mesh
        self.width, self.height, self.directions = int(width), int(height), int(directions)
        self._position = np.zeros(3, F32)
        self.rotation = Rotor3.identity()
        self._flip_normals = False
        self._seed, self._jitter, self._bias, self._flip, self.chunk_texels = 0, True, 1e-3, False, 0
        self._texels = None

    def placement(self, obj: "RenderObject"):
        """takes position, rotation and flip_normals from a RenderObject"""
        self._position, self.rotation, self._flip_normals = _v3(obj._position), obj.rotation, bool(obj._flip_normals)
        self._texels = None
        return self

    @staticmethod
    def of(scene, object_index: int, width: int, height: int, directions: int = 64) -> "Lightmap":
        """the lightmap of object `object_index` of a Scene, which must be a TriangleMesh with uvs (ValueError otherwise)"""
        objs = scene.render_objects
        if not 0 <= int(object_index) < len(objs):
            raise ValueError(f"object {object_index} does not exist: the scene has {len(objs)} objects")
        ro = objs[int(object_index)]
        if not isinstance(ro.obj, TriangleMesh) or ro.obj.uvs is None:
            raise ValueError(f"object {object_index} is not a triangle mesh with uvs ({type(ro.obj).__name__})")
        return Lightmap(ro.obj, width, height, directions).placement(ro)

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def bias(self, b):
        self._bias = float(b)
        return self

    def flip(self, on=True):
        self._flip = bool(on)
        self._texels = None
        return self

    def centres(self):
        """(u, v) float64 arrays of shape (W * H,): the texel centres in texel-id order"""
        w, h = self.width, self.height
        if w < 1 or h < 1:
            raise ValueError("width and height must be >= 1")
        y, x = np.divmod(np.arange(w * h, dtype=np.int64), w)
        return (x + 0.5) / float(w), 1.0 - (y + 0.5) / float(h)

    def texels(self):
        """the numpy statement of fw_lightmap_texels: (records (W * H, 8) float32, owner (W * H,) uint32).  Coverage: the float64 edge
        functions e(A, B; P) = (B_u - A_u)(P_v - A_v) - (B_v - A_v)(P_u - A_u) of the float32 uvs at the texel centre all >= 0 or all
        <= 0, zero-area triangles skipped, lowest triangle index first.  Records: float64 barycentrics, (b0 p0 + b1 p1) + b2 p2, the
        normalised interpolated (or geometric, (p0 - p2) x (p1 - p2)) normal, the placement's transform, one rounding."""
        if self._texels is not None:
            return self._texels
        m = self.mesh
        n = self.width * self.height
        pu, pv = self.centres()
        uv = m.uvs.astype(np.float64)
        idx = m.indicies.reshape(-1, 3).astype(np.int64)
        owner = np.full(n, LIGHTMAP_NO_OWNER, np.uint32)
        for t, (i0, i1, i2) in enumerate(idx):
            (au, av), (bu, bv), (cu, cv) = uv[i0], uv[i1], uv[i2]
            if _edge(au, av, bu, bv, cu, cv) == 0.0:
                continue
            e0, e1, e2 = _edge(au, av, bu, bv, pu, pv), _edge(bu, bv, cu, cv, pu, pv), _edge(cu, cv, au, av, pu, pv)
            inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
            owner[inside & (owner == LIGHTMAP_NO_OWNER)] = t
        rec = np.zeros((n, 8), np.float32)
        cov = np.nonzero(owner != LIGHTMAP_NO_OWNER)[0]
        if cov.size:
            tri = idx[owner[cov].astype(np.int64)]
            a, b, c = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
            P = (pu[cov], pv[cov])
            area = _edge(a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
            b0 = (_edge(b[:, 0], b[:, 1], c[:, 0], c[:, 1], *P) / area)[:, None]
            b1 = (_edge(c[:, 0], c[:, 1], a[:, 0], a[:, 1], *P) / area)[:, None]
            b2 = (_edge(a[:, 0], a[:, 1], b[:, 0], b[:, 1], *P) / area)[:, None]
            v = m.verts.astype(np.float64)
            p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
            pos = (b0 * p0 + b1 * p1) + b2 * p2
            if m.normals is not None:
                nv = m.normals.astype(np.float64)
                nrm = (b0 * nv[tri[:, 0]] + b1 * nv[tri[:, 1]]) + b2 * nv[tri[:, 2]]
            else:
                ea, eb = p0 - p2, p1 - p2
                nrm = np.stack([ea[:, 1] * eb[:, 2] - ea[:, 2] * eb[:, 1], ea[:, 2] * eb[:, 0] - ea[:, 0] * eb[:, 2],
                                ea[:, 0] * eb[:, 1] - ea[:, 1] * eb[:, 0]], axis=1)
            with np.errstate(all="ignore"):
                length = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
                nrm = nrm / length[:, None]
                rows = rotor_rows(self.rotation)
                if F32(0.5) * ((rows[0, 0] + rows[1, 1] + rows[2, 2]) - F32(1.0)) < F32(0.999):
                    R = rows.astype(np.float64)
                    pos = np.stack([(R[k, 0] * pos[:, 0] + R[k, 1] * pos[:, 1]) + R[k, 2] * pos[:, 2] for k in range(3)], axis=1)
                    nrm = np.stack([(R[k, 0] * nrm[:, 0] + R[k, 1] * nrm[:, 1]) + R[k, 2] * nrm[:, 2] for k in range(3)], axis=1)
                pos = pos + self._position.astype(np.float64)
                if self._flip_normals != self._flip:
                    nrm = -nrm
                both = np.concatenate([pos, nrm], axis=1).astype(np.float32)
            ok = (length > 0) & np.isfinite(length) & np.all(np.isfinite(both), axis=1)
            rec[cov[ok], 0:3] = both[ok, 0:3]
            rec[cov[ok], 4:7] = both[ok, 3:6]
            owner[cov[~ok]] = LIGHTMAP_NO_OWNER
        rec[:, 3] = owner.view(np.float32)
        self._texels = (rec, owner)
        return self._texels

    def covered(self) -> np.ndarray:
        """the covered list: the ascending texel ids with an owner, uint32"""
        return np.nonzero(self.texels()[1] != LIGHTMAP_NO_OWNER)[0].astype(np.uint32)

    def shifts(self, round: int, ids) -> np.ndarray:
        """(n, 2) float64: the shift (xi_u, xi_v) of the texel ids given in `round`"""
        ids = np.asarray(ids).reshape(-1)
        return texel_jitter(self._seed, round, ids) if self._jitter else np.full((ids.size, 2), 0.5)

    def rays(self, round: int, first: int = 0, n=None, device=None):
        """the numpy statement of one round's rays of the entries [first, first + n) of the covered list: (n * D, 6) float32, entry
        q * D + j = direction j of covered texel q (device: see panorama_rays).  In float64, rounded once: u = (j + xi_u) / D, r = sqrt u,
        c = sqrt(max(0, 1 - u)), t = j g + xi_v, phi = 2 pi (t - floor t), l = (r cos phi, r sin phi, c), rotated into Duff et al.'s basis
        around n = the record's float32 normal divided by its float64 length; origin = position + bias * n (bias 0: the position's bits)."""
        D = self.directions
        if D < 1:
            raise ValueError("directions must be >= 1")
        ids = self.covered()
        ids = ids[int(first):] if n is None else ids[int(first):int(first) + int(n)]
        rec = self.texels()[0][ids.astype(np.int64)]
        pos, nrm = rec[:, None, 0:3].astype(np.float64), rec[:, None, 4:7].astype(np.float64)
        xi = self.shifts(round, ids)
        j = np.arange(D, dtype=np.float64)[None, :]
        u = (j + xi[:, 0:1]) / float(D)
        r = np.sqrt(u)
        c = np.sqrt(np.maximum(0.0, 1.0 - u))
        g = (np.sqrt(5.0) - 1.0) / 2.0
        t = j * g + xi[:, 1:2]
        phi = (2.0 * np.pi) * (t - np.floor(t))
        lx, ly = r * np.cos(phi), r * np.sin(phi)
        nrm = nrm / np.sqrt((nrm[..., 0:1] * nrm[..., 0:1] + nrm[..., 1:2] * nrm[..., 1:2]) + nrm[..., 2:3] * nrm[..., 2:3])
        nx, ny, nz = nrm[..., 0], nrm[..., 1], nrm[..., 2]
        s = np.copysign(1.0, nz)
        a = -1.0 / (s + nz)
        b = (nx * ny) * a
        T = (1.0 + (s * (nx * nx)) * a, s * b, -s * nx)
        B = (b, s + (ny * ny) * a, -ny)
        d = np.stack([(lx * T[k] + ly * B[k]) + c * nrm[..., k] for k in range(3)], axis=-1).reshape(-1, 3)
        if self._bias == 0.0:
            o = np.repeat(rec[:, 0:3], D, axis=0).astype(np.float64)
        else:
            o = np.repeat((pos + float(F32(self._bias)) * nrm)[:, 0], D, axis=0)
        return _rays_out(o, d, device)

    def to_abi(self):
        """(fw_lightmap, the arrays it points into: keep them alive as long as the struct is used)"""
        m = self.mesh
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        s = A.fw_lightmap()
        s.verts, s.n_verts = m.verts.ctypes.data_as(fp), m.verts.shape[0]
        s.indices, s.n_indices = m.indicies.ctypes.data_as(up), m.indicies.shape[0]
        s.normals = m.normals.ctypes.data_as(fp) if m.normals is not None else None
        s.uvs = m.uvs.ctypes.data_as(fp)
        s.position, s.rotation, s.flip_normals = A.vec3(self._position), self.rotation.to_abi(), int(self._flip_normals)
        s.width, s.height, s.directions, s.jitter = self.width, self.height, self.directions, int(self._jitter)
        s.seed, s.bias, s.flip, s.chunk_texels = self._seed & 0xFFFFFFFFFFFFFFFF, self._bias, int(self._flip), int(self.chunk_texels)
        return s, (m.verts, m.indicies, m.normals, m.uvs)


# --------------------------------------------------------------------------- ambient occlusion (fw_bake_ao)
class AmbientOcclusion:
    """Ambient occlusion and bent normals of surface points (fw_ao): `directions` cosine-weighted hemisphere rays per
    point and round, a hit closer than `radius` occludes (falloff 0: fully; falloff 1: by 1 - dist / radius), origins moved `bias` along
    the normal.  radius may be inf with falloff 0: any hit occludes.  .seed(s) / .jitter(on) as builders; chunk_points as fw_ao's."""

    def __init__(self, radius: float, directions: int = 64, falloff: int = 0, bias: float = 1e-3):
        self.radius, self.directions, self.falloff, self.bias = float(np.float32(radius)), int(directions), int(falloff), float(np.float32(bias))
        self._seed, self._jitter, self.chunk_points = 0, True, 0

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def check(self):
        """what fw_ao_rays rejects in a description, as a ValueError, in its order"""
        if not 1 <= self.directions <= 1 << 20:
            raise ValueError("directions must be in 1..2^20")
        if self.falloff not in (0, 1):
            raise ValueError("falloff must be 0 or 1")
        if not self.radius > 0.0:
            raise ValueError("radius must be > 0")
        if np.isinf(self.radius) and self.falloff:
            raise ValueError("an infinite radius needs falloff 0")
        if not (np.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError("bias must be finite and >= 0")
        return self

    def to_abi(self) -> A.fw_ao:
        a = A.fw_ao()
        a.directions, a.falloff, a.radius, a.bias = self.directions & 0xFFFFFFFF, self.falloff & 0xFFFFFFFF, self.radius, self.bias
        a.jitter, a.chunk_points, a.seed = int(self._jitter), int(self.chunk_points), self._seed & 0xFFFFFFFFFFFFFFFF
        return a


def ao_usable(positions, normals) -> np.ndarray:
    """(M,) bool: the points fw_ao_rays generates rays for — every component finite and a normal other than (0, 0, 0)"""
    p, n = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    return np.all(np.isfinite(p), axis=1) & np.all(np.isfinite(n), axis=1) & np.any(n != 0, axis=1)


def ao_rays(ao: "AmbientOcclusion", positions, normals, ids=None, round: int = 0, device=None):
    """The numpy statement of fw_ao_rays: (n * D, 6) float32, entry q * D + j = direction j of point id = ids[q] (ids None: q) of
    positions and normals, (M, 3) float32 each (device: see panorama_rays).  Lightmap.rays' statement with the texel id replaced by id;
    an unusable point (ao_usable) gets D all-zero rays."""
    D = ao.directions
    if D < 1:
        raise ValueError("directions must be >= 1")
    P, Nn = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    ids = np.arange(P.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    at = ids.astype(np.int64)
    p32, n32 = P[at], Nn[at]
    ok = ao_usable(p32, n32)
    pos, nrm = p32[:, None, :].astype(np.float64), n32[:, None, :].astype(np.float64)
    xi = texel_jitter(ao._seed, round, ids) if ao._jitter else np.full((ids.size, 2), 0.5)
    j = np.arange(D, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        u = (j + xi[:, 0:1]) / float(D)
        r = np.sqrt(u)
        c = np.sqrt(np.maximum(0.0, 1.0 - u))
        g = (np.sqrt(5.0) - 1.0) / 2.0
        t = j * g + xi[:, 1:2]
        phi = (2.0 * np.pi) * (t - np.floor(t))
        lx, ly = r * np.cos(phi), r * np.sin(phi)
        nrm = nrm / np.sqrt((nrm[..., 0:1] * nrm[..., 0:1] + nrm[..., 1:2] * nrm[..., 1:2]) + nrm[..., 2:3] * nrm[..., 2:3])
        nx, ny, nz = nrm[..., 0], nrm[..., 1], nrm[..., 2]
        s = np.copysign(1.0, nz)
        a = -1.0 / (s + nz)
        b = (nx * ny) * a
        T = (1.0 + (s * (nx * nx)) * a, s * b, -s * nx)
        B = (b, s + (ny * ny) * a, -ny)
        d = np.stack([(lx * T[k] + ly * B[k]) + c * nrm[..., k] for k in range(3)], axis=-1)
        if ao.bias == 0.0:
            o = np.repeat(p32, D, axis=0).astype(np.float64)
        else:
            o = np.repeat((pos + float(F32(ao.bias)) * nrm)[:, 0], D, axis=0)
    d = np.where(ok[:, None, None], d, 0.0).reshape(-1, 3)
    o = np.where(np.repeat(ok, D)[:, None], o, 0.0)
    return _rays_out(o, d, device)


def ao_reduce(ao: "AmbientOcclusion", rays, hits_t, hits_object, terms: bool = False):
    """The numpy float64 statement of fw_ao_reduce: (n, 4) float64, (1 / D) x the accumulators (Bx, By, Bz, O) of one round before their
    one rounding to float32, for rays (n * D, 6) float32 (the directions as stored) and the hits' t (float32) and object (uint32,
    0xFFFFFFFF = miss) columns, summed in the device's order (G partial sums, an xor butterfly).  terms=True: returns (sums, T, dist)
    with T (n, 4) = (1 / D) sum_j |term_j| (what a rounding-error bound of the sums scales with) and dist (n, D) the distances."""
    D = int(ao.directions)
    d = np.asarray(rays, np.float32).astype(np.float64).reshape(-1, D, 6)[..., 3:]
    t = np.asarray(hits_t, np.float32).astype(np.float64).reshape(-1, D)
    miss = np.asarray(hits_object).astype(np.uint32).reshape(-1, D) == np.uint32(0xFFFFFFFF)
    radius = float(np.float32(ao.radius))
    G = 1
    while G < min(D, 64):
        G *= 2
    with np.errstate(all="ignore"):
        zero = np.all(d == 0.0, axis=-1)
        dist = t * np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        o = np.where(miss | (dist >= radius), 0.0, (1.0 - dist / radius) if ao.falloff else 1.0)
        w = 1.0 - o
        term = np.stack([w * d[..., 0], w * d[..., 1], w * d[..., 2], o], axis=-1)          # (n, D, 4)
        term = np.where(zero[..., None], 0.0, term)
    rows = -(-D // G)                                                                        # lane l takes j = l, l + G, ... in ascending order
    padded = np.zeros((d.shape[0], rows * G, 4))
    padded[:, :D] = term
    part = np.zeros((d.shape[0], G, 4))
    for row in padded.reshape(-1, rows, G, 4).transpose(1, 0, 2, 3):
        part = part + row
    m = G // 2
    while m >= 1:
        part = part + part[:, np.arange(G) ^ m]
        m //= 2
    out = (1.0 / D) * part[:, 0]
    if not terms:
        return out
    return out, (1.0 / D) * np.abs(term).sum(axis=1), np.where(zero, np.nan, dist)


def ao_resolve(sums, rounds: int) -> np.ndarray:
    """The statement of k_ao_resolve: (..., 4) float32 (bent.xyz, ao) from the float32 running sums (..., 4) of `rounds` rounds:
    ao = float32(min(1, max(0, 1 - O / rounds))), bent = B / sqrt((Bx Bx + By By) + Bz Bz) in float64, rounded once; (0, 0, 0) where that
    length is 0 or not finite."""
    s = np.asarray(sums, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2])
        ok = (length > 0.0) & np.isfinite(length)
        bent = np.where(ok[..., None], s[..., 0:3] / length[..., None], 0.0)
        occ = np.fmin(1.0, np.fmax(0.0, 1.0 - s[..., 3] / float(rounds)))
        return np.concatenate([bent, occ[..., None]], axis=-1).astype(np.float32)


# --------------------------------------------------------------------------- final gather (fw_bake_gather)
class FinalGather:
    """One bounce of gather rays lit from baked probes (fw_gather): `directions` cosine-weighted hemisphere rays per point
    and round, origins moved `bias` along the normal; each ray brings back the emission of the emitter it hit, the environment where it
    missed, or hit albedo x E(hit) / pi with E from the probes at the hit.  direct=True adds the scene's point, spot and directional
    lights at the gather hits, their shadow rays moved direct_bias along the hit's normal.  no_lights=True (FW_GATHER_NO_LIGHTS) is the
    complement of an AreaLight: a ray that hits one of the scene's sampled area lights brings back nothing; no_emitters=True
    (FW_GATHER_NO_EMITTERS) is the complement of an EmitterLights: the same for every object with an emitter entry (the two exclude each
    other).  .seed(s) / .jitter(on) as builders; chunk_points as fw_gather's."""

    def __init__(self, directions: int = 64, bias: float = 1e-3, direct: bool = False, direct_bias: float = 1e-3, no_lights: bool = False,
                 no_emitters: bool = False):
        self.directions, self.bias, self.direct, self.direct_bias = int(directions), float(np.float32(bias)), bool(direct), float(np.float32(direct_bias))
        self.no_lights, self.no_emitters = bool(no_lights), bool(no_emitters)
        self._seed, self._jitter, self.chunk_points = 0, True, 0

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def check(self):
        """what fw_bake_gather rejects in a description, as a ValueError, in its order"""
        if not 1 <= self.directions <= 1 << 20:
            raise ValueError("directions must be in 1..2^20")
        if not (np.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError("bias must be finite and >= 0")
        if not (np.isfinite(self.direct_bias) and self.direct_bias >= 0.0):
            raise ValueError("direct_bias must be finite and >= 0")
        return self

    def ao(self) -> "AmbientOcclusion":
        """the AmbientOcclusion whose rays the gather rays are, bit for bit"""
        return AmbientOcclusion(float("inf"), self.directions, 0, self.bias).seed(self._seed).jitter(self._jitter)

    def to_abi(self) -> A.fw_gather:
        g = A.fw_gather()
        g.directions, g.jitter, g.bias, g.direct_bias = self.directions & 0xFFFFFFFF, int(self._jitter), self.bias, self.direct_bias
        g.flags = (A.FW_GATHER_DIRECT if self.direct else 0) | (A.FW_GATHER_NO_LIGHTS if getattr(self, "no_lights", False) else 0)
        g.flags |= A.FW_GATHER_NO_EMITTERS if getattr(self, "no_emitters", False) else 0
        g.chunk_points, g.seed = int(self.chunk_points), self._seed & 0xFFFFFFFFFFFFFFFF
        return g


def surface_facing(normal, direction) -> np.ndarray:
    """The float32 statement of a surface record's normal (fw_hit_surface): n / len(n) with len(n) = sqrt((x x + y y) + z z), (0, 0, 0)
    where that length is 0, negated where (nx dx + ny dy) + nz dz > 0 on the hit's normal and the ray's direction as stored: (..., 3)
    float32, every operation rounded to float32 as written."""
    n, d = np.asarray(normal, np.float32), np.asarray(direction, np.float32)
    with np.errstate(all="ignore"):
        length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2], dtype=np.float32)
        unit = np.where((length == 0)[..., None], np.float32(0), n / length[..., None]).astype(np.float32)
        away = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2] > 0
    return np.where(away[..., None], -unit, unit).astype(np.float32)


def gather_reduce(surface, irradiance, directions: int, direct=None) -> np.ndarray:
    """The numpy float64 statement of fw_gather_reduce: (n, 4) float64, (pi / D) x the accumulators L.rgb and (1 / D) x sky of one round
    before their one rounding to float32, for surface (n * D, 16) float32 records, irradiance (n * D, 3) float32 and direct (n * D, 8)
    float32 or None, summed in the device's order (G partial sums, an xor butterfly)."""
    D = int(directions)
    s = np.asarray(surface, np.float32).astype(np.float64).reshape(-1, D, 16)
    E = np.asarray(irradiance, np.float32).astype(np.float64).reshape(-1, D, 3)
    n = s.shape[0]
    kind = s[..., 3]
    T = np.where(E > 0.0, E, 0.0)
    if direct is not None:
        T = T + np.asarray(direct, np.float32).astype(np.float64).reshape(-1, D, 8)[..., 0:3]
    inv_pi = 1.0 / 3.141592653589793
    with np.errstate(all="ignore"):
        L = (s[..., 0:3] * T) * inv_pi
    emits = (kind == -1.0) | (kind == 3.0)
    L = np.where(emits[..., None], s[..., 12:15], L)
    term = np.concatenate([L, (kind == -1.0)[..., None].astype(np.float64)], axis=-1)       # (n, D, 4)
    live = kind != -2.0
    G = 1
    while G < min(D, 64):
        G *= 2
    rows = -(-D // G)                                                                        # lane l takes j = l, l + G, ... in ascending order
    padded = np.zeros((n, rows * G, 4))
    padded[:, :D] = term
    take = np.zeros((n, rows * G), bool)
    take[:, :D] = live
    part = np.zeros((n, G, 4))
    with np.errstate(all="ignore"):
        for row, on in zip(padded.reshape(n, rows, G, 4).transpose(1, 0, 2, 3), take.reshape(n, rows, G).transpose(1, 0, 2)):
            part = np.where(on[..., None], part + row, part)                                 # (a ray that contributes nothing adds nothing: -0 and NaN stay out)
        m = G // 2
        while m >= 1:
            part = part + part[:, np.arange(G) ^ m]
            m //= 2
        return np.concatenate([(3.141592653589793 / D) * part[:, 0, 0:3], (1.0 / D) * part[:, 0, 3:4]], axis=-1)


def gather_resolve(sums, rounds: int) -> np.ndarray:
    """The statement of k_gather_resolve: (..., 4) float32 (E.rgb, sky) = float32(sums / rounds) from the float32 running sums."""
    with np.errstate(all="ignore"):
        return (np.asarray(sums, np.float32).astype(np.float64) / float(rounds)).astype(np.float32)


# --------------------------------------------------------------------------- reflection gather (fw_bake_reflect)
class ReflectionGather:
    """GGX-sampled reflection rays lit from baked probes (fw_reflect): `directions` rays per glossy point and round, drawn
    from the visible-normal lobe of the point's (F0, rho) around its view direction, origins moved `bias` along the normal facing the
    eye; each ray brings back what a gather ray brings back (FinalGather) and is summed with the estimator's weight F G2 / G1.
    .direct_bias(b) adds the scene's point, spot and directional lights at the hits, their shadow rays moved b along the hit's normal
    (.direct_bias(None) takes them out again).  .bias(b) / .seed(s) / .jitter(on) as builders; chunk_points as fw_reflect's."""

    def __init__(self, directions: int = 16):
        self.directions = int(directions)
        self._bias, self.direct, self._direct_bias = float(np.float32(1e-3)), False, float(np.float32(1e-3))
        self._seed, self._jitter, self.chunk_points = 0, True, 0

    def bias(self, b):
        self._bias = float(np.float32(b))
        return self

    def direct_bias(self, b):
        self.direct = b is not None
        if b is not None:
            self._direct_bias = float(np.float32(b))
        return self

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def check(self):
        """what fw_bake_reflect rejects in a description, as a ValueError, in its order"""
        if not 1 <= self.directions <= 1 << 20:
            raise ValueError("directions must be in 1..2^20")
        if not (np.isfinite(self._bias) and self._bias >= 0.0):
            raise ValueError("bias must be finite and >= 0")
        if not (np.isfinite(self._direct_bias) and self._direct_bias >= 0.0):
            raise ValueError("direct_bias must be finite and >= 0")
        return self

    def to_abi(self) -> A.fw_reflect:
        g = A.fw_reflect()
        g.directions, g.jitter, g.bias, g.direct_bias = self.directions & 0xFFFFFFFF, int(self._jitter), self._bias, self._direct_bias
        g.flags, g.chunk_points, g.seed = (A.FW_REFLECT_DIRECT if self.direct else 0), int(self.chunk_points), self._seed & 0xFFFFFFFFFFFFFFFF
        return g


def reflect_usable(positions, normals, view, spec) -> np.ndarray:
    """(M,) bool: the points fw_reflect_rays generates rays for — position, normal and view finite, normal and view other than
    (0, 0, 0), rho = spec[:, 3] finite and > 0"""
    p, n = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    v, rho = np.asarray(view, np.float32).reshape(-1, 3), np.asarray(spec, np.float32).reshape(-1, 4)[:, 3]
    with np.errstate(all="ignore"):
        return (np.all(np.isfinite(p), axis=1) & np.all(np.isfinite(n), axis=1) & np.all(np.isfinite(v), axis=1) & np.any(n != 0, axis=1)
                & np.any(v != 0, axis=1) & np.isfinite(rho) & (rho > 0))


def reflect_rays(reflect: "ReflectionGather", positions, normals, view, spec, ids=None, round: int = 0, device=None, terms: bool = False):
    """The numpy float64 statement of fw_reflect_rays: (rays (n * D, 6) float32, weights (n * D, 2) float32), entry q * D + j = ray j of
    point id = ids[q] (ids None: q) of positions, normals, view, (M, 3) float32 each, and spec (M, 4) float32 (F0.rgb, rho); weights =
    (g, s) with g = G2 / G1 and s = (1 - wo.h)^5 (device: see panorama_rays; it moves the rays only).  An unusable point
    (reflect_usable) gets D all-zero rays and weights, a dead ray (wi.z <= 0 or wo.z <= 0 in the point's frame) the same.  terms=True:
    also a dict with the float64 "wi_z" and "wo_z" (n, D) of every ray and "usable" (n,)."""
    D = reflect.directions
    if D < 1:
        raise ValueError("directions must be >= 1")
    P, Nn = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    V, Sp = np.asarray(view, np.float32).reshape(-1, 3), np.asarray(spec, np.float32).reshape(-1, 4)
    ids = np.arange(P.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    at = ids.astype(np.int64)
    p32, n32, v32, rho32 = P[at], Nn[at], V[at], Sp[at, 3]
    ok = reflect_usable(p32, n32, v32, Sp[at])
    xi = texel_jitter(reflect._seed, round, ids) if reflect._jitter else np.full((ids.size, 2), 0.5)
    j = np.arange(D, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        xi1 = (j + xi[:, 0:1]) / float(D)
        t = j * ((np.sqrt(5.0) - 1.0) / 2.0) + xi[:, 1:2]
        xi2 = t - np.floor(t)
        alpha = (rho32 * rho32).astype(np.float64)[:, None]                                  # the float32 product, widened
        a2 = alpha * alpha
        # the frame: the normal made unit in float64, wo = -view / |view|, the normal flipped towards wo, Duff's basis
        r, vw = n32.astype(np.float64), v32.astype(np.float64)
        rl = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        vl = np.sqrt((vw[:, 0] * vw[:, 0] + vw[:, 1] * vw[:, 1]) + vw[:, 2] * vw[:, 2])
        nx, ny, nz = r[:, 0] / rl, r[:, 1] / rl, r[:, 2] / rl
        wx, wy, wz = -(vw[:, 0] / vl), -(vw[:, 1] / vl), -(vw[:, 2] / vl)
        away = (wx * nx + wy * ny) + wz * nz < 0.0
        nx, ny, nz = np.where(away, -nx, nx), np.where(away, -ny, ny), np.where(away, -nz, nz)
        s = np.copysign(1.0, nz)
        a = -1.0 / (s + nz)
        b = (nx * ny) * a
        T = (1.0 + (s * (nx * nx)) * a, s * b, -s * nx)
        B = (b, s + (ny * ny) * a, -ny)
        Nv = (nx, ny, nz)
        ox = ((wx * T[0] + wy * T[1]) + wz * T[2])[:, None]
        oy = ((wx * B[0] + wy * B[1]) + wz * B[2])[:, None]
        oz = ((wx * nx + wy * ny) + wz * nz)[:, None]
        # the visible normal of Heitz 2018 for this wo
        vx, vy = alpha * ox, alpha * oy
        vlen = np.sqrt((vx * vx + vy * vy) + oz * oz)
        vhx, vhy, vhz = vx / vlen, vy / vlen, oz / vlen
        l2 = vhx * vhx + vhy * vhy
        il = 1.0 / np.sqrt(np.where(l2 > 0.0, l2, 1.0))
        t1x, t1y = np.where(l2 > 0.0, -vhy * il, 1.0), np.where(l2 > 0.0, vhx * il, 0.0)
        t2x, t2y, t2z = -(vhz * t1y), vhz * t1x, vhx * t1y - vhy * t1x
        sh = 0.5 * (1.0 + vhz)
        lo1 = 1.0 + 0.5 * (np.sqrt(1.0 + a2 * ((ox * ox + oy * oy) / (oz * oz))) - 1.0)
        rr = np.sqrt(xi1)
        phi = (2.0 * np.pi) * xi2
        p1 = rr * np.cos(phi)
        q1 = 1.0 - p1 * p1
        p2 = (1.0 - sh) * np.sqrt(np.fmax(q1, 0.0)) + sh * (rr * np.sin(phi))
        pz = np.sqrt(np.fmax(q1 - p2 * p2, 0.0))
        nhx, nhy, nhz = (p1 * t1x + p2 * t2x) + pz * vhx, (p1 * t1y + p2 * t2y) + pz * vhy, p2 * t2z + pz * vhz
        gx, gy, gz = alpha * nhx, alpha * nhy, np.fmax(nhz, 0.0)
        hl = np.sqrt((gx * gx + gy * gy) + gz * gz)
        hx, hy, hz = gx / hl, gy / hl, gz / hl
        oh = (ox * hx + oy * hy) + oz * hz
        t2 = 2.0 * oh
        ix, iy, iz = t2 * hx - ox, t2 * hy - oy, t2 * hz - oz
        alive = (iz > 0.0) & (oz > 0.0) & ok[:, None]
        zz, xy = np.where(alive, iz, 1.0), np.where(alive, ix * ix + iy * iy, 0.0)
        li = 0.5 * (np.sqrt(1.0 + a2 * (xy / (zz * zz))) - 1.0)
        g = lo1 / (lo1 + li)
        m = np.fmax(1.0 - oh, 0.0)
        sw = ((m * m) * (m * m)) * m
        d = np.stack([(ix * T[k][:, None] + iy * B[k][:, None]) + iz * Nv[k][:, None] for k in range(3)], axis=-1)
        nrm = np.stack(Nv, axis=-1)
        o = p32.astype(np.float64) + float(F32(reflect._bias)) * nrm
        o = np.broadcast_to(o[:, None, :], d.shape)
    d = np.where(alive[..., None], d, 0.0).reshape(-1, 3)
    o = np.where(alive[..., None], o, 0.0).reshape(-1, 3)
    w = np.where(alive[..., None], np.stack([g, sw], axis=-1), 0.0).reshape(-1, 2).astype(np.float32)
    rays = _rays_out(o, d, device)
    if terms:
        return rays, w, {"wi_z": np.where(ok[:, None], iz, np.nan), "wo_z": np.where(ok[:, None], np.broadcast_to(oz, iz.shape), np.nan), "usable": ok}
    return rays, w


def reflect_reduce(surface, irradiance, weights, directions: int, direct=None) -> np.ndarray:
    """The numpy float64 statement of fw_reflect_reduce: (n, 8) float64, (1 / D) x the accumulators (P.rgb, alive, Q.rgb, sky) of one
    round before their one rounding to float32, for surface (n * D, 16) float32 records, irradiance (n * D, 3) float32, weights
    (n * D, 2) float32 (g, s) and direct (n * D, 8) float32 or None: per ray L as gather_reduce forms it, P += (g (1 - s)) L,
    Q += (g s) L, alive += [g > 0], sky += [kind == -1], summed in the device's order (G partial sums, an xor butterfly)."""
    D = int(directions)
    s = np.asarray(surface, np.float32).astype(np.float64).reshape(-1, D, 16)
    E = np.asarray(irradiance, np.float32).astype(np.float64).reshape(-1, D, 3)
    w = np.asarray(weights, np.float32).astype(np.float64).reshape(-1, D, 2)
    n = s.shape[0]
    kind = s[..., 3]
    T = np.where(E > 0.0, E, 0.0)
    if direct is not None:
        T = T + np.asarray(direct, np.float32).astype(np.float64).reshape(-1, D, 8)[..., 0:3]
    inv_pi = 1.0 / 3.141592653589793
    with np.errstate(all="ignore"):
        L = (s[..., 0:3] * T) * inv_pi
        emits = (kind == -1.0) | (kind == 3.0)
        L = np.where(emits[..., None], s[..., 12:15], L)
        g, sw = w[..., 0:1], w[..., 1:2]
        term = np.concatenate([(g * (1.0 - sw)) * L, (g * sw) * L, (kind == -1.0)[..., None].astype(np.float64)], axis=-1)      # (n, D, 7)
    live = kind != -2.0
    count = (w[..., 0] > 0.0).astype(np.float64)                                              # (counted whatever the ray's kind is)
    G = 1
    while G < min(D, 64):
        G *= 2
    rows = -(-D // G)                                                                        # lane l takes j = l, l + G, ... in ascending order
    padded = np.zeros((n, rows * G, 7))
    padded[:, :D] = term
    take = np.zeros((n, rows * G), bool)
    take[:, :D] = live
    ones = np.zeros((n, rows * G))
    ones[:, :D] = count
    part, alive = np.zeros((n, G, 7)), np.zeros((n, G))
    with np.errstate(all="ignore"):
        for row, on, c in zip(padded.reshape(n, rows, G, 7).transpose(1, 0, 2, 3), take.reshape(n, rows, G).transpose(1, 0, 2),
                              ones.reshape(n, rows, G).transpose(1, 0, 2)):
            part = np.where(on[..., None], part + row, part)                                 # (a ray that contributes nothing adds nothing: -0 and NaN stay out)
            alive = alive + c
        m = G // 2
        while m >= 1:
            part, alive = part + part[:, np.arange(G) ^ m], alive + alive[:, np.arange(G) ^ m]
            m //= 2
        inv = 1.0 / D
        return np.concatenate([inv * part[:, 0, 0:3], inv * alive[:, 0:1], inv * part[:, 0, 3:6], inv * part[:, 0, 6:7]], axis=-1)


def reflect_resolve(sums, spec, rounds: int) -> np.ndarray:
    """The statement of k_reflect_resolve: (..., 4) float32 (S.rgb, alive) from the float32 running sums (..., 8) = (P.rgb, alive, Q.rgb,
    sky) of `rounds` rounds and spec (..., 4) float32 (F0.rgb, rho): S_c = float32((f0_c P_c + Q_c) / rounds), alive / rounds."""
    s = np.asarray(sums, np.float32).astype(np.float64)
    f0 = np.asarray(spec, np.float32).astype(np.float64).reshape(s.shape[:-1] + (4,))[..., 0:3]
    with np.errstate(all="ignore"):
        S = (f0 * s[..., 0:3] + s[..., 4:7]) / float(rounds)
        return np.concatenate([S, s[..., 3:4] / float(rounds)], axis=-1).astype(np.float32)


# --------------------------------------------------------------------------- area lights at surface points (fw_bake_area)
class AreaLight:
    """The direct light of a scene's sampled area lights — every EmissiveMat sphere and axis-aligned rectangle — at surface points
    (fw_area): `samples` shadow rays per point, light and round towards points drawn on the light as the point sees it,
    origins moved `bias` along the normal.  .seed(s) / .jitter(on) as builders; chunk_points as fw_area's."""

    def __init__(self, samples: int = 16, bias: float = 1e-3):
        self.samples, self.bias = int(samples), float(np.float32(bias))
        self._seed, self._jitter, self.chunk_points = 0, True, 0

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def check(self):
        """what fw_area_rays rejects in a description, as a ValueError, in its order"""
        if not 1 <= self.samples <= 1 << 20:
            raise ValueError("samples must be in 1..2^20")
        if not (np.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError("bias must be finite and >= 0")
        return self

    def to_abi(self) -> A.fw_area:
        a = A.fw_area()
        a.samples, a.jitter, a.bias = self.samples & 0xFFFFFFFF, int(self._jitter), self.bias
        a.chunk_points, a.seed = int(self.chunk_points), self._seed & 0xFFFFFFFFFFFFFFFF
        return a


def _dotd(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def area_rays(area: "AreaLight", lights, positions, normals, ids=None, round: int = 0, device=None):
    """The numpy statement of fw_area_rays: (rays (n * Ln * S, 6) float32, weights (n * Ln * S,) float32), entry (q * Ln + i) * S + s =
    sample s of light i ((Ln, 16) float32 records: object, kind, 12 geometry floats, area, p_pick) from point id = ids[q] (ids None: q)
    of positions and normals, (M, 3) float32 each (device: see panorama_rays; the weights stay numpy).  Float64 from the float32 inputs
    in the header's order, one rounding to float32; a dead entry is six zeros and the weight 0."""
    S = int(area.samples)
    if S < 1:
        raise ValueError("samples must be >= 1")
    L = np.asarray(lights, np.float32).reshape(-1, A.FW_LIGHT_RECORD_FLOATS)
    Ln = L.shape[0]
    P, Nn = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    ids = np.arange(P.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    at = ids.astype(np.int64)
    n = at.size
    p32, n32 = P[at], Nn[at]
    usable = ao_usable(p32, n32)[:, None, None]                                              # (n, 1, 1), broadcast over (n, Ln, S)
    item = (at[:, None] * Ln + np.arange(Ln, dtype=np.int64)[None, :]).reshape(-1)
    xi = (texel_jitter(area._seed, round, item) if area._jitter else np.full((n * Ln, 2), 0.5)).reshape(n, Ln, 1, 2)
    s = np.arange(S, dtype=np.float64)[None, None, :]
    G = 0.6180339887498949
    PI = 3.141592653589793
    Lg = L.astype(np.float64)
    kind = L[:, 1][None, :, None]
    with np.errstate(all="ignore"):
        a1 = (s + xi[..., 0]) / float(S)
        u1 = a1 - np.floor(a1)
        a2 = s * G + xi[..., 1]
        u2 = a2 - np.floor(a2)
        r = n32.astype(np.float64)
        rl = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        nh = [(r[:, k] / rl)[:, None, None] for k in range(3)]
        p = [p32[:, k].astype(np.float64)[:, None, None] for k in range(3)]
        bias = float(F32(area.bias))
        o = p if area.bias == 0.0 else [p[k] + bias * nh[k] for k in range(3)]
        # rectangles
        c0 = [Lg[:, 2 + k][None, :, None] for k in range(3)]
        e1 = [Lg[:, 5 + k][None, :, None] - c0[k] for k in range(3)]
        e2 = [Lg[:, 11 + k][None, :, None] - c0[k] for k in range(3)]
        dr = [((c0[k] + u1 * e1[k]) + u2 * e2[k]) - o[k] for k in range(3)]
        nl = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        Ar = np.sqrt(_dotd(nl, nl))
        d2 = _dotd(dr, dr)
        dl = np.sqrt(d2)
        w = [dr[k] / dl for k in range(3)]
        cr_r = _dotd(nh, w)
        cl = np.abs(_dotd(nl, w) / Ar)
        g_r = ((cr_r * cl) * Ar) / d2
        live_r = (cr_r > 0.0) & (Ar > 0.0)
        # spheres
        v = [c0[k] - o[k] for k in range(3)]
        dv = _dotd(v, v)
        rr = Lg[:, 5][None, :, None]
        r2 = rr * rr
        s2 = r2 / dv
        cmax = np.sqrt(1.0 - s2)
        omc = s2 / (1.0 + cmax)
        om = u1 * omc
        ct = 1.0 - om
        st = np.sqrt(np.fmax(om * (2.0 - om), 0.0))
        phi = (2.0 * PI) * u2
        lx, ly = st * np.cos(phi), st * np.sin(phi)
        dist = np.sqrt(dv)
        wv = [v[k] / dist for k in range(3)]
        sg = np.copysign(1.0, wv[2])
        a = -1.0 / (sg + wv[2])
        b = (wv[0] * wv[1]) * a
        T = (1.0 + (sg * (wv[0] * wv[0])) * a, sg * b, -sg * wv[0])
        B = (b, sg + (wv[1] * wv[1]) * a, -wv[1])
        ex = [(lx * T[k] + ly * B[k]) + ct * wv[k] for k in range(3)]
        bb = _dotd(ex, v)
        tt = bb - np.sqrt(np.fmax(bb * bb - (dv - r2), 0.0))
        ds = [tt * ex[k] for k in range(3)]
        dls = np.sqrt(_dotd(ds, ds))
        cr_s = _dotd(nh, [ds[k] / dls for k in range(3)])
        g_s = (cr_s * (2.0 * PI)) * omc
        live_s = (dv > r2) & (cr_s > 0.0)
        sphere = np.broadcast_to(kind == 0, g_s.shape)
        g = np.where(sphere, g_s, g_r)
        d = np.stack([np.where(sphere, ds[k], dr[k]) for k in range(3)], axis=-1)
        o3 = np.stack([np.broadcast_to(o[k], g.shape) for k in range(3)], axis=-1)
        gf, df, of = g.astype(np.float32), d.astype(np.float32), o3.astype(np.float32)
        live = (usable & np.where(sphere, live_s, live_r) & np.isfinite(g) & (gf > 0) & np.isfinite(gf) & np.all(np.isfinite(df), axis=-1)
                & np.all(np.isfinite(of), axis=-1) & np.any(df != 0, axis=-1))
    weights = np.where(live, gf, np.float32(0)).astype(np.float32).reshape(-1)
    of = np.where(live[..., None], of, np.float32(0)).reshape(-1, 3)
    df = np.where(live[..., None], df, np.float32(0)).reshape(-1, 3)
    return _rays_out(of, df, device), weights


def area_reduce(weights, hits_object, surface, objects, samples: int) -> np.ndarray:
    """The numpy float64 statement of fw_area_reduce: (n, 4) float64, (1 / S) x the accumulators E.rgb and (1 / M) x V of one round
    before their one rounding to float32, for weights (n * M,) float32, the hits' object column (uint32), surface (n * M, 16) float32
    records and the Ln lights' object indices, M = Ln * S, summed in the device's order (G partial sums, an xor butterfly)."""
    S = int(samples)
    obj = np.asarray(objects).astype(np.uint32).reshape(-1)
    M = obj.size * S
    w = np.asarray(weights, np.float32).reshape(-1, M)
    n = w.shape[0]
    h = np.asarray(hits_object).astype(np.uint32).reshape(n, M)
    s = np.asarray(surface, np.float32).reshape(n, M, 16)
    counts = (w > 0) & (h == np.repeat(obj, S)[None, :]) & (s[..., 3] == np.float32(3))
    with np.errstate(all="ignore"):
        term = np.concatenate([s[..., 12:15].astype(np.float64) * w.astype(np.float64)[..., None], np.ones((n, M, 1))], axis=-1)
    G = 1
    while G < min(M, 64):
        G *= 2
    rows = -(-M // G)                                                                        # lane l takes m = l, l + G, ... in ascending order
    padded = np.zeros((n, rows * G, 4))
    padded[:, :M] = term
    take = np.zeros((n, rows * G), bool)
    take[:, :M] = counts
    part = np.zeros((n, G, 4))
    with np.errstate(all="ignore"):
        for row, on in zip(padded.reshape(n, rows, G, 4).transpose(1, 0, 2, 3), take.reshape(n, rows, G).transpose(1, 0, 2)):
            part = np.where(on[..., None], part + row, part)                                 # (an entry that does not count adds nothing)
        m = G // 2
        while m >= 1:
            part = part + part[:, np.arange(G) ^ m]
            m //= 2
        return np.concatenate([(1.0 / S) * part[:, 0, 0:3], (1.0 / M) * part[:, 0, 3:4]], axis=-1)


def area_resolve(sums, rounds: int) -> np.ndarray:
    """The statement of k_area_resolve: (..., 4) float32 (E.rgb, vis) = float32(sums / rounds) from the float32 running sums."""
    with np.errstate(all="ignore"):
        return (np.asarray(sums, np.float32).astype(np.float64) / float(rounds)).astype(np.float32)


def area_mask(hits_object, surface, objects) -> np.ndarray:
    """The statement of fw_area_mask: a copy of surface ((n, 16) float32) in which every record of kind 3 whose hit's object is one of
    `objects` is (kind -2, every other float 0); every other record keeps its bits."""
    s = np.array(np.asarray(surface, np.float32).reshape(-1, 16))
    hit = (s[:, 3] == np.float32(3)) & np.isin(np.asarray(hits_object).astype(np.uint32).reshape(-1), np.asarray(objects).astype(np.uint32))
    s[hit] = 0
    s[hit, 3] = -2
    return s


# --------------------------------------------------------------------------- every emitter at surface points (fw_bake_emitters)
class EmitterLights:
    """The direct light of every emitting primitive of a scene — EmissiveMat spheres, rectangles, Rect3d faces, disks and mesh triangles —
    at surface points (fw_emitters): `samples` shadow rays per point and round whatever the number of emitters, each
    towards an entry picked in proportion to area x power, origins moved `bias` along the normal.  .seed(s) / .jitter(on) as builders;
    chunk_points as fw_emitters'."""

    def __init__(self, samples: int = 16, bias: float = 1e-3):
        self.samples, self.bias = int(samples), float(np.float32(bias))
        self._seed, self._jitter, self.chunk_points = 0, True, 0

    def seed(self, s):
        self._seed = int(s)
        return self

    def jitter(self, on=True):
        self._jitter = bool(on)
        return self

    def check(self):
        """what fw_emitters_rays rejects in a description, as a ValueError, in its order"""
        if not 1 <= self.samples <= 1 << 20:
            raise ValueError("samples must be in 1..2^20")
        if not (np.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError("bias must be finite and >= 0")
        return self

    def to_abi(self) -> A.fw_emitters:
        a = A.fw_emitters()
        a.samples, a.jitter, a.bias = self.samples & 0xFFFFFFFF, int(self._jitter), self.bias
        a.chunk_points, a.seed = int(self.chunk_points), self._seed & 0xFFFFFFFFFFFFFFFF
        return a


def emitters_cdf(weights):
    """The numpy statement of fw_emitters_cdf: (cdf (N,) float64, total): float64 inclusive prefix sums of the float32 weights in entry
    order, a negative or non-finite weight counted as 0, each divided by the last; total 0: "no emitters", the cdf is zeros."""
    w = np.asarray(weights, np.float32).reshape(-1).astype(np.float64)
    w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    c = np.zeros(w.size)
    total = 0.0
    for i in range(w.size):                                                                  # (sequential: np.cumsum's order is its own)
        total = total + float(w[i])
        c[i] = total
    if not (total > 0.0 and np.isfinite(total)):
        return np.zeros(w.size), 0.0
    return c / total, total


def emitters_rays(emitters: "EmitterLights", records, cdf, positions, normals, ids=None, round: int = 0, device=None):
    """The numpy statement of fw_emitters_rays: (rays (n * S, 6) float32, weights (n * S,) float32, picks (n * S,) uint32), entry q * S +
    s = sample s from point id = ids[q] (ids None: q) of positions and normals, (M, 3) float32 each, towards the entry of `records` ((N,
    16) float32) picked through `cdf` ((N,) float64 as emitters_cdf gives it; device: see panorama_rays; weights and picks stay numpy).
    Float64 from the float32 inputs in the header's order, one rounding to float32; a dead entry is six zeros, weight 0, pick 0xffffffff."""
    of, df, weights, picks, _margin = _emitters_entries(emitters, records, cdf, positions, normals, ids, round)
    return _rays_out(of, df, device), weights, picks


def _emitters_entries(emitters, records, cdf, positions, normals, ids, round):
    """emitters_rays' arithmetic: (origins (n * S, 3), directions (n * S, 3), weights, picks, margin), margin (n * S,) float64 = how far
    the entry's liveness tests (n . w > 0, a sphere's |v|^2 > r^2) are from their boundary in float64 (NaN at an unusable point)"""
    S = int(emitters.samples)
    if S < 1:
        raise ValueError("samples must be >= 1")
    L = np.asarray(records, np.float32).reshape(-1, A.FW_EMITTERS_RECORD_FLOATS)
    cd = np.asarray(cdf, np.float64).reshape(-1)
    N = L.shape[0]
    if N < 1 or cd.size != N or not cd[-1] == 1.0:
        raise ValueError("records and a cdf that ends in 1 are needed")
    P, Nn = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    ids = np.arange(P.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    at = ids.astype(np.int64)
    n = at.size
    p32, n32 = P[at], Nn[at]
    usable = ao_usable(p32, n32)[:, None]                                                    # (n, 1), broadcast over (n, S)
    xj = (texel_jitter(emitters._seed, round, at) if emitters._jitter else np.full((n, 2), 0.5)).reshape(n, 1, 2)
    s = np.arange(S, dtype=np.float64)[None, :]
    G = 0.6180339887498949
    PI = 3.141592653589793
    with np.errstate(all="ignore"):
        a1 = (s + xj[..., 0]) / float(S)
        xi = a1 - np.floor(a1)
        a2 = s * G + xj[..., 1]
        u2 = a2 - np.floor(a2)
        pick = np.minimum(np.searchsorted(cd, xi, side="right"), N - 1)                      # the first index with cdf[index] > xi
        lo = np.where(pick > 0, cd[np.maximum(pick - 1, 0)], 0.0)
        pp = cd[pick] - lo
        u1 = np.minimum((xi - lo) / pp, 1.0 - 2.0 ** -53)
        Lg = L.astype(np.float64)[pick]                                                      # (n, S, 16)
        kind = L[:, 1][pick]
        g12 = [Lg[..., 2 + k] for k in range(12)]
        r = n32.astype(np.float64)
        rl = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        nh = [(r[:, k] / rl)[:, None] for k in range(3)]
        p = [p32[:, k].astype(np.float64)[:, None] for k in range(3)]
        bias = float(F32(emitters.bias))
        o = p if emitters.bias == 0.0 else [p[k] + bias * nh[k] for k in range(3)]
        c0, q1, q2, c3 = g12[0:3], g12[3:6], g12[6:9], g12[9:12]
        cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        # rectangles and Rect3d faces: corners c0, c1 = q1, c3
        e1 = [q1[k] - c0[k] for k in range(3)]
        e2r = [c3[k] - c0[k] for k in range(3)]
        d_r = [((c0[k] + u1 * e1[k]) + u2 * e2r[k]) - o[k] for k in range(3)]
        nl_r = cross(e1, e2r)
        L_r = np.sqrt(_dotd(nl_r, nl_r))
        A_r = L_r
        # triangles: v0 = c0, v1 = q1, v2 = q2
        e2t = [q2[k] - c0[k] for k in range(3)]
        sq = np.sqrt(u1)
        b0, b1, b2 = 1.0 - sq, sq * (1.0 - u2), sq * u2
        d_t = [((b0 * c0[k] + b1 * q1[k]) + b2 * q2[k]) - o[k] for k in range(3)]
        nl_t = cross(e1, e2t)
        L_t = np.sqrt(_dotd(nl_t, nl_t))
        A_t = L_t / 2.0
        # disks: centre c0, axes q1 and q2, then r, r_in, phi_max
        ro2, ri2 = c3[0] * c3[0], c3[1] * c3[1]
        rr_d = np.sqrt(ri2 + u1 * (ro2 - ri2))
        phi_d = u2 * c3[2]
        ca, sa = rr_d * np.cos(phi_d), rr_d * np.sin(phi_d)
        d_d = [((c0[k] + ca * q1[k]) + sa * q2[k]) - o[k] for k in range(3)]
        nl_d = cross(q1, q2)
        L_d = np.sqrt(_dotd(nl_d, nl_d))
        A_d = (0.5 * c3[2]) * (ro2 - ri2)
        is_t, is_d = kind == 5, kind == 9
        sel = lambda t, dk, rc: np.where(is_t, t, np.where(is_d, dk, rc))
        df_ = [sel(d_t[k], d_d[k], d_r[k]) for k in range(3)]
        nl = [sel(nl_t[k], nl_d[k], nl_r[k]) for k in range(3)]
        Ln_, Ar = sel(L_t, L_d, L_r), sel(A_t, A_d, A_r)
        d2 = _dotd(df_, df_)
        dl = np.sqrt(d2)
        w = [df_[k] / dl for k in range(3)]
        cr_f = _dotd(nh, w)
        cl = np.abs(_dotd(nl, w) / Ln_)
        g_f = ((cr_f * cl) * Ar) / d2
        live_f = (cr_f > 0.0) & (Ar > 0.0) & (Ln_ > 0.0)
        # spheres: area_rays' cone
        v = [c0[k] - o[k] for k in range(3)]
        dv = _dotd(v, v)
        rr = g12[3]
        r2 = rr * rr
        s2 = r2 / dv
        cmax = np.sqrt(1.0 - s2)
        omc = s2 / (1.0 + cmax)
        om = u1 * omc
        ct = 1.0 - om
        st = np.sqrt(np.fmax(om * (2.0 - om), 0.0))
        phi = (2.0 * PI) * u2
        lx, ly = st * np.cos(phi), st * np.sin(phi)
        dist = np.sqrt(dv)
        wv = [v[k] / dist for k in range(3)]
        sg = np.copysign(1.0, wv[2])
        a = -1.0 / (sg + wv[2])
        b = (wv[0] * wv[1]) * a
        T = (1.0 + (sg * (wv[0] * wv[0])) * a, sg * b, -sg * wv[0])
        B = (b, sg + (wv[1] * wv[1]) * a, -wv[1])
        ex = [(lx * T[k] + ly * B[k]) + ct * wv[k] for k in range(3)]
        bb = _dotd(ex, v)
        tt = bb - np.sqrt(np.fmax(bb * bb - (dv - r2), 0.0))
        ds = [tt * ex[k] for k in range(3)]
        dls = np.sqrt(_dotd(ds, ds))
        cr_s = _dotd(nh, [ds[k] / dls for k in range(3)])
        g_s = (cr_s * (2.0 * PI)) * omc
        live_s = (dv > r2) & (cr_s > 0.0)
        sphere = kind == 0
        g = np.where(sphere, g_s, g_f) / pp
        d = np.stack([np.where(sphere, ds[k], df_[k]) for k in range(3)], axis=-1)
        o3 = np.stack([np.broadcast_to(o[k], g.shape) for k in range(3)], axis=-1)
        gf, df, of = g.astype(np.float32), d.astype(np.float32), o3.astype(np.float32)
        live = (usable & np.where(sphere, live_s, live_f) & np.isfinite(g) & (gf > 0) & np.isfinite(gf) & np.all(np.isfinite(df), axis=-1)
                & np.all(np.isfinite(of), axis=-1) & np.any(df != 0, axis=-1))
    weights = np.where(live, gf, np.float32(0)).astype(np.float32).reshape(-1)
    picks = np.where(live, pick, 0xFFFFFFFF).astype(np.uint32).reshape(-1)
    of = np.where(live[..., None], of, np.float32(0)).reshape(-1, 3)
    df = np.where(live[..., None], df, np.float32(0)).reshape(-1, 3)
    with np.errstate(all="ignore"):
        margin = np.where(sphere, np.minimum(np.abs(cr_s), np.abs(dv - r2)), np.abs(cr_f)).reshape(-1)
    return of, df, weights, picks, margin


def emitters_reduce(picks, weights, hits_object, hits_prim, surface, codes, samples: int) -> np.ndarray:
    """The numpy float64 statement of fw_emitters_reduce: (n, 4) float64, (1 / S) x the accumulators E.rgb and V of one round before their
    one rounding to float32, for picks (n * S,) uint32, weights (n * S,) float32, the hits' object and prim columns (uint32), surface (n *
    S, 16) float32 records and codes (N, 2) uint32, summed in the device's order (G partial sums, an xor butterfly)."""
    S = int(samples)
    cod = np.asarray(codes).astype(np.uint32).reshape(-1, 2)
    w = np.asarray(weights, np.float32).reshape(-1, S)
    n = w.shape[0]
    pk = np.asarray(picks).astype(np.uint32).reshape(n, S)
    ho, hp = np.asarray(hits_object).astype(np.uint32).reshape(n, S), np.asarray(hits_prim).astype(np.uint32).reshape(n, S)
    s = np.asarray(surface, np.float32).reshape(n, S, 16)
    valid = pk < cod.shape[0]
    at = np.where(valid, pk, 0).astype(np.int64)
    counts = (w > 0) & valid & (ho == cod[at, 0]) & (hp == cod[at, 1]) & (s[..., 3] == np.float32(3))
    with np.errstate(all="ignore"):
        term = np.concatenate([s[..., 12:15].astype(np.float64) * w.astype(np.float64)[..., None], np.ones((n, S, 1))], axis=-1)
    G = 1
    while G < min(S, 64):
        G *= 2
    rows = -(-S // G)                                                                        # lane l takes m = l, l + G, ... in ascending order
    padded = np.zeros((n, rows * G, 4))
    padded[:, :S] = term
    take = np.zeros((n, rows * G), bool)
    take[:, :S] = counts
    part = np.zeros((n, G, 4))
    with np.errstate(all="ignore"):
        for row, on in zip(padded.reshape(n, rows, G, 4).transpose(1, 0, 2, 3), take.reshape(n, rows, G).transpose(1, 0, 2)):
            part = np.where(on[..., None], part + row, part)                                 # (an entry that does not count adds nothing)
        m = G // 2
        while m >= 1:
            part = part + part[:, np.arange(G) ^ m]
            m //= 2
        return (1.0 / S) * part[:, 0, :]


emitters_resolve = area_resolve


# --------------------------------------------------------------------------- direct light of delta lights (fw_bake_direct)
class DirectLight:
    """The direct light of a scene's point, spot and directional lights at surface points (fw_direct): one shadow ray per
    point and light, origins moved `bias` along the normal.  lobe "cosine": E is the irradiance; "renderer": E is pi x what the path
    tracer's light sample adds per unit albedo at a Lambertian vertex (2 c^3).  face_view: with view directions, the side of a surface
    the eye sees is the side that is lit.  chunk_points as fw_direct's."""
    LOBES = {"cosine": 0, "renderer": 1}

    def __init__(self, bias: float = 1e-3, lobe: str = "cosine", face_view: bool = True):
        self.bias, self.lobe, self.face_view, self.chunk_points = float(np.float32(bias)), lobe, face_view, 0

    def check(self):
        """what fw_direct_rays rejects in a description, as a ValueError, in its order"""
        if self.lobe not in self.LOBES:
            raise ValueError('lobe must be "cosine" or "renderer"')
        if self.face_view not in (False, True, 0, 1):
            raise ValueError("face_view must be False or True")
        if not (np.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError("bias must be finite and >= 0")
        return self

    def to_abi(self) -> A.fw_direct:
        self.check()
        d = A.fw_direct()
        d.lobe, d.face_view, d.bias, d.chunk_points = self.LOBES[self.lobe], int(bool(self.face_view)), self.bias, int(self.chunk_points)
        return d


def light_records(lights):
    """(kind (Ln,) uint32, rec (Ln, 12) float64) of api lights or fw_light records as a resident scene keeps them: (position, -),
    (direction, cos_inner), (intensity, cos_outer), every field a float32 value, the direction divided by its float64 length and
    rounded to float32"""
    kind, rec = np.zeros(len(lights), np.uint32), np.zeros((len(lights), 12), np.float64)
    for i, light in enumerate(lights):
        l = light if isinstance(light, A.fw_light) else light.to_abi()
        kind[i] = l.kind
        d = np.array([l.direction.x, l.direction.y, l.direction.z], np.float64)
        n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        if n > 0:
            d = (d / n).astype(np.float32).astype(np.float64)
        rec[i] = (l.position.x, l.position.y, l.position.z, 0.0, d[0], d[1], d[2], l.cos_inner, l.intensity.x, l.intensity.y, l.intensity.z,
                  l.cos_outer)
    return kind, rec


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _direct_points(direct: "DirectLight", positions, normals, ids, view, spec):
    """(ids, p32 (n, 3) float32, usable (n,), nh (n, 3) float64, view (n, 3) float64 or None, spec (n, 4) float32 or None) of a call"""
    P, Nn = np.asarray(positions, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    ids = np.arange(P.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    at = ids.astype(np.int64)
    p32, n32 = P[at], Nn[at]
    ok = ao_usable(p32, n32)
    n64 = n32.astype(np.float64)
    with np.errstate(all="ignore"):
        nh = n64 / np.sqrt((n64[:, 0:1] * n64[:, 0:1] + n64[:, 1:2] * n64[:, 1:2]) + n64[:, 2:3] * n64[:, 2:3])
        vw = None
        if view is not None:
            vw = np.asarray(view, np.float32).reshape(-1, 3)[at].astype(np.float64)
            if direct.face_view:
                nh = np.where((_dot3(nh, vw) > 0.0)[:, None], -nh, nh)
    sp = None if spec is None else np.asarray(spec, np.float32).reshape(-1, 4)[at]
    if sp is not None and vw is None:
        raise ValueError("spec needs view")
    return ids, p32, ok, nh, vw, sp


def _spot_factor(c, ci, co):
    with np.errstate(all="ignore"):
        t = np.fmin(np.fmax((c - co) / (ci - co), 0.0), 1.0)
        return np.where(ci > co, (t * t) * (3.0 - 2.0 * t), np.where(c >= co, 1.0, 0.0))


def _direct_geometry(kind, rec, d):
    """(d2, w, s) of directions d (n, Ln, 3) float64 towards the lights: the squared length, the unit direction, the spot factor (1 for
    the other kinds)"""
    with np.errstate(all="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        w = d / np.sqrt(d2)[..., None]
        s = np.where(kind[None, :] == 1, _spot_factor(-_dot3(w, rec[None, :, 4:7]), rec[None, :, 7], rec[None, :, 11]), 1.0)
    return d2, w, s


def direct_rays(direct: "DirectLight", lights, positions, normals, ids=None, view=None, spec=None, device=None, terms: bool = False):
    """The numpy statement of fw_direct_rays: (n * Ln, 6) float32, entry q * Ln + i = the shadow ray of point id = ids[q] (ids None: q)
    towards light i, or six zeros (include/firework_hip.h has the rules).  positions, normals, view (M, 3) and spec (M, 4) float32,
    indexed by id (device: see panorama_rays).  terms=True: returns (rays, t) with t a dict of (n, Ln) float64 arrays — c = nh . w, cs =
    a spot's -(w . axis) (nan for the other kinds), d2 — the quantities the culling decisions compare with their thresholds."""
    direct.check()
    kind, rec = light_records(lights)
    Ln = kind.size
    ids, p32, ok, nh, vw, sp = _direct_points(direct, positions, normals, ids, view, spec)
    n = ids.size
    with np.errstate(all="ignore"):
        p64 = p32.astype(np.float64)
        o = p64 if direct.bias == 0.0 else p64 + float(F32(direct.bias)) * nh
        d = np.where((kind == 2)[None, :, None], -rec[None, :, 4:7], rec[None, :, 0:3] - o[:, None, :])
        d2, w, s = _direct_geometry(kind, rec, d)
        c = _dot3(nh[:, None, :], w)
        o32 = np.repeat(o.astype(np.float32)[:, None, :], Ln, axis=1)
        d32 = d.astype(np.float32)
        lit = ok[:, None] & np.any(rec[:, 8:11] != 0.0, axis=1)[None, :] & (d2 > 0.0) & np.isfinite(d2) & (c > 0.0) & (s != 0.0)
        if sp is not None:
            lit &= ~(sp[:, 3] < 0)[:, None]
        lit &= np.all(np.isfinite(o32), axis=-1) & np.all(np.isfinite(d32), axis=-1) & np.any(d32 != 0, axis=-1)
    rays = _rays_out(np.where(lit[..., None], o32, np.float32(0)).reshape(-1, 3), np.where(lit[..., None], d32, np.float32(0)).reshape(-1, 3), device)
    if not terms:
        return rays
    cs = np.where(kind[None, :] == 1, -_dot3(w, rec[None, :, 4:7]), np.nan)
    return rays, dict(c=c, cs=np.broadcast_to(cs, (n, Ln)), d2=d2)


def direct_reduce(direct: "DirectLight", lights, positions, normals, rays, hits_t, hits_object, ids=None, view=None, spec=None, terms: bool = False):
    """The numpy float64 statement of fw_direct_reduce: (n, 7) float64, the accumulators (E.rgb, N, S.rgb) of one round before their one
    rounding to float32, for rays (n * Ln, 6) float32 (as stored) and the hits' t (float32) and object (uint32, 0xFFFFFFFF = miss)
    columns, summed in the device's order (G partial sums, an xor butterfly).  terms=True: returns (acc, T, vis) with T (n, 7) = sum_i
    |term_i| (what a rounding-error bound of the sums scales with) and vis (n, Ln) bool, the entries that count as visible (N's terms)."""
    direct.check()
    kind, rec = light_records(lights)
    Ln = kind.size
    ids, p32, ok, nh, vw, sp = _direct_points(direct, positions, normals, ids, view, spec)
    n = ids.size
    d = np.asarray(rays, np.float32).astype(np.float64).reshape(n, Ln, 6)[..., 3:]
    t32 = np.asarray(hits_t, np.float32).reshape(n, Ln)
    miss = np.asarray(hits_object).astype(np.uint32).reshape(n, Ln) == np.uint32(0xFFFFFFFF)
    rho = np.zeros(n, np.float32) if sp is None else sp[:, 3]
    f0 = np.zeros((n, 3)) if sp is None else sp[:, 0:3].astype(np.float64)
    glossy = rho > 0
    with np.errstate(all="ignore"):
        if vw is None:
            wo, co, lo, takes = np.zeros((n, 3)), np.zeros(n), np.zeros(n), ok & ~(rho < 0) & ~glossy
        else:
            wo = -(vw / np.sqrt(_dot3(vw, vw))[:, None])
            co = _dot3(nh, wo)
            takes = ok & ~(rho < 0) & (~glossy | (co > 0.0))
        al = (rho * rho).astype(np.float64)                                                # the float32 product, widened
        al2 = al * al
        if vw is not None:
            tw = wo - co[:, None] * nh
            lo = 0.5 * (np.sqrt(1.0 + al2 * (_dot3(tw, tw) / (co * co))) - 1.0)
        d2, w, s = _direct_geometry(kind, rec, d)
        c = _dot3(nh[:, None, :], w)
        live = takes[:, None] & np.any(d != 0.0, axis=-1) & np.isfinite(d2) & (c > 0.0)
        vis = live & (miss | ((kind != 2)[None, :] & (t32 >= np.float32(1.0))))
        L = np.where((kind == 2)[None, :, None], rec[None, :, 8:11], (rec[None, :, 8:11] * s[..., None]) / d2[..., None])
        g = 2.0 * ((c * c) * c) if direct.lobe == "renderer" else c
        e = L * g[..., None]
        # GgxMat's f cos around nh without a tangent frame
        h0 = wo[:, None, :] + w
        h = h0 / np.sqrt(_dot3(h0, h0))[..., None]
        hn, oh = _dot3(nh[:, None, :], h), _dot3(wo[:, None, :], h)
        th = h - hn[..., None] * nh[:, None, :]
        sd = _dot3(th, th) + al2[:, None] * (hn * hn)
        D = al2[:, None] / (np.pi * (sd * sd))
        tu = w - c[..., None] * nh[:, None, :]
        li = 0.5 * (np.sqrt(1.0 + al2[:, None] * (_dot3(tu, tu) / (c * c))) - 1.0)
        gg = (D / (4.0 * co[:, None])) / ((1.0 + lo[:, None]) + li)
        m = 1.0 - oh
        m5 = ((m * m) * (m * m)) * m
        sg = L * ((f0[:, None, :] + (1.0 - f0[:, None, :]) * m5[..., None]) * gg[..., None])
        term = np.zeros((n, Ln, 7))
        term[..., 0:3] = np.where((vis & ~glossy[:, None])[..., None], e, 0.0)
        term[..., 3] = np.where(vis, 1.0, 0.0)
        term[..., 4:7] = np.where((vis & glossy[:, None])[..., None], sg, 0.0)
    G = 1
    while G < min(Ln, 64):
        G *= 2
    rows = -(-Ln // G)                                                                       # lane l takes i = l, l + G, ... in ascending order
    padded = np.zeros((n, rows * G, 7))
    padded[:, :Ln] = term
    part = np.zeros((n, G, 7))
    for row in padded.reshape(n, rows, G, 7).transpose(1, 0, 2, 3):
        part = part + row
    mm = G // 2
    while mm >= 1:
        part = part + part[:, np.arange(G) ^ mm]
        mm //= 2
    acc = part[:, 0]
    if not terms:
        return acc
    return acc, np.abs(term).sum(axis=1), vis


def direct_resolve(sums, rounds: int) -> np.ndarray:
    """The statement of k_direct_resolve: (..., 8) float32, the float32 running sums (..., 8) of `rounds` rounds divided by their number
    in float64 and rounded once; the eighth float 0"""
    s = np.asarray(sums, np.float32).astype(np.float64)
    out = (s / float(rounds)).astype(np.float32)
    out[..., 7] = 0.0
    return out


def material_direct_table(desc: "SceneDesc") -> np.ndarray:
    """(n_materials + 1, 4) float32: fw_bake_direct's (F0.rgb, rho) of every material of a scene description — a GgxMat (albedo,
    roughness): a glossy point; a Lambertian or Isotropic material zeros: a diffuse point; a Metal, Dielectric or Emissive material and
    the last row, a miss, rho = -1: they take no light sample"""
    n = int(desc.desc.n_materials)
    table = np.zeros((n + 1, 4), np.float32)
    table[:, 3] = -1.0
    for i in range(n):
        m = desc.materials[i]
        if m.kind == A.FW_MAT_GGX:
            table[i] = (m.albedo.x, m.albedo.y, m.albedo.z, np.float32(m.roughness))
        elif m.kind in (A.FW_MAT_LAMBERTIAN, A.FW_MAT_ISOTROPIC):
            table[i] = 0.0
    return table


# render_sequence's default cap on the samples a pixel carries over from the frames before it
DEFAULT_MAX_HISTORY = 64.0


def orbit_cameras(camera: CameraSettings, n: int) -> list:
    """n cameras evenly spaced in azimuth around `camera`'s look_at: view k rotates cam_pos - look_at about +Y by 2 pi k / n (computed
    in float64, rounded to float32); look_at, field of view, aperture and focus distance stay.  View 0 is `camera` itself, unchanged."""
    import copy
    n = int(n)
    if n < 1:
        raise ValueError("orbit_cameras needs n >= 1")
    out = [copy.deepcopy(camera)]
    pos = np.asarray(camera._cam_pos, np.float64)
    at = np.asarray(camera._look_at, np.float64)
    d = pos - at
    for k in range(1, n):
        a = 2.0 * np.pi * k / n
        c, s = np.cos(a), np.sin(a)
        rotated = np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])
        cam = copy.deepcopy(camera)
        cam._cam_pos = (at + rotated).astype(np.float32)
        cam._cam_pos[1] = camera._cam_pos[1]                 # the height, exactly
        out.append(cam)
    return out


def _placement_matrices(desc) -> tuple:
    """(R (n, 3, 3), t (n, 3)) float64 of a SceneDesc's objects as RenderObjectInternal places them (scene.rs:235-266): world = R local + t,
    R = Rotor3::into_matrix(rotation) — the identity where 0.5 (trace R - 1) >= 0.999, where the reference skips the rotation."""
    n = int(desc.desc.n_objects)
    R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        o = desc.objects[i]
        r = o.rotation
        s, xy, xz, yz = (np.float32(v) for v in (r.s, r.xy, r.xz, r.yz))
        s2, bxy2, bxz2, byz2 = s * s, xy * xy, xz * xz, yz * yz
        c0 = (s2 - bxy2 - bxz2 + byz2, np.float32(-2) * (xz * yz + s * xy), np.float32(2) * (xy * yz - s * xz))
        c1 = (np.float32(2) * (s * xy - xz * yz), s2 - bxy2 + bxz2 - byz2, np.float32(-2) * (s * yz + xy * xz))
        c2 = (np.float32(2) * (s * xz + xy * yz), np.float32(2) * (s * yz - xy * xz), s2 + bxy2 - bxz2 - byz2)
        m = np.array([c0, c1, c2], np.float32).T.astype(np.float64)          # columns c0, c1, c2
        R[i] = m if np.float32(0.5) * (np.float32(m[0, 0] + m[1, 1]) + np.float32(m[2, 2]) - np.float32(1)) < np.float32(0.999) else np.eye(3)
        t[i] = (o.position.x, o.position.y, o.position.z)
    return R, t


def previous_positions(positions, objects, scene_before, scene_after):
    """Where the surface points of a frame were one frame earlier, for the rigid placements DeviceScene.update (fw_scene_update) changes:
    fw_temporal's prev_position.  positions: (N, 3) world positions in the frame rendered from `scene_after` (fw_render_aovs' position
    columns); objects: (N,) the object each pixel shows, gbuffer()['object'] (FW_NO_HIT, or -1 in an int32 view, where the ray missed).
    Each point goes back through its object's placement in scene_after and forward through the one in scene_before
    (RenderObjectInternal, scene.rs:235-266: world = R local + position):  prev = R_b R_a^T (x - p_a) + p_b.  Missed pixels, and pixels of
    objects that did not move, keep their position bit for bit.  Scenes: Scene or SceneDesc of the same objects — a Scene is read as it
    is now, so pass the description made before it was moved.  numpy arrays give a float32 array, torch tensors a tensor on their device."""
    da = scene_after if isinstance(scene_after, SceneDesc) else scene_after.to_desc()
    db = scene_before if isinstance(scene_before, SceneDesc) else scene_before.to_desc()
    n_obj = int(da.desc.n_objects)
    if int(db.desc.n_objects) != n_obj:
        raise ValueError(f"the scenes have {db.desc.n_objects} and {n_obj} objects")
    Ra, ta = _placement_matrices(da)
    Rb, tb = _placement_matrices(db)
    M = np.einsum("nij,nkj->nik", Rb, Ra)                       # R_b R_a^T
    moved = np.array([not (np.array_equal(Ra[i], Rb[i]) and np.array_equal(ta[i], tb[i])) for i in range(n_obj)], bool)
    if type(positions).__module__.startswith("torch"):
        import torch
        dev = positions.device
        obj = objects.to(torch.int64)
        ok = (obj >= 0) & (obj < n_obj)
        idx = torch.where(ok, obj, torch.zeros_like(obj))
        ok = ok & torch.as_tensor(moved, device=dev)[idx] if n_obj else ok
        x = positions.to(torch.float64)
        Mt, tat, tbt = (torch.as_tensor(a, device=dev) for a in (M, ta, tb))
        prev = torch.einsum("nij,nj->ni", Mt[idx], x - tat[idx]) + tbt[idx]
        return torch.where(ok[:, None], prev.to(torch.float32), positions)
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    obj = np.asarray(objects).reshape(-1).astype(np.int64)
    obj = np.where(obj == A.FW_NO_HIT, -1, obj)
    ok = (obj >= 0) & (obj < n_obj)
    idx = np.where(ok, obj, 0)
    if n_obj:
        ok = ok & moved[idx]
    prev = np.einsum("nij,nj->ni", M[idx], pos.astype(np.float64) - ta[idx]) + tb[idx]
    return np.where(ok[:, None], prev.astype(np.float32), pos)


class Renderer:
    """src/render.rs:59-218.  Builder methods carry the reference's names; read the current
    values from `.settings`."""

    def __init__(self):
        # Default (render.rs:199-218)
        self.settings = dict(width=1920, height=1080, samples=128, multithreaded=True, use_bvh=False, gamma=2.2,
                             seed=0, paths_per_batch=0, flags=0)
        self._camera = CameraSettings()

    @staticmethod
    def default():
        return Renderer()

    def width(self, w):
        self.settings["width"] = int(w)
        return self

    def height(self, h):
        self.settings["height"] = int(h)
        return self

    def samples(self, s):
        self.settings["samples"] = int(s)
        return self

    def multithreaded(self, m):
        self.settings["multithreaded"] = bool(m)
        return self

    def use_bvh(self, b):
        self.settings["use_bvh"] = bool(b)
        return self

    def gamma(self, g):
        self.settings["gamma"] = float(g)
        return self

    def camera(self, settings: CameraSettings):
        self._camera = settings
        return self

    # extensions of the GPU path (not in the reference)
    def seed(self, s):
        self.settings["seed"] = int(s)
        return self

    def paths_per_batch(self, n):
        self.settings["paths_per_batch"] = int(n)
        return self

    def time_kernels(self, on=True):
        self.settings["flags"] = (self.settings["flags"] | A.FW_FLAG_TIME_KERNELS) if on else (
            self.settings["flags"] & ~A.FW_FLAG_TIME_KERNELS)
        return self

    def light_sampling(self, on=True):
        """FW_FLAG_LIGHT_SAMPLING: next-event estimation with MIS at Lambertian and Isotropic vertices — the same image in
        expectation with less noise per sample.  A scene without a sampled light (an EmissiveMat sphere or axis-aligned rectangle) renders
        the default frame; fw_render_aovs ignores the flag."""
        self.settings["flags"] = (self.settings["flags"] | A.FW_FLAG_LIGHT_SAMPLING) if on else (
            self.settings["flags"] & ~A.FW_FLAG_LIGHT_SAMPLING)
        return self

    def env_sampling(self, on=True):
        """FW_FLAG_ENV_SAMPLING: importance sampling of an HDR environment map at Lambertian and Isotropic vertices, alone or
        beside light_sampling's emitters — the same image in expectation with less noise under a bright sun.  Without an HDR map of positive
        weight (or without a Lambertian or Isotropic material) the frame is the one without the flag; fw_render_aovs ignores it."""
        self.settings["flags"] = (self.settings["flags"] | A.FW_FLAG_ENV_SAMPLING) if on else (
            self.settings["flags"] & ~A.FW_FLAG_ENV_SAMPLING)
        return self

    def all_emitters(self, on=True):
        """FW_FLAG_ALL_EMITTERS: with light_sampling, every emitting primitive is a sampled light — EmissiveMat spheres, rectangles, Rect3d
        faces, disks and mesh triangles — picked in proportion to area x power.  Without light_sampling it does nothing;
        fw_render_aovs ignores it."""
        self.settings["flags"] = (self.settings["flags"] | A.FW_FLAG_ALL_EMITTERS) if on else (
            self.settings["flags"] & ~A.FW_FLAG_ALL_EMITTERS)
        return self

    def count_deposits(self, on=True):
        """FW_FLAG_COUNT_DEPOSITS: fw_stats.deposits / bytes_shade become exact where zero deposits are elided (one extra pass)."""
        self.settings["flags"] = (self.settings["flags"] | A.FW_FLAG_COUNT_DEPOSITS) if on else (
            self.settings["flags"] & ~A.FW_FLAG_COUNT_DEPOSITS)
        return self

    def to_params(self, pixel_ids: Optional[np.ndarray] = None, rng_mode: int = A.FW_RNG_CTR) -> A.fw_render_params:
        s = self.settings
        p = A.fw_render_params()
        p.width, p.height, p.samples = s["width"], s["height"], s["samples"]
        p.gamma = s["gamma"]
        p.use_bvh = int(s["use_bvh"])
        p.multithreaded = int(s["multithreaded"])
        p.camera = self._camera.to_abi()
        p.seed = s["seed"]
        p.rng_mode = rng_mode
        p.paths_per_batch = s["paths_per_batch"]
        p.flags = s["flags"]
        if pixel_ids is not None:
            p.pixel_ids = pixel_ids.ctypes.data_as(C.POINTER(C.c_uint32))
            p.n_pixels = int(pixel_ids.shape[0])
        return p

    def render_full(self, scene, pixel_ids: Optional[Sequence[int]] = None, device: int = 0) -> RenderResult:
        """`Renderer::render` + the float buffers and counters the parity tests and bench need."""
        from . import _lib
        sd = scene if isinstance(scene, SceneDesc) else scene.to_desc()
        ids = None if pixel_ids is None else np.ascontiguousarray(np.asarray(pixel_ids, dtype=np.uint32))
        if getattr(sd, "lights", None):      # fw_render_scene takes a bare description, which carries no lights: a resident scene does
            ds = _lib.DeviceScene(sd, device)
            try:
                return ds.render(self, ids)
            finally:
                ds.close()
        return _lib.render_scene(sd, self, ids, device)

    def render_progressive(self, scene, passes: int, device: int = 0, checkpoint: Optional[str] = None):
        """Progressive preview / resumable render (not in the reference): yields a RenderResult after each of
        `passes` passes that split the samples evenly; the last one is bit-identical to `render_full`.  With `checkpoint`
        (an .npz path) the accumulation buffer is saved after every pass and a matching file is resumed from."""
        import copy
        from . import _lib
        sd = scene if isinstance(scene, SceneDesc) else scene.to_desc()
        s = self.settings
        total, n = int(s["samples"]), int(s["width"]) * int(s["height"])
        passes = max(1, min(int(passes), total))
        accum, done = np.zeros((n, 4), np.float32), 0
        # what the accumulated sums depend on: image size, seed, the scene's content, the camera and use_bvh (the hit of a
        # ray that grazes a padded box can differ between the linear scan and the BVH, as in the reference).  gamma and the
        # total sample count do not enter the sums.
        import hashlib
        import os
        import sys
        cam = self._camera.to_abi()
        # ... and on the build: an accumulation buffer written by other kernels (another ABI, other kernel sources) must not be blended in
        tag = hashlib.sha256(repr((int(s["width"]), int(s["height"]), int(s["seed"]), bool(s["use_bvh"]), sd.content_hash(),
                                   bytes(cam), int(A.FW_ABI_VERSION), int(A.FW_RNG_CTR), _lib.build_id())).encode()).hexdigest()
        if checkpoint and not str(checkpoint).endswith(".npz"):
            checkpoint = str(checkpoint) + ".npz"                       # the name np.savez would write
        if checkpoint and os.path.exists(checkpoint):
            try:
                with np.load(checkpoint) as ck:
                    ok = ck["accum"].shape == accum.shape and str(ck["tag"]) == tag and 0 < int(ck["done"]) <= total
                    if ok:
                        accum, done = np.ascontiguousarray(ck["accum"], dtype=np.float32), int(ck["done"])
                    else:
                        print(f"checkpoint {checkpoint}: written for another scene, camera, size, seed or use_bvh "
                              f"(or holds more samples than asked for) - ignored, starting from sample 0", file=sys.stderr)
            except Exception as e:                                      # truncated or foreign file
                print(f"checkpoint {checkpoint}: unreadable ({type(e).__name__}: {e}) - ignored, starting from sample 0", file=sys.stderr)
        ds = _lib.DeviceScene(sd, device)
        try:
            bounds = [round(total * k / passes) for k in range(passes + 1)]
            for k in range(passes):
                lo, hi = max(bounds[k], done), bounds[k + 1]
                if hi <= lo:
                    continue
                r = copy.copy(self); r.settings = dict(self.settings); r.settings["samples"] = hi - lo
                res = ds.render_progressive(r, lo, accum)
                done = hi
                if checkpoint:                                          # atomic: a kill during the write leaves the old file
                    tmp = f"{checkpoint}.tmp.{os.getpid()}"
                    with open(tmp, "wb") as f:
                        np.savez(f, accum=accum, done=np.int64(done), tag=np.array(tag))
                    os.replace(tmp, checkpoint)
                yield res
        finally:
            ds.close()

    def render_adaptive(self, scene, tolerance: float, min_samples: int = 16, device: int = 0, out: Optional[dict] = None) -> "AdaptiveResult":
        """Adaptive sampling (not in the reference; fw_render_adaptive): every pixel gets `min_samples` samples, then the pixels whose
        noise estimate does not yet meet `tolerance` go on in rounds that double their count, up to settings["samples"].  Each pixel's
        outputs equal bit for bit a fixed-count render at its final count (AdaptiveResult.counts).  `scene`: a Scene, a SceneDesc or an
        uploaded _lib.DeviceScene; out: device tensors to fill (see _lib.DeviceScene.render_adaptive)."""
        from . import _lib
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            return ds.render_adaptive(self, tolerance, min_samples, out=out)
        finally:
            if ds is not scene:
                ds.close()

    def render_views(self, scene, cameras, device: int = 0, pixel_ids: Optional[Sequence[int]] = None) -> ViewsResult:
        """Several camera views in one call (not in the reference; fw_render_views): view v equals bit for bit render_full() with
        camera cameras[v]; this renderer's own camera is not used.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene.
        Returns a ViewsResult: rgb8 (V, H, W, 3), or (V, N, 3) for a pixel subset."""
        from . import _lib
        ids = None if pixel_ids is None else np.ascontiguousarray(np.asarray(pixel_ids, dtype=np.uint32))
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            return ds.render_views(self, list(cameras), ids)
        finally:
            if ds is not scene:
                ds.close()

    def render_rays(self, scene, rays, samples: Optional[int] = None, first_sample: int = 0, accum=None, keys=None, key_base: int = 0,
                    device: int = 0, stream=None) -> RaysResult:
        """Radiance along caller-supplied rays (not in the reference; fw_render_rays) with this renderer's seed, use_bvh, gamma, batch
        size and flags; its camera, size and sample count are not used.  rays: (S, N, 6) per sample (S = samples, default S) or (N, 6)
        for the same rays in every sample (samples then defaults to settings["samples"]); numpy arrays or device tensors.  See
        _lib.DeviceScene.render_rays.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        from . import _lib
        s = self.settings
        if samples is None:
            samples = int(rays.shape[0]) if len(rays.shape) == 3 else int(s["samples"])
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            return ds.render_rays(rays, samples, first_sample, accum, keys, key_base, seed=s["seed"], use_bvh=s["use_bvh"], gamma=s["gamma"],
                                  stream=stream, paths_per_batch=s["paths_per_batch"], flags=s["flags"])
        finally:
            if ds is not scene:
                ds.close()

    def render_camera_model(self, scene, model, samples: int, chunk: int = 64, device: int = 0) -> RaysResult:
        """A camera model of the caller's rendered through fw_render_rays: model(sample) returns the (N, 6) rays of one absolute sample
        (numpy, or device tensors), e.g. functools.partial(panorama_rays, position, W, H) with seed=... bound.  The samples
        [0, samples) are rendered in chunks of `chunk`, accumulated in one (N, 4) buffer; any chunk size gives the same bits.  Returns
        the last chunk's RaysResult (the whole image)."""
        from . import _lib
        samples, chunk = int(samples), max(1, int(chunk))
        if samples < 1:
            raise ValueError("samples must be >= 1")
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            accum, res = None, None
            for lo in range(0, samples, chunk):
                hi = min(samples, lo + chunk)
                batch = [model(k) for k in range(lo, hi)]
                if type(batch[0]).__module__.startswith("torch"):
                    import torch
                    rays = torch.stack(batch).contiguous()
                else:
                    rays = np.ascontiguousarray(np.stack([np.asarray(b, np.float32) for b in batch]))
                res = self.render_rays(ds, rays, hi - lo, lo, accum)
                accum = res.accum
            return res
        finally:
            if ds is not scene:
                ds.close()

    def render_model(self, scene, model: "CameraModel", samples: int, first_sample: int = 0, accum=None, chunk: int = 0, device: int = 0,
                     stream=None, on_device: bool = False) -> RaysResult:
        """A CameraModel rendered on the device (not in the reference; fw_render_model): the model's rays of the samples
        [first_sample, first_sample + samples) are generated by k_model_rays, `chunk` samples at a time (0: as many as fit 256 MiB),
        and rendered with this renderer's seed, use_bvh, gamma, batch size and flags; its camera, size and sample count are not used.
        Bit for bit render_rays() over _lib.model_rays(model), for every chunk.  accum and on_device as _lib.DeviceScene.render_model.
        `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene.  The image is result.image(model.width, model.height)."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            return ds.render_model(model, samples, first_sample, accum, seed=s["seed"], use_bvh=s["use_bvh"], gamma=s["gamma"], stream=stream,
                                   paths_per_batch=s["paths_per_batch"], flags=s["flags"], chunk=chunk, on_device=on_device)
        finally:
            if ds is not scene:
                ds.close()

    def bake_probes(self, scene, probes: "ProbeSet", rounds: int = 1, first_round: int = 0, sums=None, chunk=None, device: int = 0, stream=None,
                    on_device: bool = False):
        """Irradiance probes baked on the device (not in the reference; fw_bake_probes): `rounds` rounds of the set's rays, each
        rendered with settings["samples"] paths per direction and this renderer's seed (+ the round), use_bvh, batch size and flags —
        lights and light sampling included; its camera, size and gamma are not used — and projected onto nine SH coefficients per
        probe and channel.  Returns (sh, sums): (N, 9, 3) float32 each, sh = sums / (first_round + rounds); pass sums back with
        first_round = the rounds it holds to add more.  on_device and chunk as _lib.DeviceScene.bake_probes; the call's stats are kept
        in self.probe_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            sh, sums, self.probe_stats = ds.bake_probes(probes, rounds, s["samples"], first_round, sums, seed=s["seed"], use_bvh=s["use_bvh"],
                                                        stream=stream, paths_per_batch=s["paths_per_batch"], flags=s["flags"], chunk=chunk,
                                                        on_device=on_device)
            return sh, sums
        finally:
            if ds is not scene:
                ds.close()

    def bake_probe_depth(self, scene, probes: "ProbeSet", depth: "ProbeDepth", rounds: int = 1, first_round: int = 0, sums=None, chunk=None,
                         device: int = 0, stream=None, on_device: bool = False):
        """The depth maps of a probe set baked on the device (not in the reference; fw_bake_probe_depth): `rounds` rounds
        of the set's rays traced with this renderer's seed (+ the round), use_bvh and flags, their hit distances reduced to two moments
        per texel of every probe's octahedral map.  Returns (moments, sums): (N, R, R, 2) and (N, R, R, 4) float32; pass sums back with
        first_round = the rounds it holds to add more.  on_device and chunk as _lib.DeviceScene.bake_probe_depth; the call's stats are
        kept in self.probe_depth_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            moments, sums, self.probe_depth_stats = ds.bake_probe_depth(probes, depth, rounds, first_round, sums, seed=s["seed"],
                                                                        use_bvh=s["use_bvh"], stream=stream, flags=s["flags"], chunk=chunk,
                                                                        on_device=on_device)
            return moments, sums
        finally:
            if ds is not scene:
                ds.close()

    def bake_probe_radiance(self, scene, probes: "ProbeSet", pr: "ProbeRadiance", rounds: int = 1, first_round: int = 0, sums=None,
                            on_device: bool = False, chunk=0, with_sh: bool = False, sh_sums=None, device: int = 0, stream=None):
        """The radiance maps of a probe set baked on the device (not in the reference; fw_bake_probe_radiance): bake_probes'
        rounds — the same rays, rendered with settings["samples"] paths per direction and this renderer's seed (+ the round), use_bvh,
        batch size and flags — reduced into every probe's octahedral map and prefiltered for the roughness chain of pr.  Returns (maps,
        sums): (N, M, 4) and (N, R, R, 4) float32; pass sums back with first_round = the rounds it holds to add more.  with_sh: the same
        rendered rays are also projected as bake_probes projects them, and (maps, sums, sh, sh_sums) is returned (sh_sums: bake_probes'
        running sums to add to).  on_device and chunk as _lib.DeviceScene.bake_probe_radiance; the call's stats are kept in
        self.probe_radiance_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            out = ds.bake_probe_radiance(probes, pr, rounds, s["samples"], first_round, sums, sh_sums, with_sh, seed=s["seed"], use_bvh=s["use_bvh"],
                                         stream=stream, paths_per_batch=s["paths_per_batch"], flags=s["flags"], chunk=chunk, on_device=on_device)
            self.probe_radiance_stats = out[-1]
            return out[:-1]
        finally:
            if ds is not scene:
                ds.close()

    def relocate_probes(self, scene, probes: "ProbeSet", relocation: "ProbeRelocation", first_step: int = 0, placement=None, chunk=None,
                        device: int = 0, stream=None):
        """Probes moved out of geometry and classified on the device (not in the reference; fw_relocate_probes):
        relocation.steps moving steps from `first_step`, each tracing the set's rays from the moved positions with this renderer's seed
        (+ the step), use_bvh and flags, then one classifying step.  Returns (placement, survey): (N, 4) float32 records (ox, oy, oz, a)
        and the classifying step's survey (N, 3, 4) float32; pass placement back with first_step = the steps it holds to go on.  Bake sh
        and depth maps at probes.moved(placement) and hand placement to render_probe_lit.  The call's stats are kept in
        self.probe_place_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            placement, survey, self.probe_place_stats = ds.relocate_probes(probes, relocation, None, first_step, placement, seed=s["seed"],
                                                                           use_bvh=s["use_bvh"], stream=stream, flags=s["flags"], chunk=chunk)
            return placement, survey
        finally:
            if ds is not scene:
                ds.close()

    def bake_lightmap(self, scene, lightmap: "Lightmap", rounds: int = 1, dilate: int = 2, first_round: int = 0, sums=None, chunk=None,
                      device: int = 0, stream=None, on_device: bool = False, direct: "DirectLight" = None):
        """A lightmap baked on the device (not in the reference; fw_bake_lightmap): `rounds` rounds of the lightmap's cosine-weighted
        rays, each rendered with settings["samples"] paths per direction and this renderer's seed (+ the round), use_bvh, batch size and
        flags — lights and light sampling included; its camera, size and gamma are not used — and reduced to the irradiance of every
        covered texel.  Returns (irradiance, sums): (H, W, 4) float32 each; irradiance rgb = sums / (first_round + rounds) with a = 1 on
        covered texels, then `dilate` dilation passes (a = 0.5 on filled texels, 0 elsewhere); pass sums back with first_round = the
        rounds it holds to add more.  on_device and chunk as _lib.DeviceScene.bake_lightmap; the call's stats are kept in
        self.lightmap_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene.  direct (a DirectLight with the cosine lobe;
        DESIGN.md §9w): what a lightmap's rays cannot hit — the scene's point, spot and directional lights at the texel itself — is
        added.  fw_bake_lightmap runs with 0 dilation passes; fw_bake_direct runs one round on fw_lightmap_texels' records and covered
        list in place; irradiance.rgb += E on the covered texels in float32; then fw_lightmap_dilate runs `dilate` passes.  sums stay
        the rays' own.  E (H, W, 3) is kept in self.lightmap_direct and the call's stats in self.direct_stats.  Another lobe:
        ValueError.  direct=None: the calls and the bits above."""
        from . import _lib
        s = self.settings
        if direct is not None and direct.check().lobe != "cosine":
            raise ValueError('a lightmap holds irradiance: direct needs the lobe "cosine"')
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            irr, sums, self.lightmap_stats = ds.bake_lightmap(lightmap, rounds, s["samples"], first_round, sums, dilate if direct is None else 0,
                                                              seed=s["seed"], use_bvh=s["use_bvh"], stream=stream,
                                                              paths_per_batch=s["paths_per_batch"], flags=s["flags"], chunk=chunk, on_device=on_device)
            if direct is not None:
                import torch
                w, h = int(lightmap.width), int(lightmap.height)
                rec, owner, count = _lib.lightmap_texels(lightmap, ds.device, on_device=True)
                if count == 0:
                    raise ValueError("the lightmap covers no texel")
                ids = torch.nonzero(owner != -1).flatten().to(torch.int32).contiguous()          # ascending: the covered list
                out, _dsums, self.direct_stats = ds.bake_direct(direct, rec[:, 0:3], rec[:, 4:7], ids, None, None, 1, seed=s["seed"],
                                                                use_bvh=s["use_bvh"], flags=s["flags"])
                host = not type(irr).__module__.startswith("torch")
                image = (torch.from_numpy(np.ascontiguousarray(irr)).to(rec.device) if host else irr).reshape(h * w, 4)
                at = ids.long()
                image[at, 0:3] = image[at, 0:3] + out[at, 0:3]
                image = _lib.lightmap_dilate(image.reshape(h, w, 4), dilate, ds.device)
                self.lightmap_direct = out[:, 0:3].reshape(h, w, 3).cpu().numpy()
                irr = image.cpu().numpy() if host else image
            return irr, sums
        finally:
            if ds is not scene:
                ds.close()

    def render_ao(self, scene, ao: "AmbientOcclusion", rounds: int = 1, samples: int = 1, device: int = 0):
        """Ambient occlusion and bent normals of this renderer's view (not in the reference; fw_bake_ao): the first-hit
        guide buffers (fw_render_aovs at `samples` samples) stay on the device, and fw_bake_ao reads each pixel's position and normal from
        the records in place, tracing `rounds` rounds of ao.directions rays with this renderer's seed (+ the round), use_bvh and flags.
        Returns (ao (H, W), bent (H, W, 3), sums (H, W, 4)) float32 host arrays; a pixel that missed the scene has ao 1 and bent 0.  The
        call's stats are kept in self.ao_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        ao.check()
        s = self.settings
        w, h = int(s["width"]), int(s["height"])
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=torch.device("cuda", ds.device))
            ds.aovs(self, samples, out=aov)
            out, sums, self.ao_stats = ds.bake_ao(ao, aov[:, 8:11], aov[:, 4:7], None, rounds, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        finally:
            if ds is not scene:
                ds.close()
        out = out.cpu().numpy().reshape(h, w, 4)
        return out[..., 3], out[..., 0:3], sums.cpu().numpy().reshape(h, w, 4)

    def bake_lightmap_ao(self, scene, lightmap: "Lightmap", ao: "AmbientOcclusion", rounds: int = 1, dilate: int = 2, device: int = 0):
        """An ambient-occlusion map over a lightmap's texels (not in the reference; fw_bake_ao): fw_lightmap_texels'
        records and covered list stay on the device and are read in place; ao.directions, seed, jitter and bias count, the lightmap's
        own do not.  Returns (ao (H, W), bent (H, W, 3), sums (H, W, 4)) float32 host arrays: ao of the covered texels packed as
        (ao, ao, ao, 1) and passed through `dilate` passes of fw_lightmap_dilate (texels no pass reaches stay 0); bent and sums are
        not dilated.  The call's stats are kept in self.ao_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        ao.check()
        s = self.settings
        w, h = int(lightmap.width), int(lightmap.height)
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            rec, owner, count = _lib.lightmap_texels(lightmap, ds.device, on_device=True)
            if count == 0:
                raise ValueError("the lightmap covers no texel")
            ids = torch.nonzero(owner != -1).flatten().to(torch.int32).contiguous()          # ascending: the covered list
            out, sums, self.ao_stats = ds.bake_ao(ao, rec[:, 0:3], rec[:, 4:7], ids, rounds, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
            image = torch.zeros((h * w, 4), dtype=torch.float32, device=rec.device)
            at = ids.long()
            image[at] = torch.cat([out[at, 3:4].expand(-1, 3), torch.ones_like(out[at, 3:4])], dim=1)
            image = _lib.lightmap_dilate(image.reshape(h, w, 4), dilate, ds.device)
        finally:
            if ds is not scene:
                ds.close()
        return image[..., 0].cpu().numpy(), out[:, 0:3].cpu().numpy().reshape(h, w, 3), sums.cpu().numpy().reshape(h, w, 4)

    def _direct_term(self, ds, direct: "DirectLight", aov, model, rays=None):
        """(term (N, 3), out (N, 8), spec (N, 4), rays (N, 6)) device tensors: the direct light of the resident scene's point, spot and
        directional lights at the pixels of the records `aov`.  The view's sample-0 rays (fw_camera_rays; with `model`,
        fw_model_rays; or `rays`, already made) are traced by fw_trace_rays; each hit's material gives the pixel's (F0, rho)
        (material_direct_table) and the rays' directions the view; fw_bake_direct runs one round on the records in place.  In float32,
        term = a ((v E) float32(1 / pi)) for a pixel with !(rho > 0) and v S for a glossy one.  The call's stats are kept in
        self.direct_stats."""
        import torch
        from . import _lib
        s = self.settings
        dev = aov.device
        n = int(aov.shape[0])
        if rays is None:
            if model is not None:
                rays = _lib.model_rays(model, 0, 1, ds.device, out=torch.empty((1, n, 6), dtype=torch.float32, device=dev))[0]
            else:
                rays = torch.from_numpy(ds.camera_rays(self, 0)).to(dev)
        hit = _lib.hit_fields(ds.trace(rays, s["use_bvh"], seed=s["seed"]))
        table = torch.from_numpy(material_direct_table(ds._desc)).to(dev)
        miss = torch.full_like(hit["material"], table.shape[0] - 1)
        spec = table[torch.where(hit["object"] == -1, miss, hit["material"]).long()].contiguous()
        out, _sums, self.direct_stats = ds.bake_direct(direct, aov[:, 8:11], aov[:, 4:7], None, rays[:, 3:6], spec, 1, seed=s["seed"],
                                                       use_bvh=s["use_bvh"], flags=s["flags"])
        v = aov[:, 3:4]
        term = torch.where(spec[:, 3:4] > 0, v * out[:, 4:7], aov[:, 0:3] * ((v * out[:, 0:3]) * float(np.float32(1.0 / np.pi))))
        return term, out, spec, rays

    def render_direct(self, scene, direct: "DirectLight", aov_samples: int = 1, model: "CameraModel" = None, device: int = 0) -> RenderResult:
        """The direct light of the scene's point, spot and directional lights in this renderer's view (not in the reference;
        fw_bake_direct): sharp shadows and GgxMat highlights without a path.  The first-hit guide buffers (fw_render_aovs
        at `aov_samples` samples; with `model`, fw_render_model_aovs) stay on the device; _direct_term gives the frame, resolved by
        fw_denoise at 0 iterations.  Area emitters and the environment are not in it: probes and lightmaps hold them.  The call's stats
        are kept in self.direct_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        direct.check()
        s = self.settings
        w, h = (int(model.width), int(model.height)) if model is not None else (int(s["width"]), int(s["height"]))
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=torch.device("cuda", ds.device))
            if model is not None:
                ds.model_aovs(model, aov_samples, seed=s["seed"], use_bvh=s["use_bvh"], out=aov)
            else:
                ds.aovs(self, aov_samples, out=aov)
            term = self._direct_term(ds, direct, aov, model)[0]
            rgb8, gam, lin = _lib.denoise(term.contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            stats = dict(ds.aovs_stats)
        finally:
            if ds is not scene:
                ds.close()
        return RenderResult(rgb8.cpu().numpy(), gam.cpu().numpy(), lin.cpu().numpy(), stats, w, h)

    def _area(self, ds, area: "AreaLight", rounds, aov):
        """(out (N, 4), sums (N, 4)) device tensors: fw_bake_area on the records `aov` in place (stride 12, aov + 8 / aov + 4) with this
        renderer's seed, use_bvh and flags.  The call's stats are kept in self.area_stats."""
        s = self.settings
        out, sums, self.area_stats = ds.bake_area(area, aov[:, 8:11], aov[:, 4:7], None, rounds, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        return out, sums

    def render_area(self, scene, area: "AreaLight", rounds: int = 1, aov_samples: int = 1, model: "CameraModel" = None, device: int = 0) -> RenderResult:
        """This renderer's view lit by the scene's sampled area lights alone — every EmissiveMat sphere and axis-aligned rectangle — by
        light sampling (not in the reference; fw_bake_area): soft shadows without a path.  The first-hit guide buffers
        (fw_render_aovs at `aov_samples` samples; with `model`, fw_render_model_aovs) stay on the device and fw_bake_area reads each
        pixel's position and normal from the records in place, `rounds` rounds of area.samples shadow rays per light with this
        renderer's seed (+ the round), use_bvh and flags.  With E its out the frame is, as render_direct composes a diffuse pixel,
        a ((v E) float32(1 / pi)) in float32, resolved by fw_denoise at 0 iterations.  The emitters themselves, every other emitter, the
        environment and indirect light are not in it.  The call's stats are kept in self.area_stats.  `scene`: a Scene, a SceneDesc or
        an uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        area.check()
        s = self.settings
        w, h = (int(model.width), int(model.height)) if model is not None else (int(s["width"]), int(s["height"]))
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=torch.device("cuda", ds.device))
            if model is not None:
                ds.model_aovs(model, aov_samples, seed=s["seed"], use_bvh=s["use_bvh"], out=aov)
            else:
                ds.aovs(self, aov_samples, out=aov)
            E = self._area(ds, area, rounds, aov)[0]
            term = aov[:, 0:3] * ((aov[:, 3:4] * E[:, 0:3]) * float(np.float32(1.0 / np.pi)))
            rgb8, gam, lin = _lib.denoise(term.contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            stats = dict(ds.aovs_stats)
        finally:
            if ds is not scene:
                ds.close()
        return RenderResult(rgb8.cpu().numpy(), gam.cpu().numpy(), lin.cpu().numpy(), stats, w, h)

    def _emitters(self, ds, emitters: "EmitterLights", rounds, aov):
        """(out (N, 4), sums (N, 4)) device tensors: fw_bake_emitters on the records `aov` in place (stride 12, aov + 8 / aov + 4) with
        this renderer's seed, use_bvh and flags.  The call's stats are kept in self.emitters_stats."""
        s = self.settings
        out, sums, self.emitters_stats = ds.bake_emitters(emitters, aov[:, 8:11], aov[:, 4:7], None, rounds, seed=s["seed"], use_bvh=s["use_bvh"],
                                                          flags=s["flags"])
        return out, sums

    def render_emitters(self, scene, emitters: "EmitterLights", rounds: int = 1, aov_samples: int = 1, model: "CameraModel" = None,
                        device: int = 0) -> RenderResult:
        """This renderer's view lit by every emitter of the scene alone — spheres, rectangles, Rect3d faces, disks and mesh triangles —
        by light sampling with the emitter picked by power (not in the reference; fw_bake_emitters).  Composed exactly
        as render_area composes: the first-hit guide buffers stay on the device, fw_bake_emitters reads each pixel's position and normal
        from the records in place, `rounds` rounds of emitters.samples shadow rays, and with E its out the frame is a ((v E) float32(1 /
        pi)) in float32, resolved by fw_denoise at 0 iterations.  The call's stats are kept in self.emitters_stats.  `scene`: a Scene,
        a SceneDesc or an uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        emitters.check()
        s = self.settings
        w, h = (int(model.width), int(model.height)) if model is not None else (int(s["width"]), int(s["height"]))
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=torch.device("cuda", ds.device))
            if model is not None:
                ds.model_aovs(model, aov_samples, seed=s["seed"], use_bvh=s["use_bvh"], out=aov)
            else:
                ds.aovs(self, aov_samples, out=aov)
            E = self._emitters(ds, emitters, rounds, aov)[0]
            term = aov[:, 0:3] * ((aov[:, 3:4] * E[:, 0:3]) * float(np.float32(1.0 / np.pi)))
            rgb8, gam, lin = _lib.denoise(term.contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            stats = dict(ds.aovs_stats)
        finally:
            if ds is not scene:
                ds.close()
        return RenderResult(rgb8.cpu().numpy(), gam.cpu().numpy(), lin.cpu().numpy(), stats, w, h)

    def _gather(self, ds, gather: "FinalGather", rounds, grid, d_sh, aov, depth, d_mom, normal_bias, d_pl, direct=None, no_lights=False,
                no_emitters=False):
        """(out (N, 4), sums (N, 4)) device tensors: fw_bake_gather on the records `aov` in place (stride 12, aov + 8 / aov + 4) with this
        renderer's seed, use_bvh and flags; with `direct`, a DirectLight, FW_GATHER_DIRECT with its bias; with no_lights,
        FW_GATHER_NO_LIGHTS; with no_emitters, FW_GATHER_NO_EMITTERS.  The call's stats are kept in self.gather_stats."""
        import copy
        s = self.settings
        g = copy.copy(gather)
        if no_lights:
            g.no_lights = True
        if no_emitters:
            g.no_emitters = True
        if direct is not None:
            g.direct, g.direct_bias = True, direct.bias
        out, sums, self.gather_stats = ds.bake_gather(g, grid, d_sh, aov[:, 8:11], aov[:, 4:7], None, depth, d_mom, normal_bias, d_pl, rounds,
                                                      seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        return out, sums

    def render_gather(self, scene, gather: "FinalGather", probes, sh, rounds: int = 1, samples: int = 1, wrap: bool = True, device: int = 0,
                      depth: "ProbeDepth" = None, moments=None, normal_bias: float = 0.0, placement=None):
        """The irradiance gathered at this renderer's view from baked probes (not in the reference; fw_bake_gather): the
        first-hit guide buffers (fw_render_aovs at `samples` samples) stay on the device, and fw_bake_gather reads each pixel's position
        and normal from the records in place, tracing `rounds` rounds of gather.directions rays with this renderer's seed (+ the round),
        use_bvh and flags; probes, sh, depth, moments, normal_bias and placement as render_probe_lit takes them.  Returns (E (H, W, 3),
        sky (H, W), sums (H, W, 4)) float32 host arrays; a pixel that missed the scene has E 0 and sky 0.  The call's stats are kept in
        self.gather_stats.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        gather.check()
        if depth is not None and moments is None:
            raise ValueError("depth needs the moments bake_probe_depth returned")
        grid = ProbeGrid.of(probes, wrap)
        s = self.settings
        w, h = int(s["width"]), int(s["height"])
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            dev = torch.device("cuda", ds.device)
            to = lambda a, shape: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))).to(dev)
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=dev)
            ds.aovs(self, samples, out=aov)
            R = int(depth.resolution) if depth is not None else 0
            out, sums = self._gather(ds, gather, rounds, grid, to(sh, (grid.n_probes, 9, 3)), aov, depth,
                                     to(moments if depth is not None else None, (grid.n_probes, R, R, 2)), normal_bias, to(placement, (grid.n_probes, 4)))
        finally:
            if ds is not scene:
                ds.close()
        out = out.cpu().numpy().reshape(h, w, 4)
        return out[..., 0:3], out[..., 3], sums.cpu().numpy().reshape(h, w, 4)

    def _view_spec(self, ds, model, w, h, dev):
        """(rays (N, 6), spec (N, 4)) device tensors of the glossy shades: the view's sample-0 rays (fw_camera_rays; with `model`,
        fw_model_rays) traced by fw_trace_rays, and each hit's (F0, rho) from material_spec_table — rho = 0 for a miss"""
        import torch
        from . import _lib
        s = self.settings
        if model is not None:
            rays = _lib.model_rays(model, 0, 1, ds.device, out=torch.empty((1, w * h, 6), dtype=torch.float32, device=dev))[0]
        else:
            rays = torch.from_numpy(ds.camera_rays(self, 0)).to(dev)
        hit = _lib.hit_fields(ds.trace(rays, s["use_bvh"], seed=s["seed"]))
        table = torch.from_numpy(material_spec_table(ds._desc)).to(dev)
        miss = torch.full_like(hit["material"], table.shape[0] - 1)
        return rays, table[torch.where(hit["object"] == -1, miss, hit["material"]).long()].contiguous()

    def _reflect(self, ds, reflect: "ReflectionGather", rounds, grid, d_sh, aov, rays, spec, depth, d_mom, normal_bias, d_pl, direct=None):
        """(out (N, 4), sums (N, 8)) device tensors: fw_bake_reflect on the records `aov` in place (stride 12, aov + 8 / aov + 4) with the
        view rays[:, 3:6] and `spec`, this renderer's seed, use_bvh and flags; with `direct`, a DirectLight, FW_REFLECT_DIRECT with its
        bias.  The call's stats are kept in self.reflect_stats."""
        import copy
        s = self.settings
        g = copy.copy(reflect)
        if direct is not None:
            g.direct_bias(direct.bias)
        out, sums, self.reflect_stats = ds.bake_reflect(g, grid, d_sh, aov[:, 8:11], aov[:, 4:7], rays[:, 3:6], spec, None, depth, d_mom, normal_bias,
                                                        d_pl, rounds, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"])
        return out, sums

    def render_reflect(self, scene, reflect: "ReflectionGather", probes, sh, rounds: int = 1, samples: int = 1, wrap: bool = True, device: int = 0,
                       depth: "ProbeDepth" = None, moments=None, normal_bias: float = 0.0, placement=None):
        """The radiance reflected towards this renderer's view by its glossy pixels, from baked probes (not in the reference;
        fw_bake_reflect): the first-hit guide buffers (fw_render_aovs at `samples` samples) stay on the device, view
        and spec are built as render_probe_lit's radiance branch builds them (the sample-0 rays traced, material_spec_table), and
        fw_bake_reflect reads each pixel from the records in place, tracing `rounds` rounds of reflect.directions rays with this
        renderer's seed (+ the round), use_bvh and flags; probes, sh, depth, moments, normal_bias and placement as render_probe_lit
        takes them.  Returns (S (H, W, 3), alive (H, W), sums (H, W, 8)) float32 host arrays; a pixel that is not glossy (rho = 0) or
        missed the scene has S 0 and alive 0.  The call's stats are kept in self.reflect_stats.  `scene`: a Scene, a SceneDesc or an
        uploaded _lib.DeviceScene."""
        import torch
        from . import _lib
        reflect.check()
        if depth is not None and moments is None:
            raise ValueError("depth needs the moments bake_probe_depth returned")
        grid = ProbeGrid.of(probes, wrap)
        s = self.settings
        w, h = int(s["width"]), int(s["height"])
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            dev = torch.device("cuda", ds.device)
            to = lambda a, shape: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))).to(dev)
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=dev)
            ds.aovs(self, samples, out=aov)
            rays, spec = self._view_spec(ds, None, w, h, dev)
            R = int(depth.resolution) if depth is not None else 0
            out, sums = self._reflect(ds, reflect, rounds, grid, to(sh, (grid.n_probes, 9, 3)), aov, rays, spec, depth,
                                      to(moments if depth is not None else None, (grid.n_probes, R, R, 2)), normal_bias, to(placement, (grid.n_probes, 4)))
        finally:
            if ds is not scene:
                ds.close()
        out = out.cpu().numpy().reshape(h, w, 4)
        return out[..., 0:3], out[..., 3], sums.cpu().numpy().reshape(h, w, 8)

    def render_probe_lit(self, scene, probes, sh, aov_samples: int = 8, wrap: bool = True, device: int = 0, model: "CameraModel" = None,
                         depth: "ProbeDepth" = None, moments=None, normal_bias: float = 0.0, ao: "AmbientOcclusion" = None,
                         ao_rounds: int = 1, placement=None, radiance: "ProbeRadiance" = None, maps=None,
                         direct: "DirectLight" = None, ggx_table: "GgxTable" = None, table=None, gather: "FinalGather" = None,
                         gather_rounds: int = 1, reflect: "ReflectionGather" = None, reflect_rounds: int = 1, area: "AreaLight" = None,
                         area_rounds: int = 1, emitters: "EmitterLights" = None, emitters_rounds: int = 1) -> RenderResult:
        """A preview lit from baked probes (not in the reference): the first-hit guide buffers of this renderer's view
        (fw_render_aovs at `aov_samples` samples; with `model`, a CameraModel, fw_render_model_aovs through it) shaded by fw_probe_shade
        from the probe grid `probes` (a ProbeSet made by ProbeSet.grid, or a ProbeGrid, whose own wrap then counts) and its coefficients
        sh (n, 9, 3), as bake_probes returns them.  One first-hit pass and no paths: direct and indirect diffuse light both come from the
        probes.  The records stay on the device.  A ProbeSet without a grid: ValueError.  `scene`: a Scene, a SceneDesc or an uploaded
        _lib.DeviceScene.  depth (a ProbeDepth) with moments (n, R, R, 2), as bake_probe_depth returns them: the frame is shaded by
        fw_probe_shade_vis, every probe weighted by its visibility from the surface point moved normal_bias along its normal
        (DESIGN.md §9s); depth=None: exactly the calls above.  ao (an AmbientOcclusion): fw_bake_ao runs `ao_rounds`
        rounds on the records in place; the irradiance E is looked up by fw_probe_irradiance (with depth: fw_probe_irradiance_vis) along
        the bent normal where it is not (0, 0, 0) and along the record's normal elsewhere, and not clamped; the frame is
        out_c = a_c (v (ao (E_c float32(1 / pi))) + (1 - v)) in float32, resolved by fw_denoise at 0 iterations.  ao=None: the calls and
        the bits above.  placement ((n, 4), as relocate_probes returns it): the frame is shaded by fw_probe_shade_placed
        — with ao, E is looked up by fw_probe_irradiance_placed — with or without depth; sh and moments are expected to have been baked
        at probes.moved(placement).  placement=None: the calls and the bits above.  radiance (a ProbeRadiance) with maps ((n, M, 4), as
        bake_probe_radiance returns them): conductors show reflections.  The view's sample-0 rays (fw_camera_rays; with
        `model`, fw_model_rays) are traced on the device by fw_trace_rays; each hit's material gives the pixel's (F0, rho) — a GgxMat
        (albedo, roughness), a MetalMat (albedo, roughness clipped to [0.03, 1]), every other material and every miss rho = 0 — and the
        frame is shaded by fw_probe_shade_glossy with those rays' directions as the view, with or without depth and placement.
        radiance=None: the calls and the bits above.  radiance together with ao: ValueError.  direct (a DirectLight):
        the direct light of the scene's point, spot and directional lights, which no probe holds — _direct_term's frame, fw_bake_direct
        on the records in place — is added in float32 to the linear frame of whichever branch ran and the sum resolved by fw_denoise
        at 0 iterations; with ao, only the probes' term is multiplied by ao.  The call's stats are kept in self.direct_stats.
        direct=None: the calls and the bits above.  ggx_table (a GgxTable), with radiance: the glossy pixels are shaded
        by fw_probe_shade_split — F0 A + B from the table in the place of the bare Schlick term, with ggx_table.energy the energy
        compensation — and every other pixel as before; the table is baked on the device in the call (fw_ggx_table) unless `table`,
        (n_rho, n_mu, 2) as _lib.ggx_table returns it, is passed.  ggx_table without radiance: ValueError.  ggx_table=None: the
        calls and the bits above.  gather (a FinalGather): the probes are read one bounce away instead of at the
        pixel — fw_bake_gather runs `gather_rounds` rounds on the records in place, with depth, moments, normal_bias and placement
        passed on to the lookup at the gather hits; with Eg its out, the frame is out_c = a_c (v (Eg_c float32(1 / pi)) + (1 - v))
        in float32, resolved by fw_denoise at 0 iterations.  With direct, the gather adds the delta lights at its hits as well
        (FW_GATHER_DIRECT with direct's bias), and the receivers' own term is added as above.  The call's stats are kept in
        self.gather_stats.  gather together with ao or radiance: ValueError.  gather=None: the calls and the bits above.  reflect (a
        ReflectionGather): traced reflections on conductors — view and spec are built as for radiance,
        fw_bake_reflect runs `reflect_rounds` rounds on the records in place with depth, moments, normal_bias and placement passed
        on to the lookup at the hits, and with S its out a pixel with rho > 0 becomes out_c = v S_c + (1 - v) a_c in float32 while
        every other pixel keeps the linear value of the branch above that ran (plain, depth, placement or gather); the frame is
        resolved by fw_denoise at 0 iterations.  With direct, the lights are added at the reflection rays' hits as well
        (FW_REFLECT_DIRECT with direct's bias), and the receivers' own term is added as above.  The call's stats are kept in
        self.reflect_stats.  reflect together with radiance or ao: ValueError.  reflect=None: the calls and the bits above.  area (an
        AreaLight), with gather: the final-gather split — the gather runs with FW_GATHER_NO_LIGHTS, so its rays bring
        back nothing from the scene's sampled area lights, fw_bake_area runs `area_rounds` rounds on the records in place, and its
        out's E is added in float32 to Eg before the gathered frame is shaded: out_c = a_c (v ((Eg_c + Ea_c) float32(1 / pi)) + (1 -
        v)).  The call's stats are kept in self.area_stats.  area without gather: ValueError, because the probes' SH already holds the
        emitters' direct light and adding it would count it twice.  area=None: the calls and the bits above.  emitters (an
        EmitterLights), with gather: the same split over every emitter — the gather runs with FW_GATHER_NO_EMITTERS,
        fw_bake_emitters runs `emitters_rounds` rounds on the records in place, and its out's E is added in float32 to Eg before
        shading, as area's is.  The call's stats are kept in self.emitters_stats.  emitters without gather, or together with area (a
        sphere or rectangle emitter would be sampled twice): ValueError.  emitters=None: the calls and the bits above."""
        import torch
        from . import _lib
        if emitters is not None:
            if gather is None:
                raise ValueError("emitters needs gather: the probes' SH already holds the emitters' direct light, so adding the sampled "
                                 "emitters' to a probe lookup at the pixel would count it twice")
            if area is not None:
                raise ValueError("emitters and area exclude each other: the area lights are among the emitters and would be sampled twice")
            emitters.check()
        if area is not None:
            if gather is None:
                raise ValueError("area needs gather: the probes' SH already holds the emitters' direct light, so adding the area lights' "
                                 "to a probe lookup at the pixel would count it twice")
            area.check()
        if direct is not None:
            direct.check()
        if reflect is not None:
            if ao is not None or radiance is not None:
                raise ValueError("reflect cannot be combined with radiance or ao: the traced reflections take the radiance maps' place, and "
                                 "the ambient-occlusion frame has no specular term")
            reflect.check()
        if gather is not None:
            if ao is not None or radiance is not None:
                raise ValueError("gather cannot be combined with ao or radiance: the gathered frame has neither term")
            gather.check()
        if ggx_table is not None:
            if radiance is None:
                raise ValueError("ggx_table needs radiance: the split sum's BRDF term multiplies the radiance maps' lookup")
            ggx_table.check()
        elif table is not None:
            raise ValueError("table needs the GgxTable it was baked for")
        baked = table                                                                     # (the radiance branch has a material table of its own)
        if depth is not None and moments is None:
            raise ValueError("depth needs the moments bake_probe_depth returned")
        if radiance is not None and maps is None:
            raise ValueError("radiance needs the maps bake_probe_radiance returned")
        if radiance is not None and ao is not None:
            raise ValueError("radiance and ao cannot be combined: the ambient-occlusion frame has no specular term")
        if ao is not None:
            ao.check()
        grid = ProbeGrid.of(probes, wrap)
        s = self.settings
        w, h = (int(model.width), int(model.height)) if model is not None else (int(s["width"]), int(s["height"]))
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            dev = torch.device("cuda", ds.device)
            aov = torch.empty((w * h, 12), dtype=torch.float32, device=dev)
            if model is not None:
                ds.model_aovs(model, aov_samples, seed=s["seed"], use_bvh=s["use_bvh"], out=aov)
            else:
                ds.aovs(self, aov_samples, out=aov)
            d_sh = torch.from_numpy(np.ascontiguousarray(np.asarray(sh, np.float32).reshape(grid.n_probes, 9, 3))).to(dev)
            d_mom = None
            if depth is not None:
                R = int(depth.resolution)
                d_mom = torch.from_numpy(np.ascontiguousarray(np.asarray(moments, np.float32).reshape(grid.n_probes, R, R, 2))).to(dev)
            d_pl = None
            if placement is not None:
                d_pl = torch.from_numpy(np.ascontiguousarray(np.asarray(placement, np.float32).reshape(grid.n_probes, 4))).to(dev)
            rays = None
            if gather is not None:
                Eg = self._gather(ds, gather, gather_rounds, grid, d_sh, aov, depth, d_mom, normal_bias, d_pl, direct, area is not None,
                                  emitters is not None)[0][:, 0:3]
                if area is not None:
                    Eg = Eg + self._area(ds, area, area_rounds, aov)[0][:, 0:3]
                if emitters is not None:
                    Eg = Eg + self._emitters(ds, emitters, emitters_rounds, aov)[0][:, 0:3]
                v = aov[:, 3:4]
                lit = aov[:, 0:3] * (v * (Eg * float(np.float32(1.0 / np.pi))) + (1.0 - v))
                rgb8, gam, lin = _lib.denoise(lit.contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            elif ao is not None:
                occ, _sums, self.ao_stats = ds.bake_ao(ao, aov[:, 8:11], aov[:, 4:7], None, ao_rounds, seed=s["seed"], use_bvh=s["use_bvh"],
                                                       flags=s["flags"])
                bent = torch.any(occ[:, 0:3] != 0, dim=1, keepdim=True)
                pos, nrm = aov[:, 8:11].contiguous(), torch.where(bent, occ[:, 0:3], aov[:, 4:7]).contiguous()
                if d_pl is not None:
                    E = _lib.probe_irradiance_placed(grid, d_sh, d_pl, pos, nrm, depth, d_mom, normal_bias, device=ds.device)
                elif depth is not None:
                    E = _lib.probe_irradiance_vis(grid, d_sh, depth, d_mom, pos, nrm, normal_bias, device=ds.device)
                else:
                    E = _lib.probe_irradiance(grid, d_sh, pos, nrm, device=ds.device)
                v = aov[:, 3:4]
                lit = aov[:, 0:3] * (v * (occ[:, 3:4] * (E * float(np.float32(1.0 / np.pi)))) + (1.0 - v))
                rgb8, gam, lin = _lib.denoise(lit.contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            elif radiance is not None:
                d_maps = torch.from_numpy(np.ascontiguousarray(np.asarray(maps, np.float32).reshape(grid.n_probes, radiance.texels, 4))).to(dev)
                rays, spec = self._view_spec(ds, model, w, h, dev)
                if ggx_table is not None:
                    if baked is None:
                        d_tab = _lib.ggx_table(ggx_table, device=ds.device,
                                               out=torch.empty((ggx_table.n_rho, ggx_table.n_mu, 2), dtype=torch.float32, device=dev))
                    else:
                        d_tab = torch.from_numpy(np.ascontiguousarray(np.asarray(baked, np.float32).reshape(ggx_table.n_rho, ggx_table.n_mu, 2))).to(dev)
                    rgb8, gam, lin = _lib.probe_shade_split(grid, d_sh, radiance, d_maps, aov, spec, rays[:, 3:6], d_tab, w, h, ggx_table.flags, depth,
                                                            d_mom, normal_bias, d_pl, s["gamma"], ds.device)
                else:
                    rgb8, gam, lin = _lib.probe_shade_glossy(grid, d_sh, radiance, d_maps, aov, spec, rays[:, 3:6], w, h, depth, d_mom, normal_bias,
                                                             d_pl, s["gamma"], ds.device)
            elif d_pl is not None:
                rgb8, gam, lin = _lib.probe_shade_placed(grid, d_sh, d_pl, aov, w, h, depth, d_mom, normal_bias, s["gamma"], ds.device)
            elif depth is not None:
                rgb8, gam, lin = _lib.probe_shade_vis(grid, d_sh, depth, d_mom, aov, w, h, normal_bias, s["gamma"], ds.device)
            else:
                rgb8, gam, lin = _lib.probe_shade(grid, d_sh, aov, w, h, s["gamma"], ds.device)
            if reflect is not None:
                rays, spec = self._view_spec(ds, model, w, h, dev)
                S = self._reflect(ds, reflect, reflect_rounds, grid, d_sh, aov, rays, spec, depth, d_mom, normal_bias, d_pl, direct)[0]
                v = aov[:, 3:4]
                lit = torch.where(spec[:, 3:4] > 0, v * S[:, 0:3] + (1.0 - v) * aov[:, 0:3], lin.reshape(-1, 3))
                rgb8, gam, lin = _lib.denoise(lit.contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            if direct is not None:
                term = self._direct_term(ds, direct, aov, model, rays)[0]
                rgb8, gam, lin = _lib.denoise((lin.reshape(-1, 3) + term).contiguous(), aov, None, w, h, 0, s["gamma"], ds.device)
            stats = dict(ds.aovs_stats)
        finally:
            if ds is not scene:
                ds.close()
        return RenderResult(rgb8.cpu().numpy(), gam.cpu().numpy(), lin.cpu().numpy(), stats, w, h)

    def model_aovs(self, scene, model: "CameraModel", samples: int = 8, device: int = 0) -> dict:
        """aovs() for a CameraModel (fw_render_model_aovs): the first-hit guide buffers of the model's rays, keyed as render_model keys
        its paths.  Returns (H, W, .) float32 arrays of the model's size, as aovs()."""
        from . import _lib
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            rec = ds.model_aovs(model, samples, seed=self.settings["seed"], use_bvh=self.settings["use_bvh"])
        finally:
            if ds is not scene:
                ds.close()
        h, w = int(model.height), int(model.width)
        return {k: rec[:, c].reshape((h, w, 3) if isinstance(c, slice) else (h, w)) for k, c in _lib.AOV_COLUMNS.items()}

    def render_model_denoised(self, scene, model: "CameraModel", samples: int, iterations: int = 5, aov_samples: int = 8,
                              device: int = 0) -> RenderResult:
        """render_model() filtered by fw_denoise with the model's own guide buffers (fw_render_model_aovs at `aov_samples` samples),
        without moments: the filter's luminance term is off.  Both calls share one uploaded scene.  Returns the filtered frame as a
        RenderResult whose .raw is the frame before filtering; iterations = 0 returns the raw frame bit for bit."""
        from . import _lib
        s = self.settings
        w, h = int(model.width), int(model.height)
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            res = self.render_model(ds, model, samples)
            aov = ds.model_aovs(model, aov_samples, seed=s["seed"], use_bvh=s["use_bvh"])
            dev = ds.device
        finally:
            if ds is not scene:
                ds.close()
        raw = RenderResult(res.rgb8, res.gamma, res.linear, res.stats, w, h)
        rgb8, gam, lin = _lib.denoise(raw.linear, aov, None, w, h, iterations, s["gamma"], dev)
        return RenderResult(rgb8, gam, lin, dict(raw.stats), w, h, raw=raw)

    def aovs(self, scene, samples: int = 8, device: int = 0) -> dict:
        """First-hit guide buffers (not in the reference; fw_render_aovs): for `samples` samples of every pixel the camera ray a render
        traces at segment 0, averaged.  Returns (H, W, .) float32 arrays, row 0 = image top: albedo (H, W, 3), coverage (H, W) = the
        share of samples that hit something, normal (H, W, 3), distance (H, W), position (H, W, 3).  `scene`: a Scene, a SceneDesc or an
        uploaded _lib.DeviceScene."""
        from . import _lib
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            rec = ds.aovs(self, samples)
        finally:
            if ds is not scene:
                ds.close()
        h, w = int(self.settings["height"]), int(self.settings["width"])
        return {k: rec[:, c].reshape((h, w, 3) if isinstance(c, slice) else (h, w)) for k, c in _lib.AOV_COLUMNS.items()}

    def render_denoised(self, scene, iterations: int = 5, aov_samples: int = 8, device: int = 0) -> RenderResult:
        """A render of settings["samples"] samples filtered by fw_denoise (not in the reference).  The frame comes from
        fw_render_adaptive with min_samples = samples (one round at the fixed count: bit for bit fw_render's frame, with its moments for
        the filter's luminance term), or from fw_render without moments for fewer than 2 samples; the guides from fw_render_aovs at
        `aov_samples` samples.  All three calls share one uploaded scene.  Returns the filtered frame as a RenderResult whose .raw is
        the frame before filtering."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            if int(s["samples"]) >= 2:
                res = ds.render_adaptive(self, 1.0, int(s["samples"]))
                raw = RenderResult(res.rgb8, res.gamma, res.linear, res.stats, res.width, res.height)
                moments = res.moments
            else:
                raw, moments = ds.render(self), None
            aov = ds.aovs(self, aov_samples)
            dev = ds.device
        finally:
            if ds is not scene:
                ds.close()
        rgb8, gam, lin = _lib.denoise(raw.linear, aov, moments, raw.width, raw.height, iterations, s["gamma"], dev)
        return RenderResult(rgb8, gam, lin, dict(raw.stats), raw.width, raw.height, raw=raw)

    def render_sequence(self, scene, cameras, device: int = 0, temporal: bool = True, max_history: float = DEFAULT_MAX_HISTORY,
                        iterations: int = 5, aov_samples: int = 8, updates=None):
        """The frames of a sequence, one after another on one resident scene, each using the frame before it (not in the reference;
        fw_temporal).  Frame k is rendered with cameras[k] and seed settings["seed"] + k — part of the contract: with one seed
        for every frame an unmoved camera would merge identical noise.  Per frame: fw_render_adaptive with min_samples = samples (fw_render
        for fewer than 2 samples), fw_render_aovs at `aov_samples`, fw_temporal against the previous frame's merged colour, moments and
        guides (a pixel carries over at most `max_history` samples), then fw_denoise with `iterations` on the merged colour and moments;
        everything stays on the device between the calls.  temporal=False leaves fw_temporal out: frame k then equals
        render_denoised() with cameras[k] and seed + k bit for bit.  updates[k], if given and not None, is passed to DeviceScene.update
        before frame k (a moved Scene or a SceneDesc), and the frame's prev_position comes from previous_positions().  Yields one
        RenderResult of host arrays per frame, .raw = the frame before merging and filtering; .stats["history_mean"] is the mean
        carried-over count.  `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        import copy
        import torch
        from . import _lib
        s = self.settings
        w, h, spp = int(s["width"]), int(s["height"]), int(s["samples"])
        n = w * h
        cameras = list(cameras)
        if updates is not None and len(updates) != len(cameras):
            raise ValueError("updates must have one entry (a scene or None) per camera")
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            dev = torch.device("cuda", ds.device)
            f32 = dict(dtype=torch.float32, device=dev)
            history, prev_cam = None, None
            for k, cam in enumerate(cameras):
                r = copy.copy(self); r.settings = dict(s); r.settings["seed"] = int(s["seed"]) + k; r._camera = cam
                before = None
                if updates is not None and updates[k] is not None:
                    before = ds._desc
                    ds.update(updates[k])
                out = dict(rgb8=torch.empty((n, 3), dtype=torch.uint8, device=dev), gamma=torch.empty((n, 3), **f32),
                           linear=torch.empty((n, 3), **f32))
                if spp >= 2:
                    out["moments"] = torch.empty((n, 4), **f32)
                    stats = ds.render_adaptive(r, 1.0, spp, out=out).stats
                else:
                    stats = ds.render(r, None, (out["rgb8"].data_ptr(), out["gamma"].data_ptr(), out["linear"].data_ptr()),
                                      torch.cuda.current_stream(dev).cuda_stream)
                color, moments = out["linear"], out.get("moments")
                aov = ds.aovs(r, aov_samples, out=torch.empty((n, 12), **f32))
                stats = dict(stats)
                if temporal:
                    prev_pos = None
                    if before is not None and history is not None:
                        rays = torch.from_numpy(ds.camera_rays(r, 0)).to(dev)
                        objects = _lib.hit_fields(ds.trace(rays, s["use_bvh"], seed=r.settings["seed"]))["object"]
                        prev_pos = previous_positions(aov[:, 8:11].contiguous(), objects, before, ds._desc).contiguous()
                    color, moments, n_h = _lib.temporal(color, aov, moments, history, prev_pos, w, h, cam, prev_cam, spp, max_history, ds.device)
                    history, prev_cam = (color, moments, aov), cam
                    stats["history_mean"] = float(n_h.mean().item())
                rgb8, gam, lin = _lib.denoise(color, aov, moments, w, h, iterations, s["gamma"], ds.device)
                raw = RenderResult(out["rgb8"].cpu().numpy(), out["gamma"].cpu().numpy(), out["linear"].cpu().numpy(), stats, w, h)
                yield RenderResult(rgb8.cpu().numpy(), gam.cpu().numpy(), lin.cpu().numpy(), dict(stats), w, h, raw=raw)
        finally:
            if ds is not scene:
                ds.close()

    def render(self, scene, device: int = 0) -> np.ndarray:
        """`pub fn render(&self, scene: Scene) -> Vec<Color>` (render.rs:109): (W*H, 3) uint8, row 0 = top."""
        return self.render_full(scene, None, device).rgb8

    def gbuffer(self, scene, sample: int = 0, device: int = 0) -> dict:
        """Depth / normal / ID buffers of the first hit of every pixel (not in the reference): the camera rays a render traces for
        `sample` (fw_camera_rays), traced with this renderer's use_bvh and seed (fw_trace_rays).  Returns (H, W) arrays, row 0 =
        image top: t, point (H, W, 3), normal (H, W, 3), u, v, material, object (FW_NO_HIT where the ray missed), prim.
        `scene`: a Scene, a SceneDesc or an uploaded _lib.DeviceScene."""
        from . import _lib
        s = self.settings
        ds = scene if isinstance(scene, _lib.DeviceScene) else _lib.DeviceScene(scene if isinstance(scene, SceneDesc) else scene.to_desc(), device)
        try:
            hits = ds.trace(ds.camera_rays(self, sample), s["use_bvh"], seed=s["seed"])
        finally:
            if ds is not scene:
                ds.close()
        h, w = int(s["height"]), int(s["width"])
        return {name: hits[name].reshape((h, w) + hits.dtype[name].shape) for name in hits.dtype.names}


def save_image(render: np.ndarray, path, width: int, height: int):
    """src/window.rs:59-66"""
    from PIL import Image
    Image.fromarray(np.asarray(render, dtype=np.uint8).reshape(height, width, 3), "RGB").save(path)
