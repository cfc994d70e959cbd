"""Every walk and shade kernel the launchers of fw_kernels.hip can pick is launched and checked here, one row per instantiation
(DESIGN.md §9r).  A row is a small scene, use_bvh, flags and options (set with _lib.options); it asserts

  (a) that the kernel it is meant for ran: _lib.last_kernels() after the call holds the row's name(s) — a threshold that moves sends the
      row to a neighbouring kernel, and the row then fails with the set that did run;
  (b) that the result is right, at zero tolerance.  A table mode, LDS residency, a wave count, a node encoding or the chain state change
      where operands are loaded from or how rays are scheduled, never an arithmetic operation, so equality holds by construction:
      walk rows    ds.trace over camera, secondary and adversarial rays (test_gpu_trace's generators and compare) against oracle.trace bit
                   for bit, and a frame's rgb8 and rays_per_depth against the oracle's;
      k_shade      the frame's rgb8 and rays_per_depth against the oracle's, and the pre-gamma means bit for bit where the chain applies;
      light sampling and GgxMat   the oracle has neither, so linear, gamma and rgb8 are compared as bits with the same scene's frame under
                   the variant whose values other modules check (known answers, test_no_bias, the nee_receivers probes, test_gpu_ggx): table
                   mode 1 where the scene fits it, otherwise NO_LDS_TABLES=1 (mode 0); mode 0 itself is tied to mode 1 on the unpadded scene.

Table modes: 1 is a small scene's default, 0 is NO_LDS_TABLES=1 (and C1, by size: more than 512 materials plus textures), 2 needs more than
16 384 B of object records (96 B each) with materials and textures under the limit: the row's scene plus PAD spheres of radius 1e-3 behind
the camera that share one material.  Padding changes the scene, so a padded frame is compared with the padded scene's own mode-0 frame.

Waves per workgroup of the LDS-resident wide walks (16, 12 or 8) follow from the tree's size; walk_fit restates the launcher's formula and
the rows pick a patch (coord_scenes._patch) or a sphere count on the host from fw_selftest_wide_bvh's node count; assertion (a) says whether
the size landed.  The census at the end compares the union of what the rows launched with the library's whole table of names."""
import copy
import os
import re
import sys

import numpy as np
import pytest

from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, CheckerTexture, Cone, ConstantTexture, DielectricMat, Disk, EmissiveMat, GgxMat, HdrEnvironment,
                              LambertianMat, PointLight, RenderObject, Renderer, Rotor3, Scene, SkyEnv, Sphere, TriangleMesh,
                              TurbulenceTexture, XZRect)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coord_scenes as CS  # noqa: E402
from test_gpu_trace import adversarial_set, camera_set, compare, secondary_set  # noqa: E402
from test_wide_bvh_cpu import tri_boxes  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP = 48, 32, 8
PAD = 171                                   # 171 x 96 B = 16 416 B of object records: over LDS_TABLE_LIMIT by themselves
LDS_TREE_LIMIT = 160 * 1024
COVER = {}                                  # kernel name (without @waves) -> the first row that names it, saw it run and checked the result
RAN = set()                                 # the rows that ran


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flags(r, *names):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    for n in names:
        getattr(rr, n)(True)
    return rr


def _ran(row, want, got=None):
    """assertion (a): the kernels the row names are among those the call launched; they are the ones the row covers in the census"""
    got = _lib.last_kernels() if got is None else got
    missing = sorted(set(want) - got)
    assert not missing, f"{row}: {missing} did not run; the call launched {sorted(got)}"
    return [k.split("@")[0] for k in want]


def _same_bits(a, b, what):
    assert np.array_equal(a.rgb8, b.rgb8), what
    assert np.array_equal(_u32(a.gamma), _u32(b.gamma)) and np.array_equal(_u32(a.linear), _u32(b.linear)), what


def _same_as_oracle(gpu, cpu, what, means=False):
    assert [int(x) for x in gpu.stats["rays_per_depth"]] == [int(x) for x in cpu.stats["rays_per_depth"]], what
    assert np.array_equal(gpu.rgb8, cpu.rgb8), (what, int((gpu.rgb8 != cpu.rgb8).sum()))
    if means:
        assert np.array_equal(gpu.linear, cpu.linear.astype(np.float32)), what


# ---- the shade rows' scene ----------------------------------------------------------------------------------------------------------------
def room(floor="const", glass=False, ggx=False, disk=False, hdr=False, point=False, pad=0):
    """A floor (the receiver: constant, checker or turbulence), a diffuse sphere, a rectangle light, optionally a glass sphere, a GgxMat
    sphere, a disk light, an HDR map, a point light, and `pad` tiny spheres of one material behind the camera."""
    sc = Scene.new()
    tex = {"const": ConstantTexture.new((0.6, 0.6, 0.6)), "checker": CheckerTexture.with_colors((0.2, 0.4, 0.1), (0.9, 0.9, 0.9), 3.0),
           "turbulence": TurbulenceTexture.new(3, 2.0)}[floor]
    m_floor = sc.add_material(LambertianMat.new(tex))
    m_ball = sc.add_material(LambertianMat.with_color((0.7, 0.3, 0.2)))
    m_light = sc.add_material(EmissiveMat.with_color((6.0, 6.0, 6.0)))
    sc.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 20.0, 0.0, m_floor)))
    sc.add_object(RenderObject.new(Sphere.new(1.0, m_ball)).position(-1.5, 1.0, 0.5))
    sc.add_object(RenderObject.new(XZRect.new(-1.5, 1.5, -1.0, 1.0, 4.0, m_light)).flip_normals())
    if glass:
        sc.add_object(RenderObject.new(Sphere.new(0.7, sc.add_material(DielectricMat.new(1.5)))).position(0.3, 0.7, -1.5))
    if ggx:
        sc.add_object(RenderObject.new(Sphere.new(0.9, sc.add_material(GgxMat.new((0.9, 0.7, 0.4), 0.3)))).position(1.6, 0.9, 0.8))
    if disk:
        sc.add_object(RenderObject.new(Disk.new(0.8, m_light)).position(2.5, 2.5, 2.0).rotate(Rotor3.from_euler_angles(0.6, 0.2, -0.3)))
    if hdr:
        sc.set_environment(HdrEnvironment(scenes.synthetic_hdr(64, 32)))
    else:
        sc.set_environment(SkyEnv.default())
    if point:
        sc.add_light(PointLight((1.0, 3.0, -2.0), (8.0, 7.0, 6.0)))
    if pad:
        m_pad = sc.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
        for k in range(pad):
            sc.add_object(RenderObject.new(Sphere.new(1e-3, m_pad)).position(-4.0 + 0.5 * (k % 17), 0.5 + 0.5 * (k // 17), -30.0))
    cam = CameraSettings.default().cam_pos((0.0, 2.5, -9.0)).look_at((0.0, 1.0, 0.0)).field_of_view(40.0)
    return sc, Renderer.default().width(W).height(H).samples(SPP).use_bvh(False).camera(cam).seed(5)


# class -> (room arguments, renderer flags, options, the shadow-resolve kernel, reference).  Every class of shading mode 0 outside the chain
# has a checker or turbulence receiver, so its frame reads the texture table (texp) as well as the material table the constants come from.
# reference: "oracle" (means: the pre-gamma means too, where the chain applies) or "modes" (the value-checked table mode, bit for bit)
LS, EM, ENV = "light_sampling", "all_emitters", "env_sampling"
SHADE = {
    "k_shade<L,1,chain>": (dict(), (), {}, None, "oracle+means"),
    "k_shade<L,1,no chain>": (dict(), (), dict(NO_CHAIN="1"), None, "oracle"),
    "k_shade<L,0,chain>": (dict(glass=True), (), {}, None, "oracle+means"),
    "k_shade<L,0,no chain>": (dict(floor="checker"), (), {}, None, "oracle"),
    "k_shade_ls<L,1>": (dict(), (LS,), {}, "k_shadow_resolve", "modes"),
    "k_shade_ls<L,0>": (dict(floor="turbulence"), (LS,), {}, "k_shadow_resolve", "modes"),            # Perlin staging beside the tables
    "k_shade_pl<L,1>": (dict(disk=True), (LS, EM), {}, "k_shadow_resolve_pl", "modes"),
    "k_shade_pl<L,0>": (dict(disk=True, floor="checker"), (LS, EM), {}, "k_shadow_resolve_pl", "modes"),
    "k_shade_env<L>": (dict(hdr=True, floor="checker"), (ENV,), {}, "k_shadow_resolve_env", "modes"),
    "k_shade_pl_env<L>": (dict(hdr=True, disk=True, floor="checker"), (LS, EM, ENV), {}, "k_shadow_resolve_pl", "modes"),
    "k_shade_dl<L,1>": (dict(point=True), (), {}, "k_shadow_resolve_dl", "modes"),
    "k_shade_dl<L,0>": (dict(point=True, floor="turbulence"), (), {}, "k_shadow_resolve_dl", "modes"),  # Perlin staging beside the tables
    # GgxMat: the oracle has no such material, so k_shade_gx is tied to its table mode 1 as the light-sampling kernels are
    "k_shade_gx<L,1>": (dict(ggx=True), (), {}, None, "modes"),
    "k_shade_gx<L,0>": (dict(ggx=True, glass=True, floor="checker"), (), {}, None, "modes"),
    "k_shade_gx_nee<L,0,pl_env>": (dict(ggx=True, hdr=True, disk=True, floor="checker"), (LS, EM, ENV), {}, "k_shadow_resolve_pl", "modes"),
    "k_shade_gx_nee<L,0,env>": (dict(ggx=True, hdr=True, floor="checker"), (ENV,), {}, "k_shadow_resolve_env", "modes"),
    "k_shade_gx_nee<L,0,pl>": (dict(ggx=True, disk=True, glass=True, floor="checker"), (LS, EM), {}, "k_shadow_resolve_pl", "modes"),
    "k_shade_gx_nee<L,1,pl>": (dict(ggx=True, disk=True), (LS, EM), {}, "k_shadow_resolve_pl", "modes"),
    "k_shade_gx_nee<L,0,ls>": (dict(ggx=True, glass=True, floor="turbulence"), (LS,), {}, "k_shadow_resolve_gx", "modes"),
    "k_shade_gx_nee<L,1,ls>": (dict(ggx=True), (LS,), {}, "k_shadow_resolve_gx", "modes"),
    "k_shade_gx_nee<L,0,dl>": (dict(ggx=True, point=True, glass=True, floor="checker"), (), {}, "k_shadow_resolve_gx", "modes"),
    "k_shade_gx_nee<L,1,dl>": (dict(ggx=True, point=True), (), {}, "k_shadow_resolve_gx", "modes"),
}
_frames = {}          # (class, padded, NO_LDS_TABLES) -> (frame, the kernels its call launched): rendered once, shared by the class's rows
_oracle_frames = {}   # (class, padded) -> the oracle's frame


def _shade_frame(cls, padded, no_tables):
    key = (cls, padded, no_tables)
    if key not in _frames:
        args, flags, opts, _, _ = SHADE[cls]
        sc, r = room(pad=PAD if padded else 0, **args)
        opts = dict(opts, **(dict(NO_LDS_TABLES="1") if no_tables else {}))
        with _lib.options(**opts):
            ds = _lib.DeviceScene(sc.to_desc())
            try:
                _frames[key] = (ds.render(_flags(r, *flags)), _lib.last_kernels())
            finally:
                ds.close()
    return _frames[key]


def _shade_oracle(oracle, cls, padded):
    if (cls, padded) not in _oracle_frames:
        sc, r = room(pad=PAD if padded else 0, **SHADE[cls][0])
        _oracle_frames[(cls, padded)] = oracle.render(sc, r)
    return _oracle_frames[(cls, padded)]


@pytest.mark.parametrize("L", [1, 0, 2])
@pytest.mark.parametrize("cls", list(SHADE))
def test_shade_row(oracle, cls, L):
    row = f"test_shade_row[{cls}-{L}]"
    RAN.add(row)
    name = cls.replace("<L", f"<{L}")
    resolve, ref = SHADE[cls][3], SHADE[cls][4]
    padded, no_tables = L == 2, L == 0
    frame, ran = _shade_frame(cls, padded, no_tables)
    covered = _ran(row, {name, *([resolve] if resolve else [])}, ran)
    if ref.startswith("oracle"):
        _same_as_oracle(frame, _shade_oracle(oracle, cls, padded), row, means=ref.endswith("means"))
    else:
        # table mode 1 and mode 0 on the scene that fits both; mode 2 against the padded scene's mode 0
        other, other_ran = _shade_frame(cls, padded, not no_tables) if L != 2 else _shade_frame(cls, True, True)
        other_name = cls.replace("<L", "<0" if L != 0 else "<1")
        assert other_name in other_ran, f"{row}: the reference frame ran {sorted(other_ran)}"
        _same_bits(frame, other, row)
    for k in covered:
        COVER.setdefault(k, row)


def test_shade_table_mode_0_by_size(oracle):
    """C1 has more than 512 materials plus textures: no table mode fits, without any switch"""
    row = "test_shade_table_mode_0_by_size"
    RAN.add(row)
    sc, r = scenes.config("C1_random_spheres", W, H, SPP)
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        gpu = ds.render(r)
        covered = _ran(row, {"k_shade<0,0,no chain>"})
    finally:
        ds.close()
    _same_as_oracle(gpu, oracle.render(sc, r), row)
    for k in covered:
        COVER.setdefault(k, row)


# ---- the walk rows ------------------------------------------------------------------------------------------------------------------------
def _lit(sc):
    white = sc.add_material(LambertianMat.with_color((0.6, 0.6, 0.6)))
    light = sc.add_material(EmissiveMat.with_color((5.0, 5.0, 5.0)))
    sc.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 20.0, -1.5, white)))
    sc.add_object(RenderObject.new(XZRect.new(-1.0, 1.0, -1.0, 1.0, 3.0, light)).flip_normals())
    sc.set_environment(SkyEnv.default())
    return white


def _extras(sc, white, medium, cone, spheres):
    if medium:
        sc.add_volume(RenderObject.new(Sphere.new(0.5, white)).position(1.2, 0.0, -0.8), 0.8, ConstantTexture.new((0.3, 0.5, 0.8)))
    if cone:
        sc.add_object(RenderObject.new(Cone.new(0.5, 1.0, white)).position(-1.3, -1.5, -0.6))
    rng = np.random.default_rng(9)
    mats = [sc.add_material(LambertianMat.with_color(tuple(rng.uniform(0.2, 0.9, 3)))) for _ in range(3)]
    for k in range(spheres):
        p = rng.uniform((-2.0, -1.2, -1.5), (2.0, 1.5, 1.5))
        sc.add_object(RenderObject.new(Sphere.new(float(rng.uniform(0.1, 0.3)), mats[k % 3])).position(*p))


def _renderer(use_bvh, back=4.5):
    cam = CameraSettings.default().cam_pos((0.4, 0.6, -back)).look_at((0.0, 0.0, 0.0)).field_of_view(45.0)
    return Renderer.default().width(W).height(H).samples(SPP).use_bvh(use_bvh).camera(cam).seed(3)


def mesh_scene(n=12, h=0.2, medium=False, cone=False, spheres=0, use_bvh=True):
    """The bumpy n x n patch of coord_scenes over a floor under a light, optionally beside a medium, a cone and small spheres"""
    verts, idx = CS._patch(h, 7, n)
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.7, 0.5, 0.3)))
    sc.add_object(RenderObject.new(TriangleMesh.new(verts.astype(np.float32), idx, None, None, m)))
    white = _lit(sc)
    _extras(sc, white, medium, cone, spheres)
    return sc, _renderer(use_bvh)


def cloud_scene(spheres=12, medium=False, cone=False, use_bvh=True):
    """Small spheres over a floor under a light, optionally with a medium and a cone: no mesh"""
    sc = Scene.new()
    white = _lit(sc)
    _extras(sc, white, medium, cone, spheres)
    return sc, _renderer(use_bvh)


def _cloud_centres(n):
    return np.random.default_rng(3).uniform((-2.5, -1.3, -1.5), (2.5, 2.0, 2.5), (n, 3))


def big_cloud(n):
    """n spheres of radius 0.04 in a box: a TLAS of about n / 2.3 wide nodes"""
    sc = Scene.new()
    _lit(sc)
    rng = np.random.default_rng(4)
    mats = [sc.add_material(LambertianMat.with_color(tuple(rng.uniform(0.2, 0.9, 3)))) for _ in range(4)]
    c = _cloud_centres(n)
    for k in range(n):
        sc.add_object(RenderObject.new(Sphere.new(0.04, mats[k % 4])).position(*c[k]))
    return sc, _renderer(True, back=6.0)


def cornell(cone=False, use_bvh=False):
    """cornell_box; with `cone`, a cone ahead of the two trailing boxes: no longer the SIMPLE set, the boxes still deferred"""
    sc, r = scenes.cornell_box()
    if cone:
        boxes = sc.render_objects[-2:]
        del sc.render_objects[-2:]
        sc.add_object(RenderObject.new(Cone.new(60.0, 120.0, 1)).position(420.0, 0.0, 120.0))
        sc.render_objects += boxes
    return sc, r.width(W).height(H).samples(SPP).use_bvh(use_bvh).seed(3)


# The launcher's rule for an LDS-resident wide walk (fw_kernels.hip: lds_walk_bytes), restated: the tree — 112 B per wide f32 node, 48 B per
# wide q8 node, 48 B per triangle where the triangles come along — plus waves x levels x 128 B of 16-bit stacks, levels = 3 x depth + 2,
# plus a counter and the workgroup's queue counts (under 256 B at these frame sizes), against 160 KiB: the first of 16, 12, 8 waves that
# fits.  The triangles come along only if they fit beside 16 waves.  A scene keeps f32 nodes only if they fit beside 8 waves with 4 096 B to
# spare (fw_runtime.cpp: wide_lds_bytes), else q8 nodes on the same condition, else none.
NODE_BYTES = {1: 112, 2: 48}


def walk_fit(nodes, depth, fmt, n_tris=0):
    """(waves, tris in LDS, margin in bytes to the nearest threshold) or None where the tree is not kept"""
    tree, stack = nodes * NODE_BYTES[fmt], (3 * depth + 2) * 128
    if tree + 8 * stack + 4096 > LDS_TREE_LIMIT:
        return None
    if n_tris and tree + n_tris * 48 + 16 * stack + 256 <= LDS_TREE_LIMIT:
        return 16, True, LDS_TREE_LIMIT - (tree + n_tris * 48 + 16 * stack + 256)
    room_left = {w: LDS_TREE_LIMIT - (tree + w * stack + 256) for w in (16, 12, 8)}
    for w, bigger in ((16, None), (12, 16), (8, 12)):
        if room_left[w] >= 0:
            m = min(room_left[w], LDS_TREE_LIMIT - 4096 - tree - 8 * stack)
            return w, False, m if bigger is None else min(m, -room_left[bigger])
    return None


def sized_patch(fmt, waves):
    """the grid size whose BLAS lands on `waves` waves per workgroup with the widest margin (f32 nodes: the scene's own choice up to about
    3 000 triangles; q8 nodes: its choice beyond)"""
    best = None
    for n in range(30, 66):
        verts, idx = CS._patch(0.05, 7, n)
        boxes = tri_boxes(verts.astype(np.float32), idx.astype(np.int64))
        f32 = _lib.selftest_wide_bvh(boxes, 1)[1]
        if (walk_fit(f32["nodes"], f32["depth"], 1, len(boxes)) is not None) != (fmt == 1):
            continue
        st = f32 if fmt == 1 else _lib.selftest_wide_bvh(boxes, 2)[1]
        fit = walk_fit(st["nodes"], st["depth"], fmt, len(boxes))
        if fit and fit[0] == waves and not fit[1] and (best is None or fit[2] > best[1]):
            best = (n, fit[2])
    assert best, (fmt, waves)
    return best[0]


def sized_cloud(waves):
    """the sphere count whose TLAS (f32 wide nodes over the spheres and the light; the floor is hoisted out of the tree) lands on `waves`
    waves per workgroup"""
    best = None
    for n in range(1800, 2800, 50):
        c = _cloud_centres(n).astype(np.float32)
        b = np.concatenate([c - np.float32(0.04), c + np.float32(0.04)], axis=1)
        b = np.concatenate([b, np.array([[-1.0, 2.999, -1.0, 1.0, 3.001, 1.0]], np.float32)]).astype(np.float32)
        st = _lib.selftest_wide_bvh(b, 1)[1]
        fit = walk_fit(st["nodes"], st["depth"], 1)
        if fit and fit[0] == waves and (best is None or fit[2] > best[1]):
            best = (n, fit[2])
    assert best, waves
    return best[0]


# row -> (scene builder, options, the kernels that must run)
WALK = {
    "k_extend_scan<false>": (lambda o: cornell(use_bvh=True), {}, ["k_extend_scan<false>"]),
    "k_extend_scan<true>": (lambda o: mesh_scene(medium=True), {}, ["k_extend_scan<true>"]),
    "k_extend_scan<true,true>": (lambda o: mesh_scene(cone=True), {}, ["k_extend_scan<true,true>"]),
    "k_extend_scan<true,true,true>": (lambda o: mesh_scene(), {}, ["k_extend_scan<true,true,true>", "k_blas_wide<f32,tris>@16"]),
    "k_extend_tlas_park": (lambda o: mesh_scene(spheres=8), {}, ["k_extend_tlas_park"]),
    "k_extend_tlas": (lambda o: cloud_scene(), dict(NO_LDS_TREES="1"), ["k_extend_tlas"]),
    "k_extend_tlas_lds": (lambda o: cloud_scene(), dict(WIDE="0"), ["k_extend_tlas_lds@16"]),
    "k_extend_tlas_wide<false,true>": (lambda o: cloud_scene(), {}, ["k_extend_tlas_wide<false,true>@16"]),
    "k_extend_tlas_wide<true,true>": (lambda o: cloud_scene(medium=True), {}, ["k_extend_tlas_wide<true,true>@16"]),
    "k_extend_tlas_wide<true>": (lambda o: cloud_scene(medium=True, cone=True), {}, ["k_extend_tlas_wide<true>@16"]),
    "k_extend_tlas_wide<false>": (lambda o: cloud_scene(cone=True), {}, ["k_extend_tlas_wide<false>@16"]),
    "k_extend_tlas_wide@12": (lambda o: big_cloud(sized_cloud(12)), {}, ["k_extend_tlas_wide<false,true>@12"]),
    "k_extend_tlas_wide@8": (lambda o: big_cloud(sized_cloud(8)), {}, ["k_extend_tlas_wide<false,true>@8"]),
    "k_blas_wide<f32,no tris>": (lambda o: mesh_scene(), dict(NO_LDS_TRIS="1"), ["k_blas_wide<f32,no tris>@16"]),
    "k_blas_wide<q8,tris>": (lambda o: mesh_scene(), dict(WIDE="q8"), ["k_blas_wide<q8,tris>@16"]),
    "k_blas_wide<q8,no tris>": (lambda o: mesh_scene(), dict(WIDE="q8", NO_LDS_TRIS="1"), ["k_blas_wide<q8,no tris>@16"]),
    "k_blas_wide<f32,no tris>@12": (lambda o: mesh_scene(sized_patch(1, 12), 0.05), {}, ["k_blas_wide<f32,no tris>@12"]),
    "k_blas_wide<f32,no tris>@8": (lambda o: mesh_scene(sized_patch(1, 8), 0.05), {}, ["k_blas_wide<f32,no tris>@8"]),
    "k_blas_wide<q8,no tris>@12": (lambda o: mesh_scene(sized_patch(2, 12), 0.05), {}, ["k_blas_wide<q8,no tris>@12"]),
    "k_blas_wide<q8,no tris>@8": (lambda o: mesh_scene(sized_patch(2, 8), 0.05), {}, ["k_blas_wide<q8,no tris>@8"]),
    "k_blas_lds<true>": (lambda o: mesh_scene(), dict(WIDE="0"), ["k_blas_lds<true>@16"]),
    "k_blas_lds<false>": (lambda o: mesh_scene(), dict(WIDE="0", NO_LDS_TRIS="1"), ["k_blas_lds<false>@16"]),
    "k_blas": (lambda o: mesh_scene(), dict(NO_LDS_TREES="1"), ["k_blas"]),
    "k_extend_linear": (lambda o: mesh_scene(use_bvh=False), {}, ["k_extend_linear"]),
    "k_extend_linear_nomesh": (lambda o: cloud_scene(6, medium=True, cone=True, use_bvh=False), {}, ["k_extend_linear_nomesh"]),
    "k_extend_linear_plain": (lambda o: cloud_scene(6, cone=True, use_bvh=False), {}, ["k_extend_linear_plain"]),
    "k_extend_linear_simple<false>": (lambda o: cloud_scene(6, use_bvh=False), {}, ["k_extend_linear_simple<false>"]),
    "k_extend_linear_simple<true>": (lambda o: cloud_scene(6, medium=True, use_bvh=False), {}, ["k_extend_linear_simple<true>"]),
    "k_extend_linear_defer<true>": (lambda o: cornell(), {}, ["k_extend_linear_defer<true>"]),
    "k_extend_linear_defer<false>": (lambda o: cornell(cone=True), {}, ["k_extend_linear_defer<false>"]),
    "k_extend_exact[lane]": (lambda o: mesh_scene(spheres=8), dict(EXACT_ALL="1", EXACT_FORM="lane"), ["k_extend_exact"]),
    "k_extend_exact[wave]": (lambda o: mesh_scene(spheres=8), dict(EXACT_ALL="1", EXACT_FORM="wave"), ["k_extend_exact"]),
}


@pytest.mark.parametrize("name", list(WALK))
def test_walk_row(oracle, name):
    row = f"test_walk_row[{name}]"
    RAN.add(row)
    build, opts, want = WALK[name]
    sc, r = build(oracle)
    m = int(r.settings["use_bvh"])
    with _lib.options(**opts):
        ds = _lib.DeviceScene(sc.to_desc())
        try:
            gpu = ds.render(r)
            covered = _ran(row + " render", want)
            cam = camera_set(ds, r, 1024)
            big = len(sc.render_objects) > 100 or any(isinstance(o.obj, TriangleMesh) and len(o.obj.indicies) > 3000 for o in sc.render_objects)
            sec = secondary_set(oracle, sc, r, 24 if big else 200)[:2048]      # (the oracle rebuilds the scene for every path)
            adv = adversarial_set(oracle, sc, ds, m, cam, 400)[:2048]
            for label, rays in (("camera", cam), ("secondary", sec), ("adversarial", adv)):
                hits = ds.trace(rays, m)
                _ran(f"{row} trace {label}", want)
                compare(hits, oracle.trace(sc, rays, m), f"{row} {label}")
        finally:
            ds.close()
    _same_as_oracle(gpu, oracle.render(sc, r), row)
    for k in covered:
        COVER.setdefault(k, row)


def test_replayed_graph_reports_the_captured_set():
    """A frame asked for three times under GRAPH=1 runs its launchers twice (the second time into a capture) and is replayed the third time:
    all three report the same kernels"""
    RAN.add("test_replayed_graph_reports_the_captured_set")
    sc, r = cornell()
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        with _lib.options(GRAPH="1"):
            sets, frames = [], []
            for _ in range(3):
                frames.append(ds.render(r))
                sets.append(_lib.last_kernels())
        assert frames[2].stats["reserved"] & 0x80000000, "the third frame was not a replay"
        assert sets[0] == sets[1] == sets[2] and {"k_extend_linear_defer<true>", "k_shade<1,1,chain>"} <= sets[0], sets
        hits = ds.trace(np.array([[278.0, 278.0, -800.0, 0.0, 0.0, 1.0]], np.float32), 0)       # a trace clears the set: no shade kernel
        after = _lib.last_kernels()
        assert hits.shape[0] == 1 and "k_extend_linear_defer<true>" in after and not any(k.startswith("k_shade") for k in after), after
    finally:
        ds.close()


# ---- the census ---------------------------------------------------------------------------------------------------------------------------
# walk kernels that no row here launches, each with its reason (at most four; shade and shadow-resolve kernels may not stand here)
ALLOW = {}


def test_census():
    """Every kernel name of the build (fw_debug_kernels with device -1) is named by a row above that saw it run and passed its checks, or
    stands in ALLOW.  Runs after the rows: the whole module has to run.  FW_CENSUS_OUT=<file> writes the table of names and covering rows (profiles/kernel_census.txt)."""
    n_rows = 3 * len(SHADE) + len(WALK) + 2
    assert len(RAN) == n_rows, f"the census needs every row of this module: {len(RAN)} of {n_rows} ran"
    table = sorted(_lib.last_kernels(-1))
    if _lib.has_ab():
        table = [k for k in table if not re.match(r"k_extend_bvh$|k_bounce<|k_shade<\d,2,", k)]      # the A/B build's own: its tests launch them
    assert len(ALLOW) <= 4
    walk = re.compile(r"k_extend_|k_blas")
    assert all(walk.match(k) and k in table for k in ALLOW), ALLOW
    missing = [k for k in table if k not in COVER and k not in ALLOW]
    assert not missing, f"no passing row names {missing}"
    stale = [k for k in ALLOW if k in COVER]
    assert not stale, f"{stale} is covered by a row: take it out of ALLOW"
    out = os.environ.get("FW_CENSUS_OUT")
    if out:
        with open(out, "w") as f:
            f.write("# kernel name (fw_debug_kernels, device -1)  ->  the first row of tests/test_gpu_kernel_variants.py that names it, saw it run and checked the result\n")
            for k in table:
                f.write(f"{k:36s} {COVER.get(k) or 'not launched: ' + ALLOW[k]}\n")
