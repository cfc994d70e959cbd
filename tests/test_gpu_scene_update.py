"""Moving the objects of a resident scene on the GPU (fw_scene_update), at zero tolerance: after an update every call equals the same call on
fw_scene_create of the moved scene, bit for bit (u8, the gamma and linear floats compared as uint32, the ray counters, hit records).
C1-C5, teapot and conics under a seeded animator that moves, rotates and flips objects (a rotated mesh and the gated Disk among them),
both walks; round trips and eight updates in a row; progressive, adaptive, views and traces after an update; kernel-selecting options
and both tree builders; the frame graph; the CPU oracle; a mesh whose reach grows and shrinks; hoisting that changes; every rejected
update (the scene then renders as before); and the size of an update's upload."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, LambertianMat, Renderer, RenderObject, Rotor3, Rect3d, Scene, SkyEnv, Sphere, TriangleMesh,
                              XZRect, Disk, ConstantMedium, orbit_cameras)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [("C1_random_spheres", 64, 40, 8), ("C2_cornell_box", 48, 48, 16), ("C3_suzanne", 64, 36, 8), ("C4a_hdri_test", 48, 48, 8),
          ("C4b_volume_test", 48, 48, 8), ("C5_part2_all", 64, 36, 4), ("teapot", 64, 40, 8), ("conics", 64, 40, 8)]
UPDATE_RE = re.compile(r"scene_update: (\d+) objects, TLAS build ([\d.]+) ms host, ([\d.]+) ms device, (\d+) meshes rebuilt, (\d+) B uploaded, (\d+) hoisted")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _walk(r, bvh):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    return rr.use_bvh(bvh)


def _inner(shape):
    return shape.obj if isinstance(shape, ConstantMedium) else shape


def animate(scene, rng):
    """Moves, rotates and flips a seeded choice of objects by up to 5 % of the scene's span; every mesh and every Disk is moved and
    rotated."""
    span = max(1.0, max(float(np.max(np.abs(ro._position))) for ro in scene.render_objects))
    for ro in scene.render_objects:
        special = isinstance(_inner(ro.obj), (TriangleMesh, Disk))
        k = int(rng.integers(0, 4))
        if special or k == 0:
            ro.position_vec(ro._position + rng.uniform(-0.05, 0.05, 3).astype(np.float32) * span)
        if special or k == 1:
            ro.rotate(Rotor3.from_euler_angles(*[float(x) for x in rng.uniform(-0.6, 0.6, 3)]))
        if k == 2:
            ro.flip_normals()


def assert_same(a, b):
    assert np.array_equal(a.rgb8, b.rgb8), int((a.rgb8 != b.rgb8).sum())
    assert np.array_equal(_u32(a.gamma), _u32(b.gamma))
    assert np.array_equal(_u32(a.linear), _u32(b.linear))
    for k in ("samples", "rays", "deposits"):
        assert a.stats[k] == b.stats[k], k
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in b.stats["rays_per_depth"]]


def fresh_renders(scene, renderers):
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        return [ds.render(r) for r in renderers]
    finally:
        ds.close()


def update_lines(text):
    return [tuple(float(x) if "." in x else int(x) for x in m.groups()) for m in UPDATE_RE.finditer(text)]


@pytest.mark.parametrize("name,w,h,spp", SCENES)
def test_update_equals_a_fresh_create(name, w, h, spp):
    s, r = scenes.config(name, w, h, spp)
    walks = [_walk(r, True), _walk(r, False)]
    ds = _lib.DeviceScene(s.to_desc())
    try:
        ds.render(walks[0])
        animate(s, np.random.default_rng(sum(map(ord, name))))
        ds.update(s)
        for got, want in zip([ds.render(rr) for rr in walks], fresh_renders(s, walks)):
            assert_same(got, want)
    finally:
        ds.close()


def test_round_trip_and_eight_updates():
    s, r = scenes.config("conics", 48, 32, 8)
    ds = _lib.DeviceScene(s.to_desc())
    try:
        first = ds.render(r)
        saved = [(ro._position.copy(), ro.rotation, ro._flip_normals) for ro in s.render_objects]
        animate(s, np.random.default_rng(1))
        ds.update(s)
        assert_same(ds.render(r), fresh_renders(s, [r])[0])
        for ro, (p, rot, fl) in zip(s.render_objects, saved):             # back to A
            ro.position_vec(p)
            ro.rotate(rot)
            ro._flip_normals = fl
        ds.update(s)
        assert_same(ds.render(r), first)
        rng = np.random.default_rng(2)
        for _ in range(8):
            animate(s, rng)
            ds.update(s)
            assert_same(ds.render(r), fresh_renders(s, [r])[0])
    finally:
        ds.close()


def test_every_call_after_an_update():
    """fw_render_progressive (2 passes), fw_render_adaptive, fw_render_views (2 cameras), fw_trace_rays (camera and random rays)"""
    for name, w, h, spp in (("C3_suzanne", 40, 32, 8), ("C1_random_spheres", 40, 32, 8)):
        s, r = scenes.config(name, w, h, spp)
        ds = _lib.DeviceScene(s.to_desc())
        try:
            animate(s, np.random.default_rng(7))
            ds.update(s)
            ref = _lib.DeviceScene(s.to_desc())
            try:
                n = w * h
                accs = []
                for d in (ds, ref):
                    acc = np.zeros((n, 4), np.float32)
                    d.render_progressive(r, 0, acc)
                    res = d.render_progressive(r, spp, acc)
                    accs.append((acc, res))
                assert np.array_equal(_u32(accs[0][0]), _u32(accs[1][0]))
                assert_same(accs[0][1], accs[1][1])
                ad = [d.render_adaptive(r, 0.05, min_samples=2) for d in (ds, ref)]
                for f in ("rgb8", "gamma", "linear", "accum", "moments", "round_pixels"):
                    assert np.array_equal(np.ascontiguousarray(getattr(ad[0], f)).view(np.uint8), np.ascontiguousarray(getattr(ad[1], f)).view(np.uint8)), f
                assert ad[0].stats["rays"] == ad[1].stats["rays"]
                cams = orbit_cameras(r._camera, 2)
                vs = [d.render_views(r, cams) for d in (ds, ref)]
                assert np.array_equal(vs[0].rgb8, vs[1].rgb8)
                assert np.array_equal(_u32(vs[0].linear_rgb), _u32(vs[1].linear_rgb))
                assert vs[0].stats["rays_per_depth"] == vs[1].stats["rays_per_depth"]
                rng = np.random.default_rng(11)
                rays = np.concatenate([np.asarray(ds.camera_rays(r), np.float32).reshape(-1, 6),
                                       np.concatenate([rng.uniform(-6, 6, (4096, 3)), rng.normal(size=(4096, 3))], 1).astype(np.float32)])
                for bvh in (True, False):
                    hits = [d.trace(rays, bvh, seed=3) for d in (ds, ref)]
                    assert hits[0].tobytes() == hits[1].tobytes()
            finally:
                ref.close()
        finally:
            ds.close()


OPTIONS = [dict(WIDE="0"), dict(BVH="median"), dict(EXACT_ALL="1"), dict(NO_SHORT_RAYS="1"), dict(NO_TILE_ORDER="1"),
           dict(DEP_PIXEL_MAJOR="1"), dict(DEP_SLOT_MAJOR="1"), dict(NO_HOIST="1"), dict(BUILD="device"), dict(BUILD="host")]


@pytest.mark.parametrize("opts", OPTIONS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in OPTIONS])
def test_options(opts):
    with _lib.options(**opts):
        for name, w, h, spp, bvh in (("C3_suzanne", 40, 32, 4, True), ("C1_random_spheres", 40, 32, 4, True), ("C2_cornell_box", 32, 32, 8, False)):
            s, r = scenes.config(name, w, h, spp)
            r = _walk(r, bvh)
            ds = _lib.DeviceScene(s.to_desc())
            try:
                animate(s, np.random.default_rng(5))
                ds.update(s)
                assert_same(ds.render(r), fresh_renders(s, [r])[0])
            finally:
                ds.close()


def test_graph_never_replays_a_stale_frame():
    s, r = scenes.config("C1_random_spheres", 48, 32, 4)
    ds = _lib.DeviceScene(s.to_desc())
    try:
        with _lib.options(GRAPH="1"):
            a = [ds.render(r) for _ in range(2)]
            assert a[1].stats["reserved"] & 0x80000000
            rng = np.random.default_rng(9)
            for _ in range(2):        # the first update moves the object sections to memory of the scene's own; the second rewrites it
                animate(s, rng)
                ds.update(s)
                want = fresh_renders(s, [r])[0]
                for got in [ds.render(r) for _ in range(2)]:
                    assert_same(got, want)
            ds.update(s)              # an identical description: the same bytes in the same memory, and the cached graph replays
            again = [ds.render(r) for _ in range(2)]
            assert again[0].stats["reserved"] & 0x80000000
            for got in again:
                assert_same(got, want)
    finally:
        ds.close()


def test_oracle_after_update(oracle):
    s, r = scenes.config("C2_cornell_box", 32, 32, 16)
    ds = _lib.DeviceScene(s.to_desc())
    try:
        boxes = [ro for ro in s.render_objects if isinstance(ro.obj, Rect3d)]
        assert len(boxes) == 2
        boxes[0].position(200.0, 0.0, 100.0).rotate(Rotor3.from_euler_angles(0.0, 0.4, 0.0))
        boxes[1].position(300.0, 0.0, 320.0).rotate(Rotor3.from_euler_angles(0.1, -0.3, 0.0))
        ds.update(s)
        gpu = ds.render(r)
        cpu = oracle.render(s, r)
        assert np.array_equal(np.asarray(gpu.rgb8).reshape(-1, 3), np.asarray(cpu.rgb8).reshape(-1, 3))
    finally:
        ds.close()


def test_mesh_reach_grows_and_shrinks(capfd):
    s, r = scenes.config("C3_suzanne", 40, 32, 4)
    ds = _lib.DeviceScene(s.to_desc())
    try:
        light = s.render_objects[2]
        home = light._position.copy()
        with _lib.options(TRACE="1"):
            capfd.readouterr()
            light.position(1.0e4, 0.0, 0.0)
            ds.update(s)
            err = capfd.readouterr().err
            far = update_lines(err)
            assert len(far) == 1 and far[0][3] == 1, far           # the scene's one mesh, built again with the scene re-created
            assert "scene re-created: the reach of 1 meshes rose" in err, err
            assert_same(ds.render(r), fresh_renders(s, [r])[0])
            light.position_vec(home)
            capfd.readouterr()
            ds.update(s)
            err = capfd.readouterr().err
            back = update_lines(err)
            assert len(back) == 1 and back[0][3] == 0, back
            assert "re-created" not in err
            assert_same(ds.render(r), fresh_renders(s, [r])[0])
    finally:
        ds.close()


def _hoist_scene():
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.6, 0.5, 0.4)))
    g = sc.add_material(LambertianMat.with_color((0.3, 0.7, 0.3)))
    big = sc.add_object(RenderObject.new(Sphere.new(12.0, g)))
    for i in range(4):
        for j in range(4):
            sc.add_object(RenderObject.new(Sphere.new(0.6, m)).position(-4.5 + 3.0 * i, -4.5 + 3.0 * j, -14.0))
    sc.set_environment(SkyEnv.default())
    cam = CameraSettings.default().cam_pos((0.0, 2.0, -40.0)).look_at((0.0, 0.0, 0.0)).field_of_view(50.0)
    return sc, big, Renderer.default().width(48).height(32).samples(4).use_bvh(True).camera(cam)


def test_hoisting_changes(capfd):
    sc, big, r = _hoist_scene()
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        with _lib.options(TRACE="1"):
            capfd.readouterr()
            ds.update(sc)
            before = update_lines(capfd.readouterr().err)
            sc.render_objects[big].position(900.0, 0.0, 400.0)
            ds.update(sc)
            after = update_lines(capfd.readouterr().err)
        assert before[0][5] >= 1 and after[0][5] == 0, (before, after)
        assert_same(ds.render(r), fresh_renders(sc, [r])[0])
    finally:
        ds.close()


def _status(fn):
    try:
        fn()
    except _lib.FireworkError as e:
        return e.status
    return A.FW_OK


def test_rejected_updates_leave_the_scene_as_it_was():
    lib = _lib.load()
    for name in ("C2_cornell_box", "C3_suzanne"):
        s, r = scenes.config(name, 32, 24, 4)
        ds = _lib.DeviceScene(s.to_desc())
        try:
            before = ds.render(r)
            cases = []
            plus = scenes.config(name, 32, 24, 4)[0]
            plus.add_object(RenderObject.new(Sphere.new(0.5, 0)).position(0.0, 1.0, 0.0))
            cases.append(("one more object", plus.to_desc()))
            d = s.to_desc()
            d.objects[0].shape = (d.objects[0].shape + 1) % d.desc.n_shapes
            cases.append(("another shape index", d))
            d = s.to_desc()
            t = next(i for i in range(d.desc.n_textures) if d.textures[i].kind == A.FW_TEX_CONSTANT)
            d.textures[t].color.x += 0.25
            cases.append(("a material colour", d))
            d = s.to_desc()
            d.materials[0].roughness += 0.5
            cases.append(("a material field", d))
            d = s.to_desc()
            d.desc.environment.color.y += 0.5          # (a nested ctypes struct: written in place)
            cases.append(("the environment colour", d))
            d = s.to_desc()
            k = next((i for i in range(d.desc.n_shapes) if d.shapes[i].kind == A.FW_SHAPE_TRIANGLE_MESH), None)
            if k is not None:
                d.shapes[k].n_verts -= 1
                cases.append(("n_verts", d))
            d = s.to_desc()
            k = next(i for i in range(d.desc.n_shapes) if d.shapes[i].kind != A.FW_SHAPE_TRIANGLE_MESH)
            d.shapes[k].radius += 1.0
            cases.append(("a radius", d))
            for what, desc in cases:
                assert _status(lambda: ds.update(desc)) == A.FW_ERR_BAD_ARG, what
                assert_same(ds.render(r), before)
            nan = scenes.config(name, 32, 24, 4)[0]
            nan.render_objects[-1].position(float("nan"), 0.0, 0.0)
            nd = nan.to_desc()
            h = C.c_void_p()
            want = lib.fw_scene_create(nd.ptr(), 0, C.byref(h))
            if h:
                lib.fw_scene_destroy(h)
            assert want == A.FW_ERR_NAN_BBOX
            assert _status(lambda: ds.update(nd)) == want
            assert_same(ds.render(r), before)
            assert lib.fw_scene_update(ds.handle, None) == A.FW_ERR_BAD_ARG
            assert_same(ds.render(r), before)
        finally:
            ds.close()


_UPLOAD_CHILD = r"""
import numpy as np
from firework_amd import _lib
from firework_amd.api import CameraSettings, LambertianMat, Renderer, RenderObject, Scene, SkyEnv, Sphere, TriangleMesh

def grid_mesh(n, material):                      # an n x n vertex grid over [-4, 4]^2 with a sine height: 2 (n - 1)^2 triangles
    xs = np.linspace(-4, 4, n, dtype=np.float32)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = (0.4 * np.sin(2 * X) * np.cos(2 * Z)).astype(np.float32)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1); b = a + 1; c = a + n; d = c + 1
    idx = np.stack([a, b, c, b, d, c], -1).reshape(-1).astype(np.uint32)
    return TriangleMesh.new(verts, idx, None, None, material)

sc = Scene.new()
m = sc.add_material(LambertianMat.with_color((0.7, 0.6, 0.5)))
sc.add_object(RenderObject.new(grid_mesh(101, m)).position(0.0, 1.0, 0.0))
ball = sc.add_object(RenderObject.new(Sphere.new(0.8, m)).position(0.0, 2.5, 0.0))
sc.set_environment(SkyEnv.default())
cam = CameraSettings.default().cam_pos((0.0, 6.0, -12.0)).look_at((0.0, 1.0, 0.0)).field_of_view(40.0)
r = Renderer.default().width(48).height(32).samples(4).use_bvh(True).camera(cam)
ds = _lib.DeviceScene(sc.to_desc())
ds.render(r)
sc.render_objects[ball].position(1.5, 2.0, -1.0)
ds.update(sc)
got = ds.render(r)
ref = _lib.DeviceScene(sc.to_desc())
want = ref.render(r)
assert np.array_equal(got.rgb8, want.rgb8) and np.array_equal(got.linear.view(np.uint32), want.linear.view(np.uint32))
assert got.stats["rays_per_depth"] == want.stats["rays_per_depth"]
print("UPLOAD_OK", flush=True)
"""


def test_update_uploads_only_the_object_level():
    env = dict(os.environ, FIREWORK_TRACE="1")
    p = subprocess.run([sys.executable, "-c", _UPLOAD_CHILD], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert p.returncode == 0 and "UPLOAD_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    lines = update_lines(p.stderr)
    assert len(lines) == 1, p.stderr[-4000:]
    n_obj, _ms, _dev, rebuilt, uploaded, _hoisted = lines[0]
    assert n_obj == 2 and rebuilt == 0
    assert uploaded < 64 * 1024, uploaded
    blobs = [int(x) for x in re.findall(r"scene_create: build [\d.]+ ms, blob [\d.]+ ms \((\d+) B\)", p.stderr)]
    assert blobs and blobs[0] > 20000 * 48, blobs      # the triangle section alone: 20 000 triangles x 48 B
