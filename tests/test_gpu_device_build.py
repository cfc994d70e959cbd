"""The device tree builders (fw_build.hip) against the host builders: both trees (the reference's median split, the binned SAH tree) must
come out the same nodes bit for bit — compared as uint32 words — with the same sizes and depths; and scenes built with BUILD=device must
render what BUILD=host renders."""
import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import TriangleMesh

pytestmark = pytest.mark.gpu


def _boxes(n, seed, flat=False):              # as tests/test_host_build_cpu.py
    r = np.random.default_rng(seed)
    c = r.uniform(-10, 10, (n, 3)).astype(np.float32)
    if flat:
        c[:, 1] = np.float32(0.25)
        c[: n // 3, 0] = np.float32(1.5)
    e = r.uniform(0.001, 0.3, (n, 3)).astype(np.float32)
    return np.concatenate([c - e, c + e], axis=1)


def _trees(b, device):
    ref, sah, st = _lib.selftest_bvh_trees(b, device)
    return ref.view(np.uint32), sah.view(np.uint32), st


def _assert_same(b, what, zero_sign=False):
    host = _trees(b, -1)
    dev = _trees(b, 0)
    assert np.array_equal(host[2], dev[2]), (what, host[2], dev[2])
    for k, name in ((0, "median"), (1, "sah")):
        h, d = host[k], dev[k]
        if zero_sign:         # -0 and +0 as one value in the box floats; item ids, axes and child indices exact
            h, d = h.copy(), d.copy()
            for a in (h, d):
                box = a[:, [0, 1, 2, 4, 5, 6]]
                box[box == 0x80000000] = 0
                a[:, [0, 1, 2, 4, 5, 6]] = box
        bad = np.nonzero((h != d).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} tree differs in {bad.size} of {h.shape[0]} nodes, first {bad[:5]}: host {h[bad[:2]]} device {d[bad[:2]]}"


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 968, 1409, 4095, 4096, 4097, 70001, 300000, (1 << 20) + 3])
def test_random_boxes(n):
    _assert_same(_boxes(n, 7 * n), f"n={n}")


@pytest.mark.parametrize("n", [5, 1000, 70001])
def test_flat_sets(n):
    _assert_same(_boxes(n, 7 * n + 1, flat=True), f"flat n={n}")


@pytest.mark.parametrize("n", [3, 64, 5000])
def test_identical_centres(n):
    """every centroid the same: the SAH tree is the median fallback all the way down"""
    r = np.random.default_rng(n)
    e = r.uniform(0.01, 1.0, (n, 3)).astype(np.float32)
    _assert_same(np.concatenate([np.float32(2.0) - e, np.float32(2.0) + e], axis=1), f"identical n={n}")


def test_sah_past_max_depth():
    """geometrically spaced items (2^(k/2), k = -250..251, four of each): the bins tell only the largest few apart, so each split cuts a
    few off the top and the tree runs past SAH_MAX_DEPTH (40) into the median fallback"""
    x = np.repeat(np.float32(2.0) ** (np.arange(-250, 252, dtype=np.float32) / np.float32(2)), 4).astype(np.float32)
    c = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    b = np.concatenate([c - np.float32(0.25) * x[:, None], c + np.float32(0.25) * x[:, None]], axis=1).astype(np.float32)
    _, _, st = _trees(b, -1)
    assert st[3] > 40, st
    _assert_same(b, "geometric")


def test_huge_and_subnormal_magnitudes():
    r = np.random.default_rng(5)
    big = _boxes(20000, 11) * np.float32(1e29)
    tiny = (_boxes(20000, 12) * np.float32(1e-39)).astype(np.float32)
    _assert_same(big, "1e30")
    _assert_same(tiny, "subnormal")
    mixed = np.concatenate([big[:5000], tiny[:5000], _boxes(5000, 13)])
    _assert_same(mixed[r.permutation(mixed.shape[0])], "mixed")


def test_signed_zeros():
    r = np.random.default_rng(9)
    n = 20000
    b = r.choice(np.array([0.0, -0.0, 1.0, -1.0, 0.5], np.float32), size=(n, 6)).astype(np.float32)
    lo, hi = np.minimum(b[:, :3], b[:, 3:]), np.maximum(b[:, :3], b[:, 3:])
    _assert_same(np.concatenate([lo, hi], 1), "signed zeros", zero_sign=True)


def test_nan_centre_is_an_error_then_the_device_builds_again():
    b = _boxes(5000, 1)
    b[1717, 0] = np.nan
    b[1717, 3] = np.nan
    with pytest.raises(_lib.FireworkError) as e:
        _lib.selftest_bvh_trees(b, 0)
    assert e.value.status == A.FW_ERR_NAN_BBOX
    _assert_same(_boxes(5000, 2), "after NaN")


# ---- triangle boxes of real meshes, raw and grown as Flattener grows them (fw_runtime.cpp mesh_params) ----
def _tri_boxes(verts, idx):
    p = verts[idx.reshape(-1, 3)]                         # (t, 3, 3)
    mn, mx = p.min(axis=1), p.max(axis=1)
    small = np.abs(mx - mn) < np.float32(0.001)
    mn = np.where(small, mn - np.float32(0.001), mn).astype(np.float32)
    mx = np.where(small, mx + np.float32(0.001), mx).astype(np.float32)
    return np.concatenate([mn, mx], 1).astype(np.float32)


def _grown(b):
    ext_all = np.float32(np.max(b[:, 3:].max(0) - b[:, :3].min(0)))
    typ = np.float32(ext_all / np.sqrt(np.float32(b.shape[0])))
    ext = np.max(np.abs(b[:, 3:] - b[:, :3]), axis=1)
    g = np.maximum(np.ldexp(typ, -6), np.ldexp(ext, -14)).astype(np.float32)[:, None]
    return np.concatenate([b[:, :3] - g, b[:, 3:] + g], 1).astype(np.float32)


def _grid(n):                                            # tools/big_mesh.py grid_mesh
    xs = np.linspace(-4, 4, n, dtype=np.float32)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = (0.4 * np.sin(2 * X) * np.cos(2 * Z)).astype(np.float32)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1); b = a + 1; c = a + n; d = c + 1
    return verts, np.stack([a, b, c, b, d, c], -1).reshape(-1).astype(np.uint32)


def _scene_meshes(name):
    s, _ = scenes.config(name, 16, 16, 1)
    return [v for o in s.render_objects for v in vars(o).values() if isinstance(v, TriangleMesh)]


@pytest.mark.parametrize("name", ["C3_suzanne", "teapot"])
def test_scene_meshes(name):
    for k, m in enumerate(_scene_meshes(name)):
        b = _tri_boxes(m.verts, m.indicies)
        _assert_same(b, f"{name} mesh {k} raw")
        _assert_same(_grown(b), f"{name} mesh {k} grown")


def test_million_triangle_grid():
    v, i = _grid(709)
    b = _tri_boxes(v, i)
    assert b.shape[0] > 1_000_000
    _assert_same(b, "grid raw")
    _assert_same(_grown(b), "grid grown")


# ---- scene level: BUILD=device renders what BUILD=host renders ----
def _render(name, build, w=96, h=64, spp=4, **opts):
    _lib.set_option("BUILD", build)
    for k, v in opts.items():
        _lib.set_option(k, v)
    try:
        scene, r = scenes.config(name, w, h, spp)
        r = r.use_bvh(True)
        res = r.render_full(scene)
        return res.rgb8.copy(), int(res.stats["rays"]), int(res.stats["tlas_nodes"]), int(res.stats["blas_nodes"])
    finally:
        _lib.set_option("BUILD", None)
        for k in opts:
            _lib.set_option(k, None)


@pytest.mark.parametrize("name,opts", [("C3_suzanne", {}), ("teapot", {}), ("C5_part2_all", {}), ("conics", {}), ("C3_suzanne", {"BVH": "median"})])
def test_scene_renders_equal(name, opts):
    host = _render(name, "host", **opts)
    dev = _render(name, "device", **opts)
    assert host[1:] == dev[1:], (name, host[1:], dev[1:])
    assert np.array_equal(host[0], dev[0]), (name, int((host[0] != dev[0]).sum()))


def test_trace_batch_equal():
    scene, r = scenes.config("C3_suzanne", 64, 48, 1)
    out = []
    for build in ("host", "device"):
        _lib.set_option("BUILD", build)
        try:
            ds = _lib.DeviceScene(scene.to_desc())
            try:
                rays = ds.camera_rays(r)
                out.append(ds.trace(rays, True))
            finally:
                ds.close()
        finally:
            _lib.set_option("BUILD", None)
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))


def test_million_triangle_scene_equal():
    from firework_amd.api import CameraSettings, LambertianMat, Renderer, RenderObject, Scene, SkyEnv, XZRect
    v, i = _grid(709)
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.7, 0.6, 0.5)))
    sc.add_object(RenderObject.new(TriangleMesh.new(v, i, None, None, m)).position(0.0, 1.0, 0.0))
    sc.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 20.0, -0.5, m)))
    sc.set_environment(SkyEnv.default())
    cam = CameraSettings.default().cam_pos((0.0, 6.0, -12.0)).look_at((0.0, 1.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().width(160).height(90).samples(4).use_bvh(True).camera(cam)
    res = []
    for build in ("host", "device"):
        _lib.set_option("BUILD", build)
        try:
            x = r.render_full(sc)
            res.append((x.rgb8.copy(), int(x.stats["rays"]), int(x.stats["tlas_nodes"]), int(x.stats["blas_nodes"])))
        finally:
            _lib.set_option("BUILD", None)
    assert res[0][1:] == res[1][1:]
    assert np.array_equal(res[0][0], res[1][0])


def test_build_after_release_workspace():
    """fw_release_workspace also frees the device builder's memory; the next build allocates it again"""
    b = _boxes(70001, 3)
    first = _trees(b, 0)
    _lib.release_workspace(0)
    again = _trees(b, 0)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)


@pytest.mark.skipif(_lib.device_count() < 2, reason="needs two GPUs")
def test_second_device():
    """a scene on device 1: the mesh's median tree is built on a helper thread whose current device is the default one; the build must
    still run on device 1"""
    b = _boxes(5000, 4)
    ref, sah, st = _lib.selftest_bvh_trees(b, 1)
    host = _trees(b, -1)
    assert np.array_equal(ref.view(np.uint32), host[0]) and np.array_equal(sah.view(np.uint32), host[1]) and np.array_equal(st, host[2])
    v, i = _grid(101)                                    # 20 000 triangles: the two trees are built side by side
    from firework_amd.api import CameraSettings, LambertianMat, Renderer, RenderObject, Scene, SkyEnv
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.7, 0.6, 0.5)))
    sc.add_object(RenderObject.new(TriangleMesh.new(v, i, None, None, m)).position(0.0, 1.0, 0.0))
    sc.set_environment(SkyEnv.default())
    cam = CameraSettings.default().cam_pos((0.0, 6.0, -12.0)).look_at((0.0, 1.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().width(96).height(64).samples(4).use_bvh(True).camera(cam)
    res = []
    for build in ("host", "device"):
        _lib.set_option("BUILD", build)
        try:
            x = r.render_full(sc, None, 1)
            res.append((x.rgb8.copy(), int(x.stats["rays"]), int(x.stats["blas_nodes"])))
        finally:
            _lib.set_option("BUILD", None)
    assert res[0][1:] == res[1][1:]
    assert np.array_equal(res[0][0], res[1][0])
