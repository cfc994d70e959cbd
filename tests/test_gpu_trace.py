"""Ray queries on the GPU (fw_trace_rays / fw_camera_rays) against the CPU oracle, with zero tolerance: every float field bit for bit
(NaN-aware), every integer exactly.  One root.hit(ray, 0.001, 2e9) per ray is oracle.trace (fwo_trace); the camera rays and the
secondary rays of real paths come from oracle.trace_path."""
import os
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import CameraSettings

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_HIT = A.FW_NO_HIT

# (config, width, height, modes): use_bvh 0 and 1 where the scene allows (the linear scan of part2's ~500 objects is the oracle's
# slowest, so C5 keeps its configured BVH only)
SCENES = [("C1_random_spheres", 200, 120, (0, 1)), ("C2_cornell_box", 128, 128, (0, 1)), ("C3_suzanne", 160, 90, (0, 1)),
          ("C4a_hdri_test", 128, 128, (0, 1)), ("C4b_volume_test", 128, 128, (0, 1)), ("C5_part2_all", 192, 108, (1,)),
          ("teapot", 160, 120, (0, 1)), ("conics", 160, 120, (0, 1))]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def compare(gpu, ora, what=""):
    """gpu: HIT_DTYPE records; ora: oracle.trace rows (hit, t, point, normal, material, u)."""
    # A ray that starts exactly in a plane and runs inside it meets the plane at t = 0/0: the reference accepts that NaN (or inf) t
    # as a hit (no comparison rejects it), and which one of several such "hits" wins depends on the order of the tests.  These rays
    # are counted, not compared (the exact walk does not take them yet).
    odd = (ora[:, 0] == 1) & ~np.isfinite(ora[:, 1])
    if odd.any():
        print(f"{what}: {int(odd.sum())} rays with a non-finite oracle t left out")
        gpu, ora = gpu[~odd], ora[~odd]
    hit, ohit = gpu["object"] != NO_HIT, ora[:, 0] == 1
    bad = np.nonzero(hit != ohit)[0]
    assert bad.size == 0, f"{what}: hit flag differs for {bad.size} rays, first {bad[:5]}"
    miss = ~hit
    assert (gpu["t"][miss] == 0).all() and (gpu["point"][miss] == 0).all() and (gpu["material"][miss] == 0).all() and (gpu["prim"][miss] == 0).all()
    g, o = gpu[hit], ora[hit]
    for name, a, b in (("t", g["t"], o[:, 1]), ("point", g["point"], o[:, 2:5]), ("normal", g["normal"], o[:, 5:8]), ("u", g["u"], o[:, 9])):
        ok = _same(a, b)
        ok = ok.all(axis=1) if ok.ndim == 2 else ok
        assert ok.all(), f"{what}: {name} differs for {(~ok).sum()} of {ok.size} hits, first at {np.nonzero(~ok)[0][:5]}"
    assert (g["material"] == o[:, 8].astype(np.uint32)).all(), what


def lattice_pixels(renderer, n=4096):
    w, h = renderer.settings["width"], renderer.settings["height"]
    return np.unique(np.linspace(0, w * h - 1, n).astype(np.uint32))


def camera_set(ds, renderer, n=4096):
    ids = lattice_pixels(renderer, n)
    return np.concatenate([ds.camera_rays(renderer, s, ids) for s in (0, 7)])


def secondary_set(oracle, scene, renderer, n_paths=200):
    rng = np.random.default_rng(5)
    w, h = renderer.settings["width"], renderer.settings["height"]
    out = []
    for _ in range(n_paths):
        rows, _c = oracle.trace_path(scene, renderer, int(rng.integers(w * h)), int(rng.integers(64)))
        out.append(rows[1:][rows[1:, 15] != 0][:, :6])
    return np.concatenate(out).astype(np.float32)


def scene_box(oracle, scene):
    b = oracle.object_aabbs(scene)
    b = b[np.isfinite(b).all(axis=1)]
    return np.clip(b[:, :3].min(0), -1e3, 1e3), np.clip(b[:, 3:].max(0), -1e3, 1e3)


def adversarial_set(oracle, scene, ds, use_bvh, cam_rays, n=2048):
    """Origins inside the scene box with axis-parallel directions (+0 / -0 in the other components) and directions with one or
    two signed zeros; origins ON surfaces (the camera rays' hit points) leaving along the surface (grazing: tangents, exact zeros
    along the normal of an axis-aligned face) and into random directions."""
    rng = np.random.default_rng(11)
    lo, hi = scene_box(oracle, scene)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = np.zeros((n, 3), np.float32)
    ax = rng.integers(3, size=n)
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    zeros = np.where(rng.random((n, 3)) < 0.5, np.float32(-0.0), np.float32(0.0))
    d = np.where(d == 0, zeros, d)
    d2 = rng.normal(size=(n, 3)).astype(np.float32)
    k = rng.integers(3, size=n)
    d2[np.arange(n), k] = zeros[np.arange(n), k]
    d2[: n // 4, (k[: n // 4] + 1) % 3] = np.float32(-0.0)
    sets = [np.hstack([o, d]), np.hstack([o, d2])]
    h = ds.trace(cam_rays, use_bvh)
    hit = h["object"] != NO_HIT
    if hit.any():
        p, nrm = h["point"][hit][:n], h["normal"][hit][:n]
        m = p.shape[0]
        axis = np.eye(3, dtype=np.float32)[rng.integers(3, size=m)]
        t1 = np.cross(nrm, axis).astype(np.float32)
        t2 = np.cross(nrm, rng.normal(size=(m, 3))).astype(np.float32)
        r3 = rng.normal(size=(m, 3)).astype(np.float32)
        sets += [np.hstack([p, t1]), np.hstack([p, t2]), np.hstack([p, r3])]
    rays = np.concatenate(sets).astype(np.float32)
    return rays[(rays[:, 3:] != 0).any(axis=1)]       # a zero direction is a miss by contract (test_non_finite_and_zero_direction_rays_are_misses)


@pytest.fixture(scope="module")
def ray_sets(oracle):
    """Per scene: (scene, renderer, camera, secondary, adversarial-by-mode) ray sets, each made once."""
    cache = {}

    def get(name, w, h):
        if name not in cache:
            scene, renderer = scenes.config(name, w, h, 64)
            ds = _lib.DeviceScene(scene.to_desc())
            cam = camera_set(ds, renderer)
            sec = secondary_set(oracle, scene, renderer)
            adv = {m: adversarial_set(oracle, scene, ds, m, cam[:4096]) for m in (0, 1)}
            cache[name] = (scene, renderer, ds, cam, sec, adv)
        return cache[name]
    yield get
    for v in cache.values():
        v[2].close()


@pytest.mark.parametrize("name,w,h,modes", SCENES, ids=[s[0] for s in SCENES])
def test_trace_parity_with_oracle(oracle, ray_sets, name, w, h, modes):
    scene, renderer, ds, cam, sec, adv = ray_sets(name, w, h)
    for m in modes:
        for label, rays in (("camera", cam), ("secondary", sec), ("adversarial", adv[m])):
            gpu = ds.trace(rays, m)
            compare(gpu, oracle.trace(scene, rays, m), f"{name} use_bvh={m} {label}")


def _rect3d_objects(scene):
    sd = scene.to_desc().desc
    return {i for i in range(sd.n_objects) if sd.shapes[sd.objects[i].shape].kind == A.FW_SHAPE_RECT3D}


@pytest.mark.parametrize("name", ["C1_random_spheres", "C2_cornell_box", "C5_part2_all"])
def test_v_object_and_prim(oracle, ray_sets, name):
    w, h = {s[0]: s[1:3] for s in SCENES}[name]
    scene, renderer, ds, cam, sec, adv = ray_sets(name, w, h)
    rays = np.concatenate([cam, sec])
    g = ds.trace(rays, renderer.settings["use_bvh"])
    hit = g["object"] != NO_HIT
    assert hit.any()
    sd = scene.to_desc().desc
    boxes = oracle.object_aabbs(scene)
    # object: an object of the hit's material whose box holds the point (a box is padded by ~1e-4 of its extent for the rounding of points)
    for i in np.nonzero(hit)[0][:3000]:
        k = int(g["object"][i])
        assert k < sd.n_objects
        shape = sd.shapes[sd.objects[k].shape]
        assert shape.material == int(g["material"][i]) or shape.kind == A.FW_SHAPE_CONSTANT_MEDIUM
        lo, hi = boxes[k, :3], boxes[k, 3:]
        pad = 1e-4 * (np.abs(lo) + np.abs(hi) + 1.0)
        assert ((g["point"][i] >= lo - pad) & (g["point"][i] <= hi + pad)).all(), (i, k)
    # v of an unrotated sphere: sphere_uv of the object-space normal (= the world normal, without flip_normals)
    for i in np.nonzero(hit)[0][:2000]:
        k = int(g["object"][i])
        ob = sd.objects[k]
        if sd.shapes[ob.shape].kind != A.FW_SHAPE_SPHERE or ob.flip_normals or (ob.rotation.s, ob.rotation.xy, ob.rotation.xz, ob.rotation.yz) != (1.0, 0.0, 0.0, 0.0):
            continue
        u, v = oracle.sphere_uv(g["normal"][i])
        assert _same(np.float32(u), g["u"][i]) and _same(np.float32(v), g["v"][i]), i
    # prim of a Rect3d: one face = one normal; faces 2k and 2k+1 face opposite ways
    boxes3 = _rect3d_objects(scene)
    seen = {}
    for i in np.nonzero(hit)[0]:
        k, p = int(g["object"][i]), int(g["prim"][i])
        if k not in boxes3:
            continue
        assert p < 6
        seen.setdefault((k, p), set()).add(tuple(_bits(g["normal"][i])))
    for (k, p), ns in seen.items():
        assert len(ns) == 1, (k, p, ns)
        other = seen.get((k, p ^ 1))
        if other:
            assert np.array_equal(-np.array(next(iter(ns)), np.uint32).view(np.float32), np.array(next(iter(other)), np.uint32).view(np.float32))


WALK_OPTIONS = [dict(BVH="median"), dict(WIDE="0"), dict(WIDE="f32"), dict(WIDE="q8"), dict(EXACT_ALL="1"), dict(EXACT_FORM="lane"),
                dict(EXACT_FORM="wave"), dict(NO_DEFER="1"), dict(NO_HIT4="1"), dict(NO_LDS_TREES="1"), dict(NO_LDS_TRIS="1"),
                dict(WAVES="64"), dict(PATHS_PER_BATCH="5000")]


@pytest.mark.parametrize("name", ["C2_cornell_box", "C3_suzanne", "C5_part2_all"])
def test_walk_variants_keep_parity(oracle, ray_sets, name):
    w, h = {s[0]: s[1:3] for s in SCENES}[name]
    scene, renderer, _ds, cam, sec, adv = ray_sets(name, w, h)
    m = int(renderer.settings["use_bvh"])
    rays = np.concatenate([cam[:4096], sec, adv[m]])
    ref = oracle.trace(scene, rays, m)
    for opt in WALK_OPTIONS:
        with _lib.options(**opt):
            ds = _lib.DeviceScene(scene.to_desc())        # BVH / WIDE apply to scenes created after them
            try:
                compare(ds.trace(rays, m), ref, f"{name} {opt}")
            finally:
                ds.close()


def _random_rays(oracle, scene, n, seed=3):
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(oracle, scene)
    o = lo + (hi - lo) * rng.random((n, 3))
    return np.hstack([o, rng.normal(size=(n, 3))]).astype(np.float32)


def test_batches_and_keys(oracle):
    scene, renderer = scenes.config("C4b_volume_test", 64, 64, 1)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = _random_rays(oracle, scene, 100_000)
        one = ds.trace(rays, 0, seed=9)
        st = {}
        many = ds.trace(rays, 0, seed=9, rays_per_batch=4096, stats=st)
        assert st["n_batches"] == 25
        assert one.tobytes() == many.tobytes()
        k = 12_345
        assert ds.trace(rays[k:], 0, seed=9, key_base=k).tobytes() == one[k:].tobytes()
        compare(ds.trace(rays[:20_000], 0, seed=9), oracle.trace(scene, rays[:20_000], False, 9), "C4b seed 9")
        assert st["rays"] == st["rays_per_depth"][0] == 100_000
    finally:
        ds.close()


def _camera_case(renderer, pixel_ids, samples, oracle, scene):
    for s in samples:
        got = _lib.camera_rays(renderer, s, pixel_ids)
        want = np.stack([oracle.trace_path(scene, renderer, int(p), s)[0][0, :6] for p in pixel_ids])
        assert (_bits(got) == _bits(want)).all(), (s, np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0][:5])


@pytest.mark.parametrize("case", ["C2", "C5", "thin_lens", "pos_plus0", "pos_minus0"])
def test_camera_rays_are_the_renders(oracle, case):
    name = {"C2": "C2_cornell_box", "C5": "C5_part2_all"}.get(case, "C4b_volume_test")
    scene, renderer = scenes.config(name, 96, 64, 1)
    if case == "thin_lens":
        renderer.camera(CameraSettings.default().cam_pos((1.0, 2.0, -9.0)).look_at((0.0, 0.5, 0.0)).aperture(0.3).focus_dist(9.0))
    elif case == "pos_plus0":
        renderer.camera(CameraSettings.default().cam_pos((0.0, 0.0, -10.0)))
    elif case == "pos_minus0":
        renderer.camera(CameraSettings.default().cam_pos((-0.0, 2.0, -10.0)))
    ids = lattice_pixels(renderer, 300)
    _camera_case(renderer, ids, (0, 3, 1000), oracle, scene)


def test_non_finite_and_zero_direction_rays_are_misses(oracle):
    scene, renderer = scenes.config("C2_cornell_box", 64, 64, 1)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        good = camera_set(ds, renderer, 512)
        clean = ds.trace(good, False)
        bad = np.repeat(good[:8], 8, axis=0)
        for j, v in enumerate([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf]):
            bad[8 * j:8 * j + 8, j % 6] = v
        bad[56:, 3:] = 0.0
        bad[60:, 3:] = -0.0
        mixed = np.empty((good.shape[0] + bad.shape[0], 6), np.float32)
        pos = np.random.default_rng(1).permutation(mixed.shape[0])
        gi, bi = np.sort(pos[: good.shape[0]]), np.sort(pos[good.shape[0]:])
        mixed[gi], mixed[bi] = good, bad
        st = {}
        out = ds.trace(mixed, False, stats=st)
        assert (out[bi]["object"] == NO_HIT).all()
        assert (out[bi].view(np.uint32).reshape(-1, 12)[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]] == 0).all()
        assert out[gi].tobytes() == clean.tobytes()
        assert st["rays"] == good.shape[0]
    finally:
        ds.close()


def test_trace_does_not_disturb_rendering(oracle):
    scene, renderer = scenes.config("C1_random_spheres", 200, 120, 8)
    with _lib.options(GRAPH="1"):
        ds = _lib.DeviceScene(scene.to_desc())
        try:
            a = ds.render(renderer)
            b = ds.render(renderer)
            rays = _random_rays(oracle, scene, 1_000_000)
            ds.trace(rays, True)
            c = ds.render(renderer)
        finally:
            ds.close()
    for x in (b, c):
        assert np.array_equal(a.rgb8, x.rgb8) and a.linear.tobytes() == x.linear.tobytes()


def test_torch_device_path_and_gbuffer(oracle):
    torch = pytest.importorskip("torch")
    scene, renderer = scenes.config("C3_suzanne", 96, 64, 1)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = np.concatenate([camera_set(ds, renderer, 2048), _random_rays(oracle, scene, 4096)])
        host = ds.trace(rays, True, seed=4)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dev = torch.from_numpy(rays).to("cuda:0", non_blocking=False)
            rec = ds.trace(dev, True, seed=4)
        s.synchronize()
        assert rec.shape == (rays.shape[0], 12) and rec.dtype == torch.float32
        assert rec.cpu().numpy().tobytes() == host.tobytes()
        f = _lib.hit_fields(rec)
        assert (f["object"].cpu().numpy().view(np.uint32) == host["object"]).all()
        # gbuffer = trace(camera_rays) reshaped
        gb = renderer.gbuffer(ds)
        w, h = renderer.settings["width"], renderer.settings["height"]
        ref = ds.trace(ds.camera_rays(renderer, 0), renderer.settings["use_bvh"], seed=renderer.settings["seed"])
        for k in _lib.HIT_DTYPE.names:
            assert gb[k].shape[:2] == (h, w)
            assert gb[k].tobytes() == ref[k].tobytes(), k
    finally:
        ds.close()


def test_cpp_mirror_trace(tmp_path):
    """A small host against include/firework.hpp: its trace() of C2's camera rays equals the Python path's records."""
    scene, renderer = scenes.config("C2_cornell_box", 64, 64, 1)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = ds.camera_rays(renderer, 0)
        ref = ds.trace(rays, False)
    finally:
        ds.close()
    exe = tmp_path / "trace_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "examples", "trace_rays.cpp"),
                           "-L", os.path.join(ROOT, "firework_amd", "lib"), "-lfirework_hip", "-Wl,-rpath," + os.path.join(ROOT, "firework_amd", "lib")])
    out = tmp_path / "hits.bin"
    subprocess.check_call([str(exe), str(out)], timeout=300)
    got = np.fromfile(out, dtype=_lib.HIT_DTYPE)
    assert got.tobytes() == ref.tobytes()
