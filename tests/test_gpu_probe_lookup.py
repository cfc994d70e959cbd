"""Baked probes read back on the GPU (fw_probe_irradiance, fw_probe_shade, Renderer.render_probe_lit).

k_probe_irradiance against the numpy float64 statement (api.probe_lookup) within the bound of tests/probe_lookup_ref.py — derived from
the order of operations, nothing in it measured — over flat, small and uneven grids, a grid far from the origin, points inside, on
probes, on faces and edges and outside every face, normals that are not unit, wrap on and off, strides 3 and 12, host and device
arrays, a side stream; its determinism; k_probe_shade bit for bit against the float32 statement on the lookup's own output and against
fw_denoise's resolve at iterations = 0; render_probe_lit against the three public calls chained by hand, with fw_render left as it was;
a Lambertian sphere under a constant environment against its closed form a L; the CLI's round trip."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import ColorEnv, LambertianMat, ProbeGrid, ProbeSet, RenderObject, Scene, Sphere

import probe_lookup_ref as R
import probes_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
FAR = np.array([3e3, -2e3, 5e3])
# (lo, hi, counts): a single probe, one and two flat axes, the smallest full cell, an uneven grid, and two placed far from the origin
GRIDS = [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)), ((-1.0, 0.0, 0.0), (2.0, 1.0, 1.0), (2, 1, 1)), ((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (1, 3, 2)),
         ((0.0, 0.0, 0.0), (1.0, 2.0, 0.5), (2, 2, 2)), ((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5)),
         (tuple(FAR - 1.0), tuple(FAR + (1.0, 2.0, 0.5)), (2, 2, 2)), (tuple(FAR - (1.5, 0.25, 2.0)), tuple(FAR + (2.0, 1.75, 3.0)), (4, 3, 5))]
COUNTS_N = [1, 63, 64, 65, 200]      # one point, a wave's tail, a wave, a wave plus one, several waves with a tail


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _points(grid, n, rng):
    """n float32 points in turn strictly inside the grid, exactly on a probe, on a face, on an edge and outside a face (all six in
    turn), with normals of length 1, 0.5 and 3"""
    lo, hi = np.array(grid.lo), np.array(grid.hi)
    probes = ProbeSet.grid(grid.lo, grid.hi, grid.counts).positions
    pts = (lo + rng.uniform(0.05, 0.95, size=(n, 3)) * (hi - lo)).astype(np.float32)
    for i in range(n):
        kind, k = i % 5, (i // 5) % 3
        if kind == 1:
            pts[i] = probes[rng.integers(len(probes))]
        elif kind == 2:
            pts[i, k] = np.float32((lo, hi)[(i // 15) % 2][k])
        elif kind == 3:
            pts[i, k] = np.float32(lo[k])
            pts[i, (k + 1) % 3] = np.float32(hi[(k + 1) % 3])
        elif kind == 4:
            side = (i // 15) % 2
            pts[i, k] = np.float32((lo[k] - 0.75 * (hi[k] - lo[k]) - 0.5) if side == 0 else (hi[k] + 1.25 * (hi[k] - lo[k]) + 0.5))
    nrm = rng.normal(size=(n, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * np.array([1.0, 0.5, 3.0])[np.arange(n) % 3, None]
    return pts, nrm.astype(np.float32)


def _assert_within(got, ref, T, wrap, what):
    assert got.dtype == np.float32 and got.shape == ref.shape and np.all(np.isfinite(got)), what
    err, bound = np.abs(got.astype(np.float64) - ref), R.lookup_bound(ref, T, wrap)
    print(f"{what}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (what, float((err / bound).max()), np.argwhere(err > bound)[:4])


@pytest.mark.parametrize("lo,hi,counts", GRIDS)
def test_lookup_matches_the_float64_statement(lo, hi, counts):
    torch, dev = _torch()
    lib = _lib.load()
    rng = np.random.default_rng(sum(counts) * 7 + int(lo[0] > 100))
    n_probes = counts[0] * counts[1] * counts[2]
    sh = rng.normal(size=(n_probes, 9, 3)).astype(np.float32)                     # negative entries, negative lobes
    d_sh = torch.from_numpy(sh).to(dev)
    side = torch.cuda.Stream(device=dev)
    for wrap in (False, True):
        grid = ProbeGrid(lo, hi, counts, wrap)
        for n in COUNTS_N:
            pts, nrm = _points(grid, n, rng)
            ref, T = api.probe_lookup(grid, sh, pts, nrm, terms=True)
            what = f"{counts} wrap {wrap} n {n}"
            # host arrays, stride 3, into a NaN-filled buffer
            host = np.full((n, 3), NAN, np.float32)
            assert _lib.probe_irradiance(grid, sh, pts, nrm, out=host) is host
            _assert_within(host, ref, T, wrap, what + " host")
            # device arrays in place in 48-byte records (stride 12, pointers + 8 and + 4), into a NaN-filled tensor on a side stream
            rec = np.full((n, 12), NAN, np.float32)
            rec[:, 8:11], rec[:, 4:7] = pts, nrm
            d_rec = torch.from_numpy(rec).to(dev)
            out = torch.full((n, 3), NAN, dtype=torch.float32, device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                _lib.probe_irradiance(grid, d_sh, d_rec[:, 8:11], d_rec[:, 4:7], out=out)
            side.synchronize()
            assert np.array_equal(_u32(out.cpu().numpy()), _u32(host)), what + " device records"
            # device arrays, stride 3, the current stream
            got = _lib.probe_irradiance(grid, d_sh, torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev))
            assert np.array_equal(_u32(got.cpu().numpy()), _u32(host)), what + " device packed"
            assert np.array_equal(_u32(d_rec.cpu().numpy()), _u32(rec))                       # the records are only read
            # host arrays at stride 12 through the C call itself: the host's packing loop, every tail
            out12 = np.full((n, 3), NAN, np.float32)
            g = grid.to_abi()
            st = lib.fw_probe_irradiance(C.byref(g), sh.ctypes.data, 0, n, rec[:, 8:].ctypes.data, rec[:, 4:].ctypes.data, 12, out12.ctypes.data, 0,
                                         None)
            assert st == A.FW_OK and np.array_equal(_u32(out12), _u32(host)), what + " host records"


def test_lookup_is_deterministic_and_pointwise():
    rng = np.random.default_rng(5)
    grid = ProbeGrid((-1.5, 0.25, 2.0), (2.0, 1.75, 7.0), (4, 3, 5), True)
    sh = rng.normal(size=(60, 9, 3)).astype(np.float32)
    pts, nrm = _points(grid, 200, rng)
    first = _lib.probe_irradiance(grid, sh, pts, nrm)
    assert np.array_equal(_u32(_lib.probe_irradiance(grid, sh, pts, nrm)), _u32(first))
    perm = rng.permutation(200)
    assert np.array_equal(_u32(_lib.probe_irradiance(grid, sh, pts[perm], nrm[perm])), _u32(first[perm]))
    # a NaN position, an infinite one, a zero normal and a NaN normal give zeros; their neighbours keep their results
    bad_p, bad_n = pts.copy(), nrm.copy()
    bad_p[3, 1], bad_p[64, 0], bad_n[65] = NAN, np.inf, 0.0
    bad_n[130, 2] = NAN
    got = _lib.probe_irradiance(grid, sh, bad_p, bad_n)
    bad = np.zeros(200, bool)
    bad[[3, 64, 65, 130]] = True
    assert np.all(_u32(got[bad]) == 0) and np.array_equal(_u32(got[~bad]), _u32(first[~bad]))
    assert np.all(first[bad] != 0.0)


def _records(w, h, grid, rng):
    """synthetic fw_render_aovs records: coverage 0, 0.25 and 1 in turn; a coverage-0 record has a zero normal on every other pixel"""
    n = w * h
    pts, nrm = _points(grid, n, rng)
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
    rec[:, 3] = np.array([0.0, 0.25, 1.0], np.float32)[np.arange(n) % 3]
    rec[:, 4:7], rec[:, 8:11] = nrm, pts
    rec[::6, 4:7] = 0.0
    rec[:, 7] = rng.uniform(1.0, 9.0, size=n)
    return rec


@pytest.mark.parametrize("w,h", [(17, 5), (64, 1)])
def test_shade_is_the_float32_statement_on_the_lookups_output(w, h):
    torch, dev = _torch()
    rng = np.random.default_rng(w)
    n = w * h
    for wrap in (True, False):
        grid = ProbeGrid((0.0, -1.0, 2.0), (1.0, 1.0, 3.5), (3, 2, 2), wrap)
        sh = rng.normal(size=(12, 9, 3)).astype(np.float32)
        rec = _records(w, h, grid, rng)
        E = _lib.probe_irradiance(grid, sh, rec[:, 8:11], rec[:, 4:7])
        lit = rec[:, 3] > 0
        assert np.any(E[lit] < 0.0) and np.any(E[lit] > 0.0)                              # some lookups are clamped, some are not
        want = api.probe_shade_ref(grid, sh, rec, E)
        assert np.array_equal(_u32(want[rec[:, 3] == 0]), _u32(rec[rec[:, 3] == 0, 0:3]))    # coverage 0 passes the albedo through
        gamma = 2.2 if wrap else 1.7
        rgb8, gam, lin = _lib.probe_shade(grid, sh, rec, w, h, gamma)
        assert np.array_equal(_u32(lin), _u32(want))
        ref8, refg, refl = _lib.denoise(want, rec, None, w, h, 0, gamma)                     # resolve_pixel(out, 1, gamma), as fw_denoise writes it
        assert np.array_equal(_u32(refl), _u32(want))
        assert np.array_equal(_u32(gam), _u32(refg)) and np.array_equal(rgb8, ref8)
        # device arrays give the same bits, and any single output may be asked for alone
        d_sh, d_rec = torch.from_numpy(sh).to(dev), torch.from_numpy(rec).to(dev)
        d8, dg, dl = _lib.probe_shade(grid, d_sh, d_rec, w, h, gamma)
        assert np.array_equal(d8.cpu().numpy(), rgb8) and np.array_equal(_u32(dg.cpu().numpy()), _u32(gam)) and np.array_equal(_u32(dl.cpu().numpy()), _u32(lin))
        for k, (name, full) in enumerate((("rgb8", rgb8), ("gamma", gam), ("linear", lin))):
            for arrays in (_lib.probe_shade(grid, sh, rec, w, h, gamma, outputs=(name,)),
                           tuple(None if t is None else t.cpu().numpy() for t in _lib.probe_shade(grid, d_sh, d_rec, w, h, gamma, outputs=(name,)))):
                assert [a is None for a in arrays] == [j != k for j in range(3)]
                assert np.array_equal(arrays[k].view(np.uint8), full.view(np.uint8)), name


@pytest.mark.parametrize("graph", [None, "1"])
def test_render_probe_lit_is_its_composition_and_leaves_renders_alone(graph):
    """cornell at 32 x 24: render_probe_lit equals fw_render_aovs on the device, fw_probe_irradiance at stride 12 and the float32 formula
    chained by hand; fw_render before and after gives the same frame, and under GRAPH its repeated frame is still replayed (bit 31)"""
    torch, dev = _torch()
    scene, r = scenes.config("C2_cornell_box", 32, 24, 4)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        with _lib.options(GRAPH=graph):
            before = [ds.render(r) for _ in range(3)]
            sh, _sums = r.bake_probes(ds, probes, 1)
            for wrap in (True, False):
                res = r.render_probe_lit(ds, probes, sh, aov_samples=4, wrap=wrap)
                assert (res.width, res.height) == (32, 24)
                aov = ds.aovs(r, 4, out=torch.empty((32 * 24, 12), dtype=torch.float32, device=dev))
                grid = ProbeGrid.of(probes, wrap)
                E = _lib.probe_irradiance(grid, torch.from_numpy(sh).to(dev), aov[:, 8:11], aov[:, 4:7])
                rec = aov.cpu().numpy()
                want = api.probe_shade_ref(grid, sh, rec, E.cpu().numpy())
                assert np.array_equal(_u32(res.linear), _u32(want)), wrap
                ref8, refg, _ = _lib.denoise(want, rec, None, 32, 24, 0, r.settings["gamma"])
                assert np.array_equal(res.rgb8, ref8) and np.array_equal(_u32(res.gamma), _u32(refg)), wrap
                assert np.any(rec[:, 3] == 1.0) and len(np.unique(res.rgb8.reshape(-1, 3), axis=0)) > 8     # a picture, not a constant
            after = [ds.render(r) for _ in range(2)]
        for a in before[1:] + after:
            assert np.array_equal(a.rgb8, before[0].rgb8)
            assert np.array_equal(_u32(a.linear), _u32(before[0].linear))
            assert a.stats["rays"] == before[0].stats["rays"]
        if graph:
            assert before[2].stats["reserved"] & 0x80000000 and after[1].stats["reserved"] & 0x80000000
    finally:
        ds.close()


def test_render_probe_lit_through_a_camera_model():
    torch, dev = _torch()
    scene, r = scenes.config("C2_cornell_box", 32, 24, 4)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    model = api.CameraModel.panorama((278.0, 278.0, 278.0), 24, 12)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sh, _sums = r.bake_probes(ds, probes, 1)
        res = r.render_probe_lit(ds, probes, sh, aov_samples=2, model=model)
        rec = ds.model_aovs(model, 2, seed=r.settings["seed"], use_bvh=r.settings["use_bvh"])
    finally:
        ds.close()
    assert (res.width, res.height) == (24, 12)
    E = _lib.probe_irradiance(probes, sh, rec[:, 8:11], rec[:, 4:7])
    assert np.array_equal(_u32(res.linear), _u32(api.probe_shade_ref(probes, sh, rec, E)))


def test_a_lambertian_sphere_under_a_constant_environment():
    """A convex Lambertian surface of albedo a under the constant radiance L has the exact radiance a L.  The probes stand so far from
    the small sphere that none of their rays meets it (checked), so each holds the lattice's projection of the constant L, and the
    preview's pixels of coverage 1 must show a L.  The bound, per channel, with nh the record's normalised normal:
      - the device's lookup against api.probe_lookup of the baked sh: tests/probe_lookup_ref.py;
      - api.probe_lookup of the baked sh against pi L: the weights are non-negative and sum to 1 (their roundings are inside the lookup's
        bound), so at most sum_k A_k |Y_k(nh)| max over probes |sh_k - exact_k|, exact = (2 sqrt(pi) L, 0, ...); |sh_k - exact_k| is at
        most L times the lattice's C_k / D for the constant (probes_ref.quadrature_bound of Y_k), plus fw_probe_project's own bound
        against api.sh_project of the constant on the same rays (probes_ref.project_bound);
      - the float32 shade step at coverage 1: v x and x + 0 are exact, so E float32(1 / pi), the constant's own rounding and the product
        with the albedo: at most 4 x 2^-24 relative;
      - the albedo's float32 value (0.5, 0.25, 0.75: its sums over the samples are exact) and the environment's float32 L."""
    a, L = np.array([0.5, 0.25, 0.75]), np.array([0.75, 0.5, 0.25], np.float32).astype(np.float64)
    scene = Scene.new()
    m = scene.add_material(LambertianMat.with_color(tuple(a)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, m)).position(0.0, 0.0, 0.0))
    scene.set_environment(ColorEnv(tuple(L)))
    D = 256
    probes = ProbeSet.grid((-3000.0, -3000.0, -3000.0), (3000.0, 3000.0, 3000.0), (2, 2, 2), D).seed(9)
    cam = api.CameraSettings.default().cam_pos((0.0, 0.0, 6.0)).look_at((0.0, 0.0, 0.0)).field_of_view(30.0)
    r = api.Renderer.default().width(16).height(16).samples(1).use_bvh(True).seed(3).camera(cam)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rays = _lib.probe_rays(probes, 0)
        assert np.all(ds.trace(rays, True)["object"] == A.FW_NO_HIT)
        sh, sums = r.bake_probes(ds, probes, 1)
        res = r.render_probe_lit(ds, probes, sh, aov_samples=8)
        rec = ds.aovs(r, 8)
    finally:
        ds.close()
    acc = np.zeros((8 * D, 4), np.float32)
    acc[:, :3] = L
    proj = api.sh_project(rays, acc, 1, D)
    exact = np.zeros((9, 3))
    exact[0] = 2.0 * np.sqrt(np.pi) * L
    coeff = np.array([P.quadrature_bound(lambda x, k=k: api.sh_basis(x)[..., k], D) for k in range(9)])[:, None] * L.max()
    coeff = coeff + P.project_bound(proj, P.abs_terms(api, rays, acc, 1, D), np.zeros((8, 9, 3), np.float32), D).max(axis=0)
    assert np.all(np.abs(sh.astype(np.float64) - exact) <= coeff)                             # the bake itself is where it should be
    full = rec[:, 3] == 1.0
    assert full.sum() >= 16
    ref, T = api.probe_lookup(probes, sh, rec[:, 8:11], rec[:, 4:7], terms=True)
    nh = rec[full, 4:7].astype(np.float64)
    nh = nh / np.linalg.norm(nh, axis=1, keepdims=True)
    weight = np.abs(api.sh_basis(nh) * api._SH_COSINE)                                        # (n, 9)
    e_bound = R.lookup_bound(ref, T, True)[full] + weight @ coeff
    bound = (a / np.pi) * e_bound * (1.0 + 2.0 ** -20) + 4.0 * 2.0 ** -24 * a * L
    err = np.abs(res.linear[full].astype(np.float64) - a * L)
    print(f"largest error / bound {float((err / bound).max()):.3f} (largest error {float(err.max()):.3e})")
    assert np.all(err <= bound), float((err / bound).max())
    assert np.array_equal(_u32(rec[full, 0:3]), _u32(np.broadcast_to(a.astype(np.float32), (int(full.sum()), 3))))


def test_cli_bakes_a_grid_and_lights_a_view_from_it(tmp_path):
    from firework_amd.__main__ import main
    yml = os.path.join(ROOT, "scenes", "three_lights.yml")
    npz, png = str(tmp_path / "p.npz"), str(tmp_path / "lit.png")
    assert main(["--scene-file", yml, "-s", "2", "--bake-probes", "2,1,3", "--probe-min=-12,1,-12", "--probe-max", "12,9,12", "--probe-dirs", "32",
                 "-o", npz]) == 0
    with np.load(npz) as z:
        assert z["grid_lo"].tolist() == [-12.0, 1.0, -12.0] and z["grid_hi"].tolist() == [12.0, 9.0, 12.0] and z["grid_counts"].tolist() == [2, 1, 3]
        assert z["grid_lo"].dtype == np.float64 and z["sh"].shape == (6, 9, 3) and z["positions"].shape == (6, 3)
        grid, sh = ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"], False), z["sh"]
    assert main(["--scene-file", yml, "-s", "2", "--probe-lit", npz, "--probe-no-wrap", "--width", "24", "--height", "16", "--aov-samples", "2",
                 "-o", png]) == 0
    from PIL import Image
    from firework_amd.yaml_io import load_scene
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(24).height(16).samples(2).use_bvh(True).camera(cam).seed(0)
    want = r.render_probe_lit(load_scene(yml), grid, sh, aov_samples=2)
    assert np.array_equal(np.asarray(Image.open(png).convert("RGB")).reshape(-1, 3), want.rgb8)


CPP = r"""
#include "firework.hpp"
#include <cstdio>
using namespace firework;
int main(int argc, char **argv) {      // probe_lit <sh.bin> <out.bin> <wrap>: cornell at 32 x 24, seed 5, 4 guide samples, a 2 x 2 x 2 grid
    Scene world = Scene::new_();
    MaterialIdx red = world.add_material(LambertianMat::with_color({0.65f, 0.05f, 0.05f}));
    MaterialIdx white = world.add_material(LambertianMat::with_color({0.73f, 0.73f, 0.73f}));
    MaterialIdx green = world.add_material(LambertianMat::with_color({0.12f, 0.45f, 0.15f}));
    MaterialIdx light = world.add_material(EmissiveMat::with_color({15.f, 15.f, 15.f}));
    world.add_object(RenderObject::new_(XZRect::new_(213.f, 343.f, 227.f, 332.f, 554.f, light)));
    world.add_object(RenderObject::new_(YZRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, green)).flip_normals());
    world.add_object(RenderObject::new_(YZRect::new_(0.f, 555.f, 0.f, 555.f, 0.f, red)));
    world.add_object(RenderObject::new_(XZRect::new_(0.f, 555.f, 0.f, 555.f, 0.f, white)));
    world.add_object(RenderObject::new_(XZRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, white)).flip_normals());
    world.add_object(RenderObject::new_(XYRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, white)).flip_normals());
    world.add_object(RenderObject::new_(Rect3d::with_size({165.f, 165.f, 165.f}, white)).rotate(Rotor3::from_rotation_xz(18.f * RADS_PER_DEG)).position(130.f, 0.f, 65.f));
    world.add_object(RenderObject::new_(Rect3d::with_size({165.f, 330.f, 165.f}, white)).rotate(Rotor3::from_rotation_xz(-15.f * RADS_PER_DEG)).position(265.f, 0.f, 295.f));
    CameraSettings camera = CameraSettings::default_().cam_pos({278.f, 278.f, -800.f}).look_at({278.f, 278.f, 0.f}).field_of_view(40.f);
    Renderer renderer = Renderer::default_().width(32).height(24).samples(4).camera(camera).seed(5);
    ProbeSet probes = ProbeSet::grid({100.f, 100.f, 100.f}, {450.f, 450.f, 450.f}, 2, 2, 2, 65);
    std::vector<float> sh(8 * 27);
    FILE *f = std::fopen(argv[1], "rb");
    if (argc < 4 || !f || std::fread(sh.data(), 4, sh.size(), f) != sh.size()) return 2;
    std::fclose(f);
    try {
        std::vector<Color> img = renderer.probe_lit(world, probes, sh, 4, argv[3][0] == '1');
        f = std::fopen(argv[2], "wb");
        for (const Color &c : img) { const uint8_t b[3] = {c.r, c.g, c.b}; std::fwrite(b, 1, 3, f); }
        std::fclose(f);
    } catch (const std::exception &e) { std::fprintf(stderr, "probe_lit failed: %s\n", e.what()); return 1; }
    return 0;
}
"""


def test_cpp_probe_lit_renders_the_same_bytes_as_the_python_host(tmp_path):
    """include/firework.hpp's Renderer::probe_lit (fw_render_aovs to the host, fw_probe_shade with host arrays) against
    Renderer.render_probe_lit (the records stay on the device): the same rgb8, with and without wrap"""
    (tmp_path / "t.cpp").write_text(CPP)
    lib_dir = os.path.join(ROOT, "firework_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.cpp"),
                           "-L", lib_dir, "-lfirework_hip", "-Wl,-rpath," + lib_dir])
    scene, r = scenes.cornell_box()
    r.width(32).height(24).samples(4).seed(5)
    probes = ProbeSet.grid((100.0, 100.0, 100.0), (450.0, 450.0, 450.0), (2, 2, 2), 65)
    sh, _sums = r.bake_probes(scene, probes, 1)
    sh.tofile(tmp_path / "sh.bin")
    for wrap in (True, False):
        subprocess.run([str(tmp_path / "t"), str(tmp_path / "sh.bin"), str(tmp_path / "out.bin"), "1" if wrap else "0"], check=True, timeout=120)
        got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(-1, 3)
        assert np.array_equal(got, r.render_probe_lit(scene, probes, sh, aov_samples=4, wrap=wrap).rgb8), wrap
