"""Every-emitter measurements (FW_FLAG_ALL_EMITTERS): device time and RMSE of the default estimator, bit 4 alone and bits
4 + 16 on cornell with its ceiling light as an emissive mesh of 2 x 16^2 triangles (512^2 @1024) and on one bright sphere among 100 dim
ones, each frame rendered twice and the second timed (FW_FLAG_TIME_KERNELS), RMSE of the linear image against ref_spp samples of bits 4 + 16
with another seed.  Equal-time RMSE is derived, not measured: RMSE x sqrt(device-time ratio).  Also the table's one-shot build for a
1 M-triangle emissive mesh (host wall time of the first 1-spp frame that asks for it, less that of a second).  Writes profiles/all_emitters.txt.

    python tools/all_emitters.py [--out profiles/all_emitters.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, scenes  # noqa: E402
from firework_amd.api import (CameraSettings, EmissiveMat, LambertianMat, Renderer, RenderObject, Scene, Sphere, TriangleMesh,  # noqa: E402
                              XZRect)

LS, PL, TIME = A.FW_FLAG_LIGHT_SAMPLING, A.FW_FLAG_LIGHT_SAMPLING | A.FW_FLAG_ALL_EMITTERS, A.FW_FLAG_TIME_KERNELS


def quad_mesh(x0, x1, z0, z1, n, material):
    xs, zs = np.linspace(x0, x1, n + 1), np.linspace(z0, z1, n + 1)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    verts = np.stack([X, np.zeros_like(X), Z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = (i * (n + 1) + j).ravel(), ((i + 1) * (n + 1) + j).ravel()
    idx = np.stack([a, b, b + 1, a, b + 1, a + 1], -1).ravel().astype(np.uint32)
    return TriangleMesh(verts, idx, material=material)


def mesh_cornell(w=512, h=512, spp=1024, n=16):
    scene, r = scenes.config("C2_cornell_box", w, h, spp)
    (l,) = _lib.selftest_lights(scene.to_desc())
    ro = scene.render_objects[l["obj"]]
    rect = ro.obj
    ro.obj = quad_mesh(rect.a_min, rect.a_max, rect.b_min, rect.b_max, n, rect.material)
    ro.position(0.0, float(rect.k), 0.0)
    return scene, r


def spheres(w=512, h=512, spp=256):
    scene = Scene.new()
    floor = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    bright = scene.add_material(EmissiveMat.with_color((40.0, 40.0, 40.0)))
    dim = scene.add_material(EmissiveMat.with_color((0.05, 0.05, 0.05)))
    scene.add_object(RenderObject.new(XZRect.new(-50, 50, -50, 50, 0, floor)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, bright)).position(0.0, 3.0, 0.0))
    rng = np.random.default_rng(1)
    for _ in range(100):
        x, z = rng.uniform(-20, 20, 2)
        scene.add_object(RenderObject.new(Sphere.new(0.3, dim)).position(float(x), float(rng.uniform(4, 12)), float(z)))
    cam = CameraSettings.default().cam_pos((0.0, 6.0, 12.0)).look_at((0.0, 0.0, 0.0)).field_of_view(50.0)
    return scene, Renderer.default().width(w).height(h).samples(spp).use_bvh(True).camera(cam)


CASES = {"mesh_cornell": (mesh_cornell, 4096), "spheres": (spheres, 4096)}


def frame(ds, r, flags, spp=None, seed=None):
    rr = Renderer.default()
    rr.settings = dict(r.settings)
    rr._camera = r._camera
    rr.settings["flags"] = flags
    if spp:
        rr.settings["samples"] = spp
    if seed is not None:
        rr.settings["seed"] = seed
    return ds.render(rr)


def measure(name):
    make, ref_spp = CASES[name]
    scene, r = make()
    ds = _lib.DeviceScene(scene.to_desc())
    ref = frame(ds, r, PL, spp=ref_spp, seed=12345).linear.astype(np.float64)
    assert np.isfinite(ref).all(), f"{name}: the reference has non-finite pixels"
    rows = []
    for label, fl in (("default", 0), ("bit 4", LS), ("bits 4+16", PL)):
        frame(ds, r, fl | TIME)
        res = frame(ds, r, fl | TIME)
        e = float(np.sqrt(np.mean((res.linear.astype(np.float64) - ref) ** 2)))
        rows.append((label, res.stats["ms_render"], res.stats["ms_extend"], res.stats["ms_shade"], e))
    s = r.settings
    return dict(name=name, size=f"{s['width']}x{s['height']}", spp=s["samples"], ref_spp=ref_spp, rows=rows)


def table_build(n_side=708):
    """a 2 x 708^2 = 1.0 M-triangle emissive mesh over a floor: the first 1-spp frame with bits 4+16 against a second"""
    scene = Scene.new()
    floor = scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    emit = scene.add_material(EmissiveMat.with_color((4.0, 4.0, 4.0)))
    scene.add_object(RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, floor)))
    scene.add_object(RenderObject.new(quad_mesh(-1, 1, -1, 1, n_side, emit)).position(0.0, 3.0, 0.0))
    cam = CameraSettings.default().cam_pos((0.0, 2.0, 8.0)).look_at((0.0, 1.0, 0.0)).field_of_view(45.0)
    r = Renderer.default().width(64).height(64).samples(1).use_bvh(True).camera(cam)
    ds = _lib.DeviceScene(scene.to_desc())
    frame(ds, r, LS)                                   # context, arena
    t0 = time.time(); frame(ds, r, PL); first = (time.time() - t0) * 1e3
    t0 = time.time(); frame(ds, r, PL); second = (time.time() - t0) * 1e3
    return 2 * n_side * n_side, first, second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "all_emitters.txt"))
    opt = ap.parse_args()
    lines = [__doc__.split("\n\n")[0], ""]
    lines.append(f"{'scene':13s} {'size':9s} {'spp':>5s}  {'estimator':10s} {'ms_render':>10s} {'ms_extend':>10s} {'ms_shade':>10s} {'RMSE':>10s}  ref_spp")
    summary = []
    for name in CASES:
        m = measure(name)
        for label, mr, me, ms, e in m["rows"]:
            lines.append(f"{name:13s} {m['size']:9s} {m['spp']:5d}  {label:10s} {mr:10.2f} {me:10.2f} {ms:10.2f} {e:10.5f}  {m['ref_spp']}")
            print(lines[-1]); sys.stdout.flush()
        (_, t0, _, _, e0), (_, t1, _, _, e1), (_, t2, _, _, e2) = m["rows"]
        summary.append((name, "bits 4+16 / default", t2 / t0, e2 / e0, e2 / e0 * np.sqrt(t2 / t0)))
        summary.append((name, "bits 4+16 / bit 4", t2 / t1, e2 / e1, e2 / e1 * np.sqrt(t2 / t1)))
    lines += ["", f"{'':13s} {'':20s} {'device time':>12s} {'RMSE at equal spp':>18s} {'RMSE at equal time (derived)':>30s}"]
    for name, what, tr, er, eq in summary:
        lines.append(f"{name:13s} {what:20s} {tr:11.2f}x {er:17.2f}x {eq:29.2f}x")
    n, first, second = table_build()
    lines += ["", f"table build, {n} emissive triangles: first 1-spp frame {first:.1f} ms host, second {second:.1f} ms: about {first - second:.1f} ms for the table"]
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-8:]))


if __name__ == "__main__":
    main()
