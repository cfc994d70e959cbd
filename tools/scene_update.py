"""Scene-update measurements: fw_scene_create (+ fw_scene_destroy) of a moved scene against fw_scene_update of a resident
one to the same placements, alternated, synchronised host wall time (the device is drained after each call, so the asynchronous upload
counts).  The descriptions are prepared before the timed calls: both sides time the library call alone.  Then a per-frame loop: update +
a 1-spp 512x512 render against create + the same render + destroy.  Prints one JSON line per case and a median table.

    python tools/scene_update.py [--case grid1m,hdri,part2,spheres200k] [--reps 7] [--frames 5] [--out profiles/scene_update.txt]

    grid1m       one sphere moving in front of the 1 M-triangle grid (tools/big_mesh.py's grid_mesh(709))
    hdri         hdri_test (4096x2048 HDR map) with a sphere moved
    part2        part2_all with every object jittered
    spheres200k  200 000 spheres, every one moved (the TLAS trees are built on the device)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from firework_amd import _lib, scenes  # noqa: E402
from firework_amd.api import (CameraSettings, LambertianMat, Renderer, RenderObject, Scene, SkyEnv, Sphere, TriangleMesh,  # noqa: E402
                              XZRect)


def grid_mesh(n, material):
    xs = np.linspace(-4, 4, n, dtype=np.float32)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = (0.4 * np.sin(2 * X) * np.cos(2 * Z)).astype(np.float32)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1); b = a + 1; c = a + n; d = c + 1
    idx = np.stack([a, b, c, b, d, c], -1).reshape(-1).astype(np.uint32)
    return TriangleMesh.new(verts, idx, None, None, material)


def frame(r):
    return r.width(512).height(512).samples(1)


def case_grid1m():
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.7, 0.6, 0.5)))
    sc.add_object(RenderObject.new(grid_mesh(709, m)).position(0.0, 1.0, 0.0))
    sc.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 20.0, -0.5, m)))
    ball = sc.add_object(RenderObject.new(Sphere.new(0.8, m)).position(0.0, 2.5, -2.0))
    sc.set_environment(SkyEnv.default())
    cam = CameraSettings.default().cam_pos((0.0, 6.0, -12.0)).look_at((0.0, 1.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().use_bvh(True).camera(cam)

    def move(k):
        sc.render_objects[ball].position(-2.0 + 0.5 * (k % 8), 2.5, -2.0)
    return sc, frame(r), move


def case_hdri():
    sc, r = scenes.config("C4a_hdri_test", 512, 512, 1)

    def move(k):
        sc.render_objects[1].position(-4.0 + 0.25 * (k % 8), 1.0, 0.5 * (k % 3))
    return sc, frame(r), move


def case_part2():
    sc, r = scenes.config("C5_part2_all", 512, 512, 1)
    home = [ro._position.copy() for ro in sc.render_objects]

    def move(k):
        rng = np.random.default_rng(k)
        for ro, p in zip(sc.render_objects, home):
            ro.position_vec(p + rng.uniform(-0.05, 0.05, 3).astype(np.float32))
    return sc, frame(r), move


def case_spheres200k():
    n = 200_000
    rng = np.random.default_rng(1)
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.6, 0.5, 0.4)))
    ball = Sphere.new(0.15, m)
    home = rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32)
    for p in home:
        sc.add_object(RenderObject.new(ball).position_vec(p))
    sc.set_environment(SkyEnv.default())
    cam = CameraSettings.default().cam_pos((0.0, 20.0, -120.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().use_bvh(True).camera(cam)

    def move(k):
        off = np.random.default_rng(100 + k).uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
        for ro, p in zip(sc.render_objects, home + off):
            ro._position = p
    return sc, frame(r), move


CASES = {"grid1m": case_grid1m, "hdri": case_hdri, "part2": case_part2, "spheres200k": case_spheres200k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    _lib.init(0)
    lib = _lib.load()
    sync = torch.cuda.synchronize
    rows = []
    for name in a.case.split(","):
        sc, r, move = CASES[name]()
        base = sc.to_desc()
        descs = []
        t_pl = []
        for k in range(2 * a.reps + a.frames + 1):       # every placement the runs ask for, converted before the timed calls
            move(k)
            t0 = time.perf_counter()
            descs.append(base.placements(sc))
            t_pl.append(time.perf_counter() - t0)
        ds = _lib.DeviceScene(base)
        ds.render(r)
        sync()

        def create(d):
            h = C.c_void_p()
            t0 = time.perf_counter()
            _lib._check(lib, lib.fw_scene_create(d.ptr(), 0, C.byref(h)))
            lib.fw_scene_destroy(h)
            sync()
            return time.perf_counter() - t0

        def update(d):
            t0 = time.perf_counter()
            _lib._check(lib, lib.fw_scene_update(ds.handle, d.ptr()))
            sync()
            return time.perf_counter() - t0
        create(descs[0]); update(descs[1])                   # warm-up of each
        tc, tu = [], []
        for k in range(a.reps):
            tc.append(create(descs[2 + 2 * k]))
            tu.append(update(descs[3 + 2 * k]))
        # per-frame loops: update + render against create + render + destroy, the same placements
        fu, fc = [], []
        for k in range(a.frames):
            d = descs[2 * a.reps + 1 + k]
            t0 = time.perf_counter()
            _lib._check(lib, lib.fw_scene_update(ds.handle, d.ptr()))
            ds.render(r)
            fu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            fresh = _lib.DeviceScene(d)
            fresh.render(r)
            fresh.close()
            sync()
            fc.append(time.perf_counter() - t0)
        ds.close()
        row = dict(case=name, objects=base.desc.n_objects, reps=a.reps, frames=a.frames,
                   create_ms=1e3 * statistics.median(tc), update_ms=1e3 * statistics.median(tu),
                   frame_create_ms=1e3 * statistics.median(fc), frame_update_ms=1e3 * statistics.median(fu),
                   placements_py_ms=1e3 * statistics.median(t_pl), create_all_ms=[round(1e3 * x, 2) for x in tc],
                   update_all_ms=[round(1e3 * x, 2) for x in tu])
        row["ratio"] = row["create_ms"] / row["update_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    lines = ["case          objects   create+destroy ms   update ms   ratio   frame: create+render ms   update+render ms   (Python placements() ms)"]
    for w in rows:
        lines.append(f"{w['case']:<13} {w['objects']:>7}   {w['create_ms']:>17.2f}   {w['update_ms']:>9.3f}   {w['ratio']:>5.0f}   "
                     f"{w['frame_create_ms']:>23.2f}   {w['frame_update_ms']:>16.2f}   {w['placements_py_ms']:>8.2f}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(w) for w in rows) + "\n")


if __name__ == "__main__":
    main()
