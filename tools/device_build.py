"""Scene creation time, host tree builds against device tree builds (BUILD=host|device), for grid meshes as tools/big_mesh.py makes them.
Each setting runs in a child process of its own (FIREWORK_BUILD_THREADS is read once per process), after one warm-up creation; the median
of three creations is reported, with the FIREWORK_TRACE lines of the last one.  Usage: python tools/device_build.py [n,n,...] (grid sides;
default 101,317,709,1415: 20 k, 200 k, 1 M and 4 M triangles)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_scene(n):
    import numpy as np
    from firework_amd.api import LambertianMat, RenderObject, Scene, SkyEnv, TriangleMesh, XZRect
    xs = np.linspace(-4, 4, n, dtype=np.float32)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = (0.4 * np.sin(2 * X) * np.cos(2 * Z)).astype(np.float32)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1); b = a + 1; c = a + n; d = c + 1
    idx = np.stack([a, b, c, b, d, c], -1).reshape(-1).astype(np.uint32)
    sc = Scene.new()
    m = sc.add_material(LambertianMat.with_color((0.7, 0.6, 0.5)))
    sc.add_object(RenderObject.new(TriangleMesh.new(verts, idx, None, None, m)).position(0.0, 1.0, 0.0))
    sc.add_object(RenderObject.new(XZRect.new(-20.0, 20.0, -20.0, 20.0, -0.5, m)))
    sc.set_environment(SkyEnv.default())
    return sc, int(idx.size // 3)


def child(n):
    from firework_amd import _lib
    from firework_amd import _abi as A
    _lib.init(0, A.FW_INIT_NO_ARENA)
    sc, tris = grid_scene(n)
    desc = sc.to_desc()
    _lib.DeviceScene(grid_scene(11)[0].to_desc()).close()      # warm-up: the device build's first launches
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ds = _lib.DeviceScene(desc)
        times.append((time.perf_counter() - t0) * 1e3)
        ds.close()
    times.sort()
    print(json.dumps(dict(tris=tris, create_ms=round(times[1], 2), all_ms=[round(t, 2) for t in times])))


def main():
    sides = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "101,317,709,1415").split(",")]
    settings = [("host", None), ("host", "1"), ("device", None)]
    for n in sides:
        for build, threads in settings:
            env = dict(os.environ, FIREWORK_BUILD=build, FIREWORK_TRACE="1")
            env.pop("FIREWORK_BUILD_THREADS", None)
            if threads:
                env["FIREWORK_BUILD_THREADS"] = threads
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                print(f"side {n} BUILD={build} threads={threads or 'default'}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                sys.exit(1)
            r = json.loads(p.stdout.strip().splitlines()[-1])
            trace = [ln for ln in p.stderr.splitlines() if "scene_create" in ln][-3:]
            print(json.dumps(dict(side=n, build=build, threads=threads or "default", **r)), flush=True)
            for ln in trace:
                print("   ", ln, flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
