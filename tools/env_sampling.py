"""Environment sampling measurements (FW_FLAG_ENV_SAMPLING): device time and RMSE of the default estimator against bit 8
(C4a) and against bits 4 + 8 (an HDR coverage scene), each frame rendered twice and the second timed (FW_FLAG_TIME_KERNELS), RMSE of the
linear image against a reference of ref_spp samples of the sampled estimator with another seed.  Equal-time RMSE is derived, not
measured: RMSE x sqrt(device-time ratio).  Writes profiles/env_sampling.txt.

    python tools/env_sampling.py [--out profiles/env_sampling.txt] [--kernel-stats NAME=rocprofv3_kernel_stats.csv ...]
    python tools/env_sampling.py --one FLAGS [--scene c4a|coverage]    one frame (for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, scenes  # noqa: E402
from firework_amd.api import (CameraSettings, ConstantTexture, DielectricMat, EmissiveMat, HdrEnvironment, LambertianMat, MetalMat,  # noqa: E402
                              Renderer, RenderObject, Scene, Sphere, XYRect, XZRect)

ENV, LS, TIME = A.FW_FLAG_ENV_SAMPLING, A.FW_FLAG_LIGHT_SAMPLING, A.FW_FLAG_TIME_KERNELS


def coverage():
    """the HDR coverage scene of tests/test_gpu_env_sampling.py over synthetic_hdr: a diffuse floor and wall, metal, glass, an emitter
    sphere and a medium"""
    scene = Scene.new()
    scene.set_environment(HdrEnvironment(scenes.synthetic_hdr()))
    floor = scene.add_material(LambertianMat.with_color((0.6, 0.6, 0.6)))
    wall = scene.add_material(LambertianMat.with_color((0.3, 0.5, 0.7)))
    emit = scene.add_material(EmissiveMat.with_color((6.0, 5.0, 4.0)))
    metal = scene.add_material(MetalMat.new((0.9, 0.9, 0.9), 0.05))
    glass = scene.add_material(DielectricMat.new(1.5))
    scene.add_object(RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, floor)))
    scene.add_object(RenderObject.new(XYRect.new(-10, 10, 0, 3, -4, wall)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, emit)).position(0.0, 3.0, 1.0))
    scene.add_object(RenderObject.new(Sphere.new(0.8, metal)).position(-1.2, 0.8, 0.5))
    scene.add_object(RenderObject.new(Sphere.new(0.8, glass)).position(1.3, 0.8, 0.8))
    scene.add_volume(RenderObject.new(Sphere.new(0.7, floor)).position(0.0, 0.7, -1.5), 0.8, ConstantTexture.new((0.8, 0.8, 0.8)))
    cam = CameraSettings.default().cam_pos((0.0, 3.0, 9.0)).look_at((0.0, 1.0, 0.0)).field_of_view(45.0)
    return scene, Renderer.default().width(512).height(512).samples(256).use_bvh(True).camera(cam)


CASES = {"c4a": (lambda: scenes.config("C4a_hdri_test", 1024, 1024, 512), ENV, 4096),
         "coverage": (coverage, ENV | LS, 4096)}


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
    make, flags, ref_spp = CASES[name]
    scene, r = make()
    ds = _lib.DeviceScene(scene.to_desc())
    t0 = time.time()
    frame(ds, r, flags, spp=1)                      # the table's build (the first render that asks for it)
    first_ms = (time.time() - t0) * 1e3
    ref = frame(ds, r, flags, spp=ref_spp, seed=12345).linear.astype(np.float64)
    rows = []
    for label, fl in (("default", 0), ("sampled", flags)):
        frame(ds, r, fl | TIME)
        res = frame(ds, r, fl | TIME)
        e = float(np.sqrt(np.mean((res.linear.astype(np.float64) - ref) ** 2)))
        rows.append((label, res.stats["ms_render"], res.stats["ms_extend"], res.stats["ms_shade"], e))
    s = r.settings
    return dict(name=name, size=f"{s['width']}x{s['height']}", spp=s["samples"], flags=flags, ref_spp=ref_spp, rows=rows,
                first_ms=first_ms)


def kernel_stats(path):
    """rocprofv3 --stats kernel_stats.csv -> [(kernel, calls, total ms, mean us)] of the kernels this feature added or uses"""
    out = []
    with open(path) as f:
        for row in csv.DictReader(f):
            n = row.get("Name", "")
            if any(k in n for k in ("k_shade_env", "k_shadow_resolve", "k_shade_ls", "k_shade<", "k_env_", "k_extend")):
                out.append((n.split("(")[0][:60], int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6, float(row["AverageNs"]) / 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_sampling.txt"))
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="NAME=CSV")
    ap.add_argument("--one", type=int, default=None, metavar="FLAGS")
    ap.add_argument("--scene", default="c4a", choices=sorted(CASES))
    opt = ap.parse_args()
    if opt.one is not None:
        scene, r = CASES[opt.scene][0]()
        ds = _lib.DeviceScene(scene.to_desc())
        res = frame(ds, r, opt.one)
        print(f"{opt.scene} flags={opt.one} ms_render={res.stats['ms_render']:.2f}")
        return
    lines = [__doc__.split("\n\n")[0], ""]
    lines.append(f"{'scene':10s} {'size':10s} {'spp':>5s}  {'estimator':9s} {'ms_render':>10s} {'ms_extend':>10s} {'ms_shade':>10s} {'RMSE':>10s}  ref_spp")
    summary = []
    for name in CASES:
        m = measure(name)
        for label, mr, me, ms, e in m["rows"]:
            est = "default" if label == "default" else ("bit 8" if m["flags"] == ENV else "bits 4+8")
            lines.append(f"{name:10s} {m['size']:10s} {m['spp']:5d}  {est:9s} {mr:10.2f} {me:10.2f} {ms:10.2f} {e:10.5f}  {m['ref_spp']}")
        (_, t0, _, _, e0), (_, t1, _, _, e1) = m["rows"]
        summary.append((name, t1 / t0, e1 / e0, e1 / e0 * np.sqrt(t1 / t0), m["first_ms"]))
        print(lines[-2]); print(lines[-1]); sys.stdout.flush()
    lines += ["", f"{'':10s} {'device time':>12s} {'RMSE at equal spp':>18s} {'RMSE at equal time (derived)':>30s} {'first 1-spp frame, host ms (table build incl.)':>48s}"]
    for name, tr, er, eq, fm in summary:
        lines.append(f"{name:10s} {tr:11.2f}x {er:17.2f}x {eq:29.2f}x {fm:48.1f}")
    for spec in opt.kernel_stats:
        label, path = spec.split("=", 1)
        lines += ["", f"rocprofv3 --kernel-trace --stats, {label}: kernel, calls, total ms, mean us"]
        for n, c, tot, avg in kernel_stats(path):
            lines.append(f"  {n:60s} {c:6d} {tot:10.3f} {avg:10.2f}")
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-12:]))


if __name__ == "__main__":
    main()
