"""Probe-visibility measurements (fw_bake_probe_depth, fw_probe_irradiance_vis); the results are kept in
profiles/probe_depth.txt.  Nothing here is a gate.

    python tools/probe_depth.py bake [--reps N]     cornell, a 16 x 16 x 16 grid, D = 256, R = 8, k = 6, one round: the whole depth bake
                                                    (fw_stats.ms_render, first launch to last, and ms_wall) and, under
                                                    FW_FLAG_TIME_KERNELS, its parts — k_probe_rays (ms_raygen), the walks (ms_extend) and
                                                    k_probe_depth (ms_accumulate: device events around the launch) — one warm-up call,
                                                    then medians of N (default 5).  Beside it fw_bake_probes at S = 1 on the same set.
    python tools/probe_depth.py lookup [--calls N]  k_probe_irradiance with the depth maps against without, on the same 1920 x 1080 buffer of
                                                    fw_render_aovs records (cornell), in place at stride 12, alternated in one process:
                                                    3 warm-up calls each, then N (default 20) calls each timed by device events around the
                                                    call (host call and stream drain included); medians.
    python tools/probe_depth.py rmse                two rooms divided by a wall, the lamp in one: Renderer.render_probe_lit with and without
                                                    the depth moments against a converged path-traced frame (every surface is Lambertian, so
                                                    the frame is diffuse light only), RMSE over the pixels of coverage 1 that do not see the
                                                    lamp — all of them, the floor's and the wall's — for a view of the dark room and one of the lit room.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

W, H, GRID, D, RES, K = 1920, 1080, (16, 16, 16), 256, 8, 6
WARMUP = 3


def _cornell_set():
    return api.ProbeSet.grid((40.0, 40.0, 40.0), (515.0, 515.0, 515.0), GRID, D).seed(1), api.ProbeDepth(RES, K, 823.0)     # r_max: the grid's diagonal


def bake(reps):
    scene, r = scenes.config("C2_cornell_box", 64, 64, 1)
    r.seed(3)
    probes, pd = _cornell_set()
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        r.bake_probe_depth(ds, probes, pd, 1)                                            # warm-up: arena growth, first launches
        plain, timed = [], []
        for _ in range(reps):
            r.settings["flags"] &= ~A.FW_FLAG_TIME_KERNELS
            r.bake_probe_depth(ds, probes, pd, 1)
            plain.append(dict(r.probe_depth_stats))
            r.settings["flags"] |= A.FW_FLAG_TIME_KERNELS
            r.bake_probe_depth(ds, probes, pd, 1)
            timed.append(dict(r.probe_depth_stats))
        r.settings["flags"] &= ~A.FW_FLAG_TIME_KERNELS
        r.bake_probes(ds, probes, 1)
        sh_ms = []
        for _ in range(reps):
            r.bake_probes(ds, probes, 1)
            sh_ms.append(r.probe_stats["ms_render"])
    finally:
        ds.close()
    med = lambda rows, key: float(np.median([x[key] for x in rows]))      # noqa: E731
    n = probes.n_probes
    print(f"workload: cornell, {GRID[0]} x {GRID[1]} x {GRID[2]} = {n} probes, D = {D}, R = {RES}, k = {K}, one round = {n * D} rays, "
          f"{n * D * RES * RES} (ray, texel) pairs; {reps} repetitions after one warm-up, medians")
    print(f"fw_bake_probe_depth            ms_render {med(plain, 'ms_render'):8.3f}  ms_wall {med(plain, 'ms_wall'):8.3f}  "
          f"(all ms_render: {' '.join('%.3f' % x['ms_render'] for x in plain)})")
    print(f"  under FW_FLAG_TIME_KERNELS   ms_render {med(timed, 'ms_render'):8.3f}  k_probe_rays {med(timed, 'ms_raygen'):7.3f}  "
          f"walks {med(timed, 'ms_extend'):7.3f}  k_probe_depth {med(timed, 'ms_accumulate'):7.3f}  "
          f"(all k_probe_depth: {' '.join('%.3f' % x['ms_accumulate'] for x in timed)})")
    t = med(timed, "ms_accumulate")
    print(f"  k_probe_depth: {n * D * RES * RES * 15 / t / 1e6:.1f} Gflop/s of float64 at 15 operations per (ray, texel) pair; "
          f"{100.0 * t / med(timed, 'ms_render'):.1f} % of the timed bake")
    print(f"fw_bake_probes, S = 1, same set  ms_render {float(np.median(sh_ms)):8.3f}")


def lookup(calls):
    import torch
    scene, r = scenes.config("C2_cornell_box", W, H, 4)
    r.seed(3)
    probes, pd = _cornell_set()
    grid = api.ProbeGrid.of(probes, True)
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)
    try:
        moments, _sums = r.bake_probe_depth(ds, probes, pd, 1)
        sh, _s = r.bake_probes(ds, probes, 1)
        aov = ds.aovs(r, 8, out=torch.empty((W * H, 12), dtype=torch.float32, device=dev))
    finally:
        ds.close()
    d_sh, d_mom = torch.from_numpy(sh).to(dev), torch.from_numpy(moments).to(dev)
    out = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    plain, vis = "k_probe_irradiance<false, false>", "k_probe_irradiance<false, true>"      # <PLACED, DEPTH>
    fns = {plain: lambda: _lib.probe_irradiance(grid, d_sh, aov[:, 8:11], aov[:, 4:7], out=out),
           vis: lambda: _lib.probe_irradiance_vis(grid, d_sh, pd, d_mom, aov[:, 8:11], aov[:, 4:7], 0.0, out=out)}
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(calls):
        for name, fn in fns.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    print(f"{W * H} points (cornell's fw_render_aovs records in place, stride 12), {grid.n_probes} probes, R = {RES}; alternated, {calls} calls each after "
          f"{WARMUP}, device events around the calls (host call and stream drain included)")
    for name, t in ms.items():
        print(f"{name:34s} median {np.median(t):7.3f} ms  min {min(t):7.3f}  max {max(t):7.3f}")
    print(f"ratio vis / plain {np.median(ms[vis]) / np.median(ms[plain]):.2f}")


def _rooms():
    from firework_amd.api import ColorEnv, EmissiveMat, LambertianMat, RenderObject, Scene, Sphere, XZRect, YZRect
    scene = Scene.new()
    white = scene.add_material(LambertianMat.with_color((0.7, 0.7, 0.7)))
    lamp = scene.add_material(EmissiveMat.with_color((20.0, 16.0, 12.0)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, lamp)).position(-2.0, 1.0, 0.0))
    scene.add_object(RenderObject.new(YZRect.new(-1000.0, 1000.0, -1000.0, 1000.0, 1.0, white)))
    scene.add_object(RenderObject.new(XZRect.new(-1000.0, 1000.0, -1000.0, 1000.0, -1.0, white)))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    return scene


def rmse():
    scene = _rooms()
    probes = api.ProbeSet.grid((-4.0, -0.5, -3.0), (6.0, 2.0, 3.0), (6, 2, 3), 256).seed(1)
    pd = api.ProbeDepth(RES, K, 12.0)
    w, h = 160, 90
    views = dict(dark=((6.0, 1.5, 5.0), (2.5, -0.5, 0.0)), lit=((-1.0, 1.5, 6.0), (-1.0, -0.5, 0.0)))
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        baker = api.Renderer.default().samples(64).use_bvh(True).seed(2)
        sh, _s = baker.bake_probes(ds, probes, 4)
        moments, _d = baker.bake_probe_depth(ds, probes, pd, 4)
        print(f"two rooms: wall at x = 1, lamp at (-2, 1, 0); {probes.n_probes} probes (6 x 2 x 3), D = 256, 4 rounds of 64 samples; R = {RES}, k = {K}; "
              f"{w} x {h}, reference 4096 samples per pixel")
        for name, (pos, at) in views.items():
            cam = api.CameraSettings.default().cam_pos(pos).look_at(at).field_of_view(50.0)
            r = api.Renderer.default().width(w).height(h).samples(4096).use_bvh(True).seed(7).camera(cam).gamma(1.0)
            ref = ds.render(r).linear.astype(np.float64)
            rec = ds.aovs(r, 8)
            keep = (rec[:, 3] == 1.0) & (rec[:, 0:3].max(axis=1) <= 1.0)                  # whole coverage, not the lamp (its record holds its emission)
            parts = (("all", keep), ("floor", keep & (np.abs(rec[:, 5]) > 0.9)), ("wall", keep & (np.abs(rec[:, 4]) > 0.9)))
            print(f"  view of the {name} room: " + ", ".join(f"{what} {int(m.sum())} pixels, reference mean {ref[m].mean():.4e}" for what, m in parts))
            for label, kw in (("wrap alone", {}), ("with visibility", dict(depth=pd, moments=moments)),
                              ("with visibility, bias 0.1", dict(depth=pd, moments=moments, normal_bias=0.1)),
                              ("with visibility, bias 0.5", dict(depth=pd, moments=moments, normal_bias=0.5))):
                lit = r.render_probe_lit(ds, probes, sh, aov_samples=8, **kw).linear.astype(np.float64)
                print(f"    {label:26s} " + "  ".join(f"{what}: RMSE {float(np.sqrt(np.mean((lit[m] - ref[m]) ** 2))):.4e} mean {lit[m].mean():.4e}"
                                                      for what, m in parts))
    finally:
        ds.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("bake", "lookup", "rmse"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    opt = ap.parse_args()
    if opt.mode == "bake":
        bake(opt.reps)
    elif opt.mode == "lookup":
        lookup(opt.calls)
    else:
        rmse()


if __name__ == "__main__":
    main()
