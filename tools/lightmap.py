"""Lightmap-baker measurements (fw_lightmap_*, fw_bake_lightmap); the results are kept in profiles/lightmap.txt.
Nothing here is a gate.  The workload: cornell, a 128 x 128 lightmap of a quad on the floor (16 384 covered texels) x D = 64 directions
= 1 048 576 texel-directions x S = 16 samples x 1 round, 2 dilation passes.

    python tools/lightmap.py wall [--reps N]      Renderer.bake_lightmap against the host path it replaces — the numpy statements
                                                  Lightmap.texels / .rays, fw_render_rays with host arrays, api.lightmap_reduce and
                                                  api.lightmap_dilate — alternated, medians of N (default 5): wall time (host clock; both
                                                  paths end with the irradiance on the host) and the summed device time (fw_stats.ms_render).
    python tools/lightmap.py kernel [--calls N]   the public calls alone on device tensors of the workload's size, beside a device-to-device
                                                  copy of 1 GiB: time per call by device events (host call, uploads and stream drain
                                                  included).  The kernels' own time comes only from a run under the profiler, alone:
                                                  rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/lightmap.py kernel
    python tools/lightmap.py trace DIR [--calls N] that run's *_kernel_trace.csv, read back: the new kernels' dispatches, medians, as bytes
                                                  over time against the 1 GiB copies' own kernel time in the same trace.
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _lib, api, scenes  # noqa: E402

W = H = 128
D, S, ROUNDS, DILATE = 64, 16, 1, 2
WARMUP = 3


def _lightmap():
    x0, z0, x1, z1 = 40.0, 60.0, 520.0, 500.0
    mesh = api.TriangleMesh([[x0, 0.0, z1], [x1, 0.0, z1], [x1, 0.0, z0], [x0, 0.0, z0]], [0, 1, 2, 0, 2, 3], [[0.0, 1.0, 0.0]] * 4,
                            [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], 0)
    return api.Lightmap(mesh, W, H, D).seed(1).bias(0.01)


def wall(reps):
    scene, r = scenes.config("C2_cornell_box", 8, 8, S)
    r.use_bvh(False).seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    s = r.settings

    def device_path():
        irr, _sums = r.bake_lightmap(ds, _lightmap(), ROUNDS, DILATE)
        return irr, r.lightmap_stats["ms_render"]

    def host_path():
        lm = _lightmap()                                  # (a fresh one: the statement's rasterisation is part of the path)
        own = lm.texels()[1]
        ids = lm.covered().astype(np.int64)
        sums = np.zeros((W * H, 3))
        ms = 0.0
        for rnd in range(ROUNDS):
            rays = lm.rays(rnd)
            res = ds.render_rays(rays, S, 0, None, seed=s["seed"] + rnd, use_bvh=s["use_bvh"], paths_per_batch=s["paths_per_batch"], flags=s["flags"])
            ms += res.stats["ms_render"]
            sums[ids] += api.lightmap_reduce(res.accum, S, D)
        irr = np.zeros((H, W, 4), np.float32)
        cov = (own != api.LIGHTMAP_NO_OWNER).reshape(H, W)
        irr[cov, :3] = (sums.reshape(H, W, 3)[cov] / ROUNDS).astype(np.float32)
        irr[cov, 3] = 1.0
        return api.lightmap_dilate(irr, DILATE), ms

    try:
        host_path(), device_path()                      # warm-up: arena growth, first launches
        t = dict(host=[], device=[])
        dev_ms = dict(host=[], device=[])
        out = {}
        for _ in range(reps):
            for name, fn in (("host", host_path), ("device", device_path)):
                t0 = time.perf_counter()
                out[name], ms = fn()
                t[name].append(time.perf_counter() - t0)
                dev_ms[name].append(ms)
    finally:
        ds.close()
    print(f"workload: cornell, {W} x {H} texels x {D} directions x {S} samples x {ROUNDS} round(s), {DILATE} dilation passes, {reps} alternated repetitions")
    for name in ("host", "device"):
        print(f"{name:7s} wall median {np.median(t[name]) * 1e3:9.1f} ms  (all: {' '.join(f'{x * 1e3:.1f}' for x in t[name])})   "
              f"device time median {np.median(dev_ms[name]):8.1f} ms")
    print(f"wall ratio host / device {np.median(t['host']) / np.median(t['device']):.2f}")
    print(f"largest |irradiance_host - irradiance_device| {float(np.abs(out['host'].astype(np.float64) - out['device']).max()):.3e} "
          f"(largest irradiance {float(np.abs(out['device'][..., :3]).max()):.3e}; the rays differ at most by float32 neighbours)")


def kernel(calls):
    import torch
    dev = torch.device("cuda", 0)
    lm = _lightmap()
    n = W * H
    rays = torch.empty((n * D, 6), dtype=torch.float32, device=dev)
    accum = torch.rand((n * D, 4), dtype=torch.float32, device=dev)
    sums = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    img = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    img[::3, ::3] = 1.0
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(calls):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / calls

    t_copy = timed(lambda: b.copy_(a))
    t_tex = timed(lambda: _lib.lightmap_texels(lm, on_device=True))
    t_rays = timed(lambda: _lib.lightmap_rays(lm, 1, out=rays))
    t_red = timed(lambda: _lib.lightmap_reduce(accum, S, D, sums, texel_ids=ids))
    t_dil = timed(lambda: _lib.lightmap_dilate(img, 2))
    print(f"{n} texels x {D} directions, {calls} calls after {WARMUP} (device events around the calls: host call, uploads, the host pass over "
          f"the owner map and stream drain included)")
    print(f"copy 1 GiB d2d        {t_copy:8.3f} ms/call  {2 * (1 << 30) / t_copy / 1e6:8.1f} GB/s (read + write)")
    print(f"fw_lightmap_texels    {t_tex:8.3f} ms/call")
    print(f"fw_lightmap_rays      {t_rays:8.3f} ms/call  (rasterises first)  {n * D * 24 / t_rays / 1e6:8.1f} GB/s of 24 B/entry")
    print(f"fw_lightmap_reduce    {t_red:8.3f} ms/call  {n * D * 16 / t_red / 1e6:8.1f} GB/s of 16 B/entry")
    print(f"fw_lightmap_dilate x2 {t_dil:8.3f} ms/call")


def trace(path, calls):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {path}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = W * H

    def durations(name):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if name in r["Kernel_Name"]]

    big = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows
           if "k_lm_" not in r["Kernel_Name"] and int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) > 100000]
    if big:
        us = float(np.median(big))
        print(f"1 GiB copy kernels   median {us:9.1f} us over {len(big)} dispatches  {2 * (1 << 30) / us / 1e3:8.1f} GB/s (read + write)")
    # bytes per dispatch: cover — the owner map's atomics (4 B per covered texel, read-modify-write) and the mesh; texels — owner in, 32 B
    # record out; rays — 24 B per entry out, 36 B per texel in; reduce — 16 B per entry in, 4 + 2 x 12 B per texel; dilate — 16 B in (+ up
    # to 8 neighbours, cached) and 16 B out per texel
    for name, bytes_ in (("k_lm_cover", n * 8), ("k_lm_texels", n * 36), ("k_lm_rays", n * D * 24 + n * 36), ("k_lm_reduce", n * D * 16 + n * 28),
                         ("k_lm_dilate", n * 32), ("k_lm_resolve", n * 36)):
        d = durations(name)
        if not d:
            print(f"{name}: no dispatch in the trace")
            continue
        us = float(np.median(d))
        print(f"{name:14s} median {us:9.1f} us over {len(d)} dispatches  {bytes_ / us / 1e3:8.1f} GB/s of {bytes_ / 1e6:.2f} MB")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("wall", "kernel", "trace"))
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    opt = ap.parse_args()
    if opt.mode == "wall":
        wall(opt.reps)
    elif opt.mode == "kernel":
        kernel(opt.calls)
    else:
        trace(opt.dir or ".", opt.calls)


if __name__ == "__main__":
    main()
