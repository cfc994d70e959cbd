"""Probe-lookup measurements (fw_probe_irradiance, fw_probe_shade, Renderer.render_probe_lit); the results are kept in
profiles/probe_lookup.txt.  Nothing here is a gate.  The workload: cornell at 1920 x 1080, a 16 x 16 x 16 grid baked once (D = 64, S = 4).

    python tools/probe_lookup.py wall [--reps N]      Renderer.render_probe_lit against the host path it replaces — fw_render_aovs to the
                                                      host, api.probe_lookup and api.probe_shade_ref in numpy — alternated, medians of N
                                                      (default 5) wall times (host clock; both paths end with the linear frame on the
                                                      host), and the device time of each part of the device path: fw_render_aovs
                                                      (fw_stats.ms_render) and fw_probe_shade (device events around the call).  Also the
                                                      largest difference between the two paths' frames.
    python tools/probe_lookup.py kernel [--calls N]   k_probe_irradiance (on the records in place, stride 12) and k_probe_shade alone on
                                                      device tensors of the workload's size, beside a device-to-device copy of 1 GiB: time
                                                      per call by device events (host call and stream drain included).  The kernels' own
                                                      time comes only from a run under the profiler, alone:
                                                      rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/probe_lookup.py kernel
    python tools/probe_lookup.py trace DIR [--calls N] that run's *_kernel_trace.csv, read back: the two kernels' dispatches (3 warm-up
                                                      calls then N), medians of the N, as bytes of their own streams over time —
                                                      k_probe_irradiance 24 B + 12 B per point, k_probe_shade 48 B + 27 B per pixel —
                                                      against the 1 GiB copies' own kernel time in the same trace.
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

W, H, GRID, AOV_SAMPLES = 1920, 1080, (16, 16, 16), 8
WARMUP = 3


def _baked(ds, r):
    probes = api.ProbeSet.grid((40.0, 40.0, 40.0), (515.0, 515.0, 515.0), GRID, 64).seed(1)
    sh, _sums = r.bake_probes(ds, probes, 1)
    return probes, sh


def wall(reps):
    import torch
    scene, r = scenes.config("C2_cornell_box", W, H, 4)
    r.seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)

    def host_path():
        rec = ds.aovs(r, AOV_SAMPLES)
        return api.probe_shade_ref(probes, sh, rec)

    def device_path():
        return r.render_probe_lit(ds, probes, sh, AOV_SAMPLES).linear

    try:
        probes, sh = _baked(ds, r)
        host_path(), device_path()                      # warm-up: arena growth, first launches
        t = dict(host=[], device=[])
        out = {}
        for _ in range(reps):
            for name, fn in (("host", host_path), ("device", device_path)):
                t0 = time.perf_counter()
                out[name] = fn()
                t[name].append(time.perf_counter() - t0)
        # the device path's parts
        aov = torch.empty((W * H, 12), dtype=torch.float32, device=dev)
        d_sh = torch.from_numpy(sh).to(dev)
        ms_aov, ms_shade = [], []
        for _ in range(reps):
            ds.aovs(r, AOV_SAMPLES, out=aov)
            ms_aov.append(ds.aovs_stats["ms_render"])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _lib.probe_shade(probes, d_sh, aov, W, H, r.settings["gamma"])
            ev[1].record()
            torch.cuda.synchronize()
            ms_shade.append(ev[0].elapsed_time(ev[1]))
    finally:
        ds.close()
    print(f"workload: cornell {W} x {H}, {AOV_SAMPLES} guide samples, {GRID[0]} x {GRID[1]} x {GRID[2]} probes, {reps} alternated repetitions")
    for name in ("host", "device"):
        print(f"{name:7s} wall median {np.median(t[name]) * 1e3:9.1f} ms  (all: {' '.join(f'{x * 1e3:.1f}' for x in t[name])})")
    print(f"wall ratio host / device {np.median(t['host']) / np.median(t['device']):.2f}")
    print(f"device path's parts: fw_render_aovs median {np.median(ms_aov):.2f} ms (ms_render), fw_probe_shade median {np.median(ms_shade):.2f} ms "
          f"(device events around the call, outputs allocated inside)")
    diff = np.abs(out["host"].astype(np.float64) - out["device"])
    print(f"largest |host frame - device frame| {float(diff.max()):.3e}, pixels that differ {int((diff.max(axis=1) > 0).sum())} of {W * H} "
          f"(the host path rounds the same float64 lookup; sqrt may differ by ulps)")


def kernel(calls):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    grid = api.ProbeGrid((40.0, 40.0, 40.0), (515.0, 515.0, 515.0), GRID, True)
    n = W * H
    sh = torch.from_numpy(rng.normal(size=(grid.n_probes, 9, 3)).astype(np.float32)).to(dev)
    # records as a frame has them: neighbouring pixels at neighbouring positions (a plane through the grid), unit normals
    y, x = np.meshgrid(np.linspace(60.0, 500.0, H), np.linspace(60.0, 500.0, W), indexing="ij")
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0:3], rec[:, 3] = 0.5, 1.0
    rec[:, 4:7] = (0.0, 0.6, 0.8)
    rec[:, 8], rec[:, 9], rec[:, 10] = x.reshape(-1), y.reshape(-1), 0.5 * (x + y).reshape(-1)
    aov = torch.from_numpy(rec).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
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
    t_irr = timed(lambda: _lib.probe_irradiance(grid, sh, aov[:, 8:11], aov[:, 4:7], out=out))
    t_shade = timed(lambda: _lib.probe_shade(grid, sh, aov, W, H))
    print(f"{n} points, {grid.n_probes} probes, {calls} calls after {WARMUP} (device events around the calls: host call and stream drain included)")
    print(f"copy 1 GiB d2d        {t_copy:8.3f} ms/call  {2 * (1 << 30) / t_copy / 1e6:8.1f} GB/s (read + write)")
    print(f"fw_probe_irradiance   {t_irr:8.3f} ms/call  {n * 36 / t_irr / 1e6:8.1f} GB/s of 24 B + 12 B per point")
    print(f"fw_probe_shade        {t_shade:8.3f} ms/call  {n * 75 / t_shade / 1e6:8.1f} GB/s of 48 B + 27 B per pixel")


def trace(path, calls):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {path}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = W * H

    def durations(match):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if match(r["Kernel_Name"])]
        return d[WARMUP:WARMUP + calls] if len(d) >= WARMUP + calls else d

    # the 1 GiB copies: the first kernel() times after its tensors are made, WARMUP + calls dispatches of one copy kernel, matched by name
    # (torch's copy_ of a contiguous tensor is the runtime's buffer-copy kernel) and by their place before the first k_probe dispatch
    first_probe = next((k for k, r in enumerate(rows) if "k_probe" in r["Kernel_Name"]), len(rows))
    copies = [r for r in rows[:first_probe] if "copy" in r["Kernel_Name"].lower()][-(WARMUP + calls):]
    big = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in copies][WARMUP:]
    copy_rate = None
    if big:
        us = float(np.median(big))
        copy_rate = 2 * (1 << 30) / us / 1e3
        names = sorted({r["Kernel_Name"][:60] for r in copies})
        print(f"1 GiB copy kernels   median {us:9.1f} us over {len(big)} dispatches  {copy_rate:8.1f} GB/s (read + write)  [{', '.join(names)}]")
    else:
        print("no copy kernel found before the first k_probe dispatch: the rates below stand alone")
    for name, per_item in (("k_probe_irradiance", 36), ("k_probe_shade", 75)):
        d = durations(lambda k: name in k)
        if not d:
            print(f"{name}: no dispatch in the trace")
            continue
        us = float(np.median(d))
        rate = n * per_item / us / 1e3
        share = "" if copy_rate is None else f"  {100.0 * rate / copy_rate:5.1f} % of the copy rate"
        print(f"{name:20s} median {us:9.1f} us over {len(d)} dispatches  {rate:8.1f} GB/s of {n * per_item / 1e6:.1f} MB{share}  "
              f"{n / us / 1e3:6.2f} G lookups/s")


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
