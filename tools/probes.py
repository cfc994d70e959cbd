"""Probe-baker measurements (fw_probe_rays, fw_probe_project, fw_bake_probes); the results are kept in profiles/probes.txt.
Nothing here is a gate.  The workload: cornell, a 16 x 16 x 16 grid x D = 256 directions x S = 16 samples x 4 rounds.

    python tools/probes.py wall [--reps N]      Renderer.bake_probes against the host path it replaces — numpy ProbeSet.rays, fw_render_rays
                                                with host arrays, api.sh_project — alternated, medians of N (default 5): wall time (host
                                                clock; both paths end with the coefficients on the host) and the summed device time
                                                (fw_stats.ms_render).  Also the largest difference between the two paths' coefficients.
    python tools/probes.py kernel [--calls N]   k_probe_rays and k_probe_project alone on device tensors of the workload's size, beside a
                                                device-to-device copy of 1 GiB: time per call by device events (host call and stream drain
                                                included).  The kernels' own time comes only from a run under the profiler, alone:
                                                rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/probes.py kernel
    python tools/probes.py trace DIR [--calls N] that run's *_kernel_trace.csv, read back: the two kernels' dispatches (3 warm-up calls then
                                                N), medians of the N, as bytes over time — k_probe_rays writes 24 B per entry and reads
                                                12 B per probe, k_probe_project reads 40 B per entry and reads and writes 108 B per probe
                                                — against the 1 GiB copies' own kernel time in the same trace.
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

GRID, D, S, ROUNDS = (16, 16, 16), 256, 16, 4
WARMUP = 3


def _probes():
    return api.ProbeSet.grid((40.0, 40.0, 40.0), (515.0, 515.0, 515.0), GRID, D).seed(1)


def wall(reps):
    scene, r = scenes.config("C2_cornell_box", 8, 8, S)
    r.use_bvh(False).seed(3)
    probes = _probes()
    n = probes.n_probes
    ds = _lib.DeviceScene(scene.to_desc())
    s = r.settings

    def device_path():
        sh, _sums = r.bake_probes(ds, probes, ROUNDS)
        return sh, r.probe_stats["ms_render"]

    def host_path():
        sums = np.zeros((n, 9, 3))
        ms = 0.0
        for rnd in range(ROUNDS):
            rays = probes.rays(rnd)
            res = ds.render_rays(rays, S, 0, None, seed=s["seed"] + rnd, use_bvh=s["use_bvh"], paths_per_batch=s["paths_per_batch"], flags=s["flags"])
            ms += res.stats["ms_render"]
            sums += api.sh_project(rays, res.accum, S, D)
        return (sums / ROUNDS).astype(np.float32), ms

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
    print(f"workload: cornell, {n} probes x {D} directions x {S} samples x {ROUNDS} rounds, {reps} alternated repetitions")
    for name in ("host", "device"):
        print(f"{name:7s} wall median {np.median(t[name]) * 1e3:9.1f} ms  (all: {' '.join(f'{x * 1e3:.1f}' for x in t[name])})   "
              f"device time median {np.median(dev_ms[name]):8.1f} ms")
    print(f"wall ratio host / device {np.median(t['host']) / np.median(t['device']):.2f}")
    print(f"largest |sh_host - sh_device| {float(np.abs(out['host'].astype(np.float64) - out['device']).max()):.3e} "
          f"(largest |sh| {float(np.abs(out['device']).max()):.3e}; the rays differ by float32 neighbours, so paths may differ)")


def kernel(calls):
    import torch
    dev = torch.device("cuda", 0)
    probes = _probes()
    n = probes.n_probes
    rays = torch.empty((n * D, 6), dtype=torch.float32, device=dev)
    accum = torch.rand((n * D, 4), dtype=torch.float32, device=dev)
    sums = torch.zeros((n, 9, 3), dtype=torch.float32, device=dev)
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
    t_rays = timed(lambda: _lib.probe_rays(probes, 1, out=rays))
    t_proj = timed(lambda: _lib.probe_project(rays, accum, S, D, sums=sums))
    print(f"{n} probes x {D} directions, {calls} calls after {WARMUP} (device events around the calls: host call, upload of the positions and "
          f"stream drain included)")
    print(f"copy 1 GiB d2d      {t_copy:8.3f} ms/call  {2 * (1 << 30) / t_copy / 1e6:8.1f} GB/s (read + write)")
    print(f"fw_probe_rays       {t_rays:8.3f} ms/call  {n * D * 24 / t_rays / 1e6:8.1f} GB/s of 24 B/entry")
    print(f"fw_probe_project    {t_proj:8.3f} ms/call  {n * D * 40 / t_proj / 1e6:8.1f} GB/s of 40 B/entry")


def trace(path, calls):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {path}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = _probes().n_probes

    def durations(match):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if match(r["Kernel_Name"])]
        return d[WARMUP:WARMUP + calls] if len(d) >= WARMUP + calls else d

    big = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows
           if "k_probe" not in r["Kernel_Name"] and int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) > 100000]
    if big:
        us = float(np.median(big))
        print(f"1 GiB copy kernels   median {us:9.1f} us over {len(big)} dispatches  {2 * (1 << 30) / us / 1e3:8.1f} GB/s (read + write)")
    for name, per_entry, per_probe in (("k_probe_rays", 24, 12), ("k_probe_project", 40, 216)):
        d = durations(lambda k: name in k)
        if not d:
            print(f"{name}: no dispatch in the trace")
            continue
        us = float(np.median(d))
        bytes_ = n * D * per_entry + n * per_probe
        print(f"{name:20s} median {us:9.1f} us over {len(d)} dispatches  {bytes_ / us / 1e3:8.1f} GB/s of {bytes_ / 1e6:.1f} MB")


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
