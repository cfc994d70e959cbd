"""Ambient-occlusion measurements (fw_bake_ao, Renderer.render_ao); the results are kept in profiles/ao.txt.  Nothing
here is a gate.  Workload: cornell at 512 x 512 from its own camera, D = 64, radius 120, one round.

    python tools/ao.py paths [--reps N]    Renderer.render_ao (fw_render_aovs on the device, fw_bake_ao on the records in place) against
                                           the host path — fw_render_aovs to the host, numpy api.ao_rays, fw_trace_rays with host arrays,
                                           numpy api.ao_reduce and api.ao_resolve — alternated, host first, one warm-up each, then N
                                           (default 3) runs each by the wall clock with the device drained; both end on the host, and
                                           the two results are compared bit for bit (numpy's sin and cos are not the device's: the
                                           count of differing values is reported, not expected to be 0).
    python tools/ao.py split [--reps N]    fw_bake_ao on resident records under FW_FLAG_TIME_KERNELS: k_ao_rays (ms_raygen), the walks
                                           (ms_extend) and k_ao_reduce (ms_accumulate), medians of N (default 5) after a warm-up, beside
                                           the untimed call; the reducer's achieved bytes per second at 72 B per ray beside the copy
                                           rate of a device-to-device copy of 256 MiB measured in the same process.
    python tools/ao.py beyond              the share of traced rays whose hit lay at or beyond the radius — the work a ranged query
                                           would have cut short — for a few radii, from fw_ao_rays and fw_trace_rays chained by hand.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

W, H, D, RADIUS = 512, 512, 64, 120.0
SLAB = 16384                      # points per slab of the host path's numpy statements


def _setup():
    scene, r = scenes.config("C2_cornell_box", W, H, 1)
    r.seed(3)
    return scene, r, api.AmbientOcclusion(RADIUS, D).seed(1)


def _host_path(ds, r, ao):
    s = r.settings
    rec = ds.aovs(r, 1)
    n = rec.shape[0]
    sums = np.zeros((n, 4), np.float32)
    for q0 in range(0, n, SLAB):
        ids = np.arange(q0, min(n, q0 + SLAB), dtype=np.uint32)
        rays = api.ao_rays(ao, rec[:, 8:11], rec[:, 4:7], ids, 0)
        hits = ds.trace(rays, s["use_bvh"], seed=s["seed"], key_base=q0 * D)
        sums[ids] = api.ao_reduce(ao, rays, hits["t"], hits["object"]).astype(np.float32)
    return api.ao_resolve(sums, 1)


def paths(reps):
    import torch
    scene, r, ao = _setup()
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ms = dict(host=[], device=[])
        for k in range(reps + 1):                                                         # run 0 warms both up
            for name in ("host", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "host":
                    host = _host_path(ds, r, ao)
                else:
                    occ, bent, _sums = r.render_ao(ds, ao, 1, 1)
                torch.cuda.synchronize()
                if k:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
    finally:
        ds.close()
    dev = np.concatenate([bent.reshape(-1, 3), occ.reshape(-1, 1)], axis=1)
    differ = dev.view(np.uint32) != host.view(np.uint32)
    print(f"workload: cornell {W} x {H}, D = {D}, radius {RADIUS}, one round = {W * H * D} rays; alternated, host first, {reps} runs each after one warm-up, "
          f"wall clock, device drained")
    for name, t in ms.items():
        print(f"{name:7s} path  median {np.median(t):10.2f} ms   (all: {' '.join('%.2f' % x for x in t)})")
    print(f"ratio host / device {np.median(ms['host']) / np.median(ms['device']):.1f}")
    print(f"bit for bit: ao differs at {int(differ[:, 3].sum())} of {W * H} pixels (largest |difference| {np.abs(dev[:, 3] - host[:, 3]).max():.3e}), "
          f"bent at {int(differ[:, :3].any(axis=1).sum())} (largest component difference {np.abs(dev[:, :3] - host[:, :3]).max():.3e})")


def split(reps):
    import torch
    scene, r, ao = _setup()
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)
    try:
        aov = ds.aovs(r, 1, out=torch.empty((W * H, 12), dtype=torch.float32, device=dev))
        call = lambda flags: ds.bake_ao(ao, aov[:, 8:11], aov[:, 4:7], None, 1, seed=s["seed"], use_bvh=s["use_bvh"], flags=flags)[2]      # noqa: E731
        call(0)
        plain, timed = [], []
        for _ in range(reps):
            plain.append(call(0))
            timed.append(call(A.FW_FLAG_TIME_KERNELS))
        # the box's copy rate: 256 MiB device to device, read and written once
        a, b = torch.empty(64 << 20, dtype=torch.float32, device=dev), torch.empty(64 << 20, dtype=torch.float32, device=dev)
        b.copy_(a)
        copy_ms = []
        for _ in range(reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            b.copy_(a)
            ev[1].record()
            torch.cuda.synchronize()
            copy_ms.append(ev[0].elapsed_time(ev[1]))
    finally:
        ds.close()
    med = lambda rows, key: float(np.median([x[key] for x in rows]))      # noqa: E731
    traced = plain[0]["rays"]
    print(f"workload: cornell {W} x {H} records resident, D = {D}, one round = {W * H * D} rays of which {traced} traced (the rest belong to pixels that "
          f"missed the scene); {reps} repetitions after one warm-up, medians")
    print(f"fw_bake_ao                     ms_render {med(plain, 'ms_render'):8.3f}  ms_wall {med(plain, 'ms_wall'):8.3f}  "
          f"(all ms_render: {' '.join('%.3f' % x['ms_render'] for x in plain)})")
    print(f"  under FW_FLAG_TIME_KERNELS   ms_render {med(timed, 'ms_render'):8.3f}  k_ao_rays {med(timed, 'ms_raygen'):7.3f}  "
          f"walks {med(timed, 'ms_extend'):7.3f}  k_ao_reduce {med(timed, 'ms_accumulate'):7.3f}  "
          f"(all k_ao_reduce: {' '.join('%.3f' % x['ms_accumulate'] for x in timed)})")
    t, c = med(timed, "ms_accumulate"), float(np.median(copy_ms))
    print(f"  k_ao_reduce: {W * H * D * 72 / t / 1e6:.1f} GB/s at 72 B per ray (24 B of ray, 48 B of hit; of a hit 8 B are used); "
          f"device-to-device copy of 256 MiB: {2 * (256 << 20) / c / 1e6:.1f} GB/s read + written (median {c:.3f} ms)")
    print(f"  k_ao_rays: {W * H * D * 24 / med(timed, 'ms_raygen') / 1e6:.1f} GB/s written at 24 B per ray")


def beyond():
    import torch
    scene, r, _ao = _setup()
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)
    try:
        aov = ds.aovs(r, 1, out=torch.empty((W * H, 12), dtype=torch.float32, device=dev))
        rays = _lib.ao_rays(api.AmbientOcclusion(RADIUS, D).seed(1), aov[:, 8:11], aov[:, 4:7])
        hits = ds.trace(rays, s["use_bvh"], seed=s["seed"])
        f = _lib.hit_fields(hits)
        live = torch.any(rays[:, 3:] != 0, dim=1)
        dist = f["t"].double() * torch.linalg.norm(rays[:, 3:].double(), dim=1)
        hit = live & (f["object"] != -1)
        traced = int(live.sum())
        print(f"workload: cornell {W} x {H}, D = {D}: {traced} rays traced, {int(hit.sum())} of them hit something ({100.0 * int(hit.sum()) / traced:.1f} %)")
        for radius in (30.0, 60.0, RADIUS, 240.0, 480.0):
            far = int((hit & (dist >= radius)).sum())
            print(f"  radius {radius:6.1f}: {far} hits at or beyond it = {100.0 * far / traced:.1f} % of the traced rays ({100.0 * far / max(1, int(hit.sum())):.1f} % of the hits); "
                  f"with the misses, {100.0 * (far + traced - int(hit.sum())) / traced:.1f} % of the rays change nothing")
    finally:
        ds.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("paths", "split", "beyond"))
    ap.add_argument("--reps", type=int, default=None)
    opt = ap.parse_args()
    if opt.mode == "paths":
        paths(3 if opt.reps is None else opt.reps)
    elif opt.mode == "split":
        split(5 if opt.reps is None else opt.reps)
    else:
        beyond()


if __name__ == "__main__":
    main()
