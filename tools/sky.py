"""SunSky measurements (fw_sky_map, fw_sky_radiance); the results are kept in profiles/sky.txt.  Nothing here is a gate.

    python tools/sky.py map [--reps N]     fw_sky_map into a device tensor at 2048 x 1024 and 4096 x 2048, the defaults (32 / 16 steps,
                                           S = 8), sun at 35 degrees: device events around the call with the disc off (k_sky_map alone)
                                           and on (k_sky_map, then k_sky_sun); medians of N (default 7) after two warm-ups.  The
                                           exponentials per second that implies — NV (2 NL + 5) per texel that sees the sky — beside
                                           the numpy statement at 256 x 128, and the two results compared.
    python tools/sky.py dirs [--reps N]    fw_sky_radiance on 2^21 device directions, the same way.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _lib, api  # noqa: E402
from firework_amd.api import SunSky  # noqa: E402


def _event_ms(fn):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    ms = [_event_ms(fn)[0] for _ in range(reps)]
    return float(np.median(ms)), ms


def exps_per_texel(sky):
    return sky.view_steps * (2 * sky.light_steps + 5)


def sky_map(reps):
    import torch
    dev = torch.device("cuda", 0)
    sky = SunSky(35.0, 60.0)
    print(f"workload: SunSky(35, 60), {sky.view_steps} / {sky.light_steps} steps, S = {sky.sun_samples}: {exps_per_texel(sky)} float64 exponentials "
          f"and {sky.view_steps * (sky.light_steps + 1)} square roots per texel; {reps} repetitions after two warm-ups, medians, device events")
    for w, h in ((2048, 1024), (4096, 2048)):
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        off, off_all = _median_ms(lambda: _lib.sky_map(sky.to_abi(disc=False), w, h, out=out), reps)
        on, on_all = _median_ms(lambda: _lib.sky_map(sky.to_abi(disc=True), w, h, out=out), reps)
        n = w * h
        print(f"  {w} x {h}: disc off {off:8.3f} ms  (all: {' '.join(f'{x:.3f}' for x in off_all)})")
        print(f"  {' ' * len(f'{w} x {h}')}  disc on  {on:8.3f} ms  (all: {' '.join(f'{x:.3f}' for x in on_all)})   k_sky_sun by difference {on - off:.3f} ms")
        print(f"  {' ' * len(f'{w} x {h}')}  {n * exps_per_texel(sky) / off / 1e6:.1f} G exponentials / s, {n / off / 1e3:.1f} M texels / s, "
              f"{n * 12 / off / 1e6:.2f} GB/s stored")
    w, h = 256, 128
    t0 = time.perf_counter()
    ref = api.sky_map(sky, w, h, disc=True)
    cpu = time.perf_counter() - t0
    got = _lib.sky_map(sky.to_abi(disc=True), w, h)
    print(f"  numpy statement at {w} x {h}: {cpu:.2f} s, {w * h * exps_per_texel(sky) / cpu / 1e6:.1f} M exponentials / s; "
          f"the device's map differs at {int(np.any(got != ref, axis=2).sum())} of {w * h} texels")


def sky_dirs(reps):
    import torch
    dev = torch.device("cuda", 0)
    sky = SunSky(35.0, 60.0)
    n = 1 << 21
    rng = np.random.default_rng(1)
    rays = torch.from_numpy(rng.normal(size=(n, 6)).astype(np.float32)).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ms, all_ms = _median_ms(lambda: _lib.sky_radiance(sky.to_abi(disc=True), rays[:, 3:6], out=out), reps)
    print(f"fw_sky_radiance on {n} device directions inside a ray buffer (stride 6): {ms:.3f} ms  (all: {' '.join(f'{x:.3f}' for x in all_ms)}), "
          f"{n * exps_per_texel(sky) / ms / 1e6:.1f} G exponentials / s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("map", "dirs"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    _lib.init(0)
    {"map": sky_map, "dirs": sky_dirs}[a.what](a.reps)
