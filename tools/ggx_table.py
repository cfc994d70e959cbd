"""GGX albedo table measurements (fw_ggx_table, fw_ggx_table_lookup, fw_probe_shade_split); the results are kept in
profiles/ggx_table.txt.  Nothing here is a gate.

    python tools/ggx_table.py table [--reps N]   fw_ggx_table into a device tensor at 64 x 64 texels x 128^2 samples and at 256 x 256 x
                                                 256^2: device events around the call, medians of N (default 7) after two warm-ups,
                                                 and the samples per second that implies; beside the numpy statement's time for the
                                                 small table, and the two results compared.
    python tools/ggx_table.py shade [--reps N]   fw_ggx_table_lookup and fw_probe_shade_split on 1920 x 1080 hand-made records (a
                                                 third of them glossy) beside fw_probe_shade_glossy on the same records, the same way.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _lib, api  # noqa: E402
from firework_amd.api import GgxTable, ProbeGrid, ProbeRadiance  # noqa: E402


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


def table(reps):
    import torch
    dev = torch.device("cuda", 0)
    print(f"fw_ggx_table into a device tensor; {reps} repetitions after two warm-ups, medians, device events")
    for n, m in ((64, 128), (256, 256)):
        g = GgxTable(n, n, m, m)
        out = torch.empty((n, n, 2), dtype=torch.float32, device=dev)
        ms, all_ms = _median_ms(lambda: _lib.ggx_table(g, out=out), reps)
        samples = n * n * m * m
        print(f"  {n} x {n} texels x {m} x {m} samples: {ms:8.3f} ms  (all: {' '.join(f'{x:.3f}' for x in all_ms)})   "
              f"{samples / ms / 1e6:.2f} G samples / s, {n * n / ms / 1e3:.2f} M texels / s")
    g = GgxTable(64, 64, 128, 128)
    t0 = time.perf_counter()
    ref = api.ggx_table(64, 64, 128, 128)
    cpu = time.perf_counter() - t0
    got = _lib.ggx_table(g)
    ulp = np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32))
    print(f"  numpy statement at 64 x 64 x 128 x 128: {cpu:.2f} s, {64 * 64 * 128 * 128 / cpu / 1e6:.1f} M samples / s; the device's table "
          f"differs at {int(np.any(got != ref, axis=2).sum())} of {64 * 64} texels, by at most {float(ulp.max()):.2f} float32 ulps")


def shade(reps):
    import torch
    dev = torch.device("cuda", 0)
    w, h = 1920, 1080
    n = w * h
    rng = np.random.default_rng(1)
    grid = ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8), True)
    pr = ProbeRadiance(16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    sh = t(rng.normal(size=(512, 9, 3)).astype(np.float32))
    maps = t(rng.uniform(0.0, 4.0, size=(512, pr.texels, 4)).astype(np.float32))
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0:3], rec[:, 3] = rng.uniform(0.0, 1.0, size=(n, 3)), 1.0
    nrm = rng.normal(size=(n, 3))
    rec[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    rec[:, 8:11] = rng.uniform(0.0, 1.0, size=(n, 3))
    spec = np.zeros((n, 4), np.float32)
    spec[:, 0:3] = rng.uniform(0.0, 1.0, size=(n, 3))
    spec[::3, 3] = rng.uniform(0.05, 1.0, size=len(spec[::3]))
    rays = np.zeros((n, 6), np.float32)
    rays[:, 3:6] = -rec[:, 4:7] + 0.5 * rng.normal(size=(n, 3))
    d_rec, d_spec, d_rays = t(rec), t(spec), t(rays)
    table = _lib.ggx_table(GgxTable(), out=torch.empty((64, 64, 2), dtype=torch.float32, device=dev))
    mu, rho = t(rng.uniform(0.0, 1.0, n).astype(np.float32)), t(rng.uniform(0.0, 1.0, n).astype(np.float32))
    out = torch.empty((n, 2), dtype=torch.float32, device=dev)
    print(f"{w} x {h} records, a third glossy, 512 probes with R = 16 maps, a 64 x 64 table; {reps} repetitions after two warm-ups, medians, device events")
    ms, all_ms = _median_ms(lambda: _lib.ggx_table_lookup(table, mu, rho, out=out), reps)
    print(f"  fw_ggx_table_lookup      {ms:8.3f} ms  (all: {' '.join(f'{x:.3f}' for x in all_ms)})   {n * 16 / ms / 1e6:.1f} GB/s of pairs and terms")
    for name, fn in (("fw_probe_shade_glossy   ", lambda: _lib.probe_shade_glossy(grid, sh, pr, maps, d_rec, d_spec, d_rays[:, 3:6], w, h)),
                     ("fw_probe_shade_split    ", lambda: _lib.probe_shade_split(grid, sh, pr, maps, d_rec, d_spec, d_rays[:, 3:6], table, w, h, 0)),
                     ("fw_probe_shade_split + E", lambda: _lib.probe_shade_split(grid, sh, pr, maps, d_rec, d_spec, d_rays[:, 3:6], table, w, h, 1))):
        ms, all_ms = _median_ms(fn, reps)
        print(f"  {name} {ms:8.3f} ms  (all: {' '.join(f'{x:.3f}' for x in all_ms)})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("table", "shade"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    _lib.init(0)
    {"table": table, "shade": shade}[a.what](a.reps)
