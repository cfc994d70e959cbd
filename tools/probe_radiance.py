"""Probe-radiance measurements (fw_probe_radiance_reduce, fw_probe_radiance_prefilter, fw_probe_radiance_lookup, fw_probe_shade_glossy,
fw_bake_probe_radiance); the results are kept in profiles/probe_radiance.txt.  Nothing here is a gate.

    python tools/probe_radiance.py [--calls N] [--out profiles/probe_radiance.txt]

One process, three parts, every call timed by device events around it (the host call and the stream drain included) after 2 warm-up
calls, N (default 7) calls each, the kernels of a part alternated; medians, with the least and the most.
  maps    32 768 probes, D = 256, seeded random unit rays, radiances and hits on the device; for R = 16 (three levels) and R = 32 (four):
          k_probe_radiance_reduce and k_probe_radiance_prefilter, beside k_probe_depth at the same R on the same rays.
  points  1920 x 1080 seeded random records inside a 32 x 32 x 32 grid; for R = 16 and R = 32: k_probe_radiance_lookup beside
          k_probe_irradiance<true, false>, and k_probe_shade_glossy (every pixel glossy) beside k_probe_shade<true, false> (<PLACED,
          DEPTH>: the placed forms), on the same records, with a neutral placement and without depth maps.
  bake    cornell, the same 32 768 probes, D = 256, one round of one sample, R = 16 and R = 32: fw_bake_probe_radiance's ms_render
          (first launch to last) and, under FW_FLAG_TIME_KERNELS, k_probe_rays (ms_raygen) and the reducers with the prefilter
          (ms_accumulate); the prefilter of the bake's own sums alone beside them.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

GRID, D, W, H, WARMUP = (32, 32, 32), 256, 1920, 1080, 2
CHAINS = {16: (0.1, 0.4, 1.0), 32: (0.1, 0.25, 0.5, 1.0)}


def timed(fns, calls):
    """{name: [ms, ...]} of the callables, alternated"""
    import torch
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
    return ms


def line(name, t, note=""):
    return f"  {name:34s} median {np.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  {note}"


def maps_part(calls, say):
    import torch
    dev = torch.device("cuda", 0)
    n = GRID[0] * GRID[1] * GRID[2]
    g = torch.Generator(device=dev).manual_seed(1)
    d = torch.randn((n * D, 3), generator=g, device=dev)
    rays = torch.zeros((n * D, 6), device=dev)
    rays[:, 3:] = d / d.norm(dim=1, keepdim=True)
    accum = torch.rand((n * D, 4), generator=g, device=dev) * 3.0
    hits = torch.zeros((n * D, 12), device=dev)
    hits[:, 0] = torch.rand((n * D,), generator=g, device=dev) * 5.0                      # t; object 0: a hit
    say(f"maps: {n} probes, D = {D}: {n * D} rays; {calls} calls each after {WARMUP}")
    for R, chain in CHAINS.items():
        pr, pd = api.ProbeRadiance(R, 2, chain), api.ProbeDepth(R, 6, 10.0)
        sums = torch.zeros((n, R, R, 4), device=dev)
        dsums = torch.zeros((n, R, R, 4), device=dev)
        out = torch.empty((n, pr.texels, 4), device=dev)
        _lib.probe_radiance_reduce(pr, rays, accum, 1, D, sums=sums)
        ms = timed(dict(k_probe_radiance_reduce=lambda: _lib.probe_radiance_reduce(pr, rays, accum, 1, D, sums=sums),
                        k_probe_depth=lambda: _lib.probe_depth_reduce(pd, rays, hits, D, sums=dsums),
                        k_probe_radiance_prefilter=lambda: _lib.probe_radiance_prefilter(pr, sums, out=out)), calls)
        pairs = n * D * R * R
        pf_pairs = n * (pr.texels - R * R) * R * R
        say(f" R = {R}, {pr.levels} levels, M = {pr.texels} texels per probe")
        t = np.median(ms["k_probe_radiance_reduce"])
        say(line("k_probe_radiance_reduce", ms["k_probe_radiance_reduce"],
                 f"{pairs / t / 1e6:8.1f} G (ray, texel) pairs/s; reads {n * D * 40 / t / 1e6:7.1f} GB/s"))
        t = np.median(ms["k_probe_depth"])
        say(line("k_probe_depth (k = 6)", ms["k_probe_depth"], f"{pairs / t / 1e6:8.1f} G (ray, texel) pairs/s"))
        t = np.median(ms["k_probe_radiance_prefilter"])
        say(line("k_probe_radiance_prefilter", ms["k_probe_radiance_prefilter"],
                 f"{pf_pairs / t / 1e6:8.1f} G (output, source) pairs/s; moves {n * (R * R + pr.texels) * 16 / t / 1e6:7.1f} GB/s"))
        del sums, dsums, out


def points_part(calls, say):
    import torch
    dev = torch.device("cuda", 0)
    n_probes, n = GRID[0] * GRID[1] * GRID[2], W * H
    grid = api.ProbeGrid((0.0, 0.0, 0.0), (31.0, 31.0, 31.0), GRID, True)
    g = torch.Generator(device=dev).manual_seed(2)
    unit = lambda: torch.nn.functional.normalize(torch.randn((n, 3), generator=g, device=dev), dim=1)      # noqa: E731
    rec = torch.zeros((n, 12), device=dev)
    rec[:, 0:3] = torch.rand((n, 3), generator=g, device=dev)
    rec[:, 3] = 1.0
    rec[:, 4:7] = unit()
    rec[:, 8:11] = torch.rand((n, 3), generator=g, device=dev) * 31.0
    pos, nrm, dirs = rec[:, 8:11].contiguous(), rec[:, 4:7].contiguous(), unit()
    rough = torch.rand((n,), generator=g, device=dev)
    spec = torch.cat([torch.rand((n, 3), generator=g, device=dev), rough[:, None] * 0.9 + 0.05], dim=1).contiguous()
    sh = torch.randn((n_probes, 9, 3), generator=g, device=dev)
    neutral = torch.zeros((n_probes, 4), device=dev)
    neutral[:, 3] = 1.0
    out = torch.empty((n, 3), device=dev)
    say(f"points: {n} records (seeded random points inside a {GRID[0]} x {GRID[1]} x {GRID[2]} grid, wrap on, neutral placement, no depth "
        f"maps); {calls} calls each after {WARMUP}")
    for R, chain in CHAINS.items():
        pr = api.ProbeRadiance(R, 2, chain)
        maps = torch.rand((n_probes, pr.texels, 4), generator=g, device=dev)
        ms = timed({"k_probe_radiance_lookup": lambda: _lib.probe_radiance_lookup(grid, pr, maps, pos, nrm, dirs, rough, placement=neutral, out=out),
                    "k_probe_irradiance<true, false>": lambda: _lib.probe_irradiance_placed(grid, sh, neutral, pos, nrm, out=out),
                    "k_probe_shade_glossy": lambda: _lib.probe_shade_glossy(grid, sh, pr, maps, rec, spec, dirs, W, H, placement=neutral),
                    "k_probe_shade<true, false>": lambda: _lib.probe_shade_placed(grid, sh, neutral, rec, W, H)}, calls)
        say(f" R = {R}, {pr.levels} levels: maps of {n_probes * pr.texels * 16 / 2 ** 20:.0f} MiB; a point reads 8 corners x 2 levels x 4 texels x 16 B = 1024 B of them")
        for name, t in ms.items():
            say(line(name, t, f"{n / np.median(t) / 1e6:7.2f} G points/s"))
        del maps


def bake_part(calls, say):
    import torch
    scene, r = scenes.config("C2_cornell_box", 64, 64, 1)
    r.seed(3)
    probes = api.ProbeSet.grid((40.0, 40.0, 40.0), (515.0, 515.0, 515.0), GRID, D).seed(1)
    ds = _lib.DeviceScene(scene.to_desc())
    say(f"bake: cornell, {probes.n_probes} probes, D = {D}, one round of one sample; {calls} calls each after one warm-up")
    try:
        for R, chain in CHAINS.items():
            pr = api.ProbeRadiance(R, 2, chain)
            r.settings["flags"] &= ~A.FW_FLAG_TIME_KERNELS
            _maps, sums = r.bake_probe_radiance(ds, probes, pr, 1, on_device=True)
            plain, parts = [], []
            for _ in range(calls):
                r.settings["flags"] &= ~A.FW_FLAG_TIME_KERNELS
                r.bake_probe_radiance(ds, probes, pr, 1, on_device=True)
                plain.append(dict(r.probe_radiance_stats))
                r.settings["flags"] |= A.FW_FLAG_TIME_KERNELS
                r.bake_probe_radiance(ds, probes, pr, 1, on_device=True)
                parts.append(dict(r.probe_radiance_stats))
            r.settings["flags"] &= ~A.FW_FLAG_TIME_KERNELS
            out = torch.empty((probes.n_probes, pr.texels, 4), device=sums.device)
            pf = timed(dict(prefilter=lambda: _lib.probe_radiance_prefilter(pr, sums, out=out)), calls)["prefilter"]
            med = lambda rows, key: float(np.median([x[key] for x in rows]))      # noqa: E731
            rest = med(parts, "ms_render") - med(parts, "ms_raygen") - med(parts, "ms_accumulate")
            say(f" R = {R}, {pr.levels} levels")
            say(f"  fw_bake_probe_radiance           ms_render {med(plain, 'ms_render'):9.3f}  ms_wall {med(plain, 'ms_wall'):9.3f}  "
                f"(all ms_render: {' '.join('%.3f' % x['ms_render'] for x in plain)})")
            say(f"    under FW_FLAG_TIME_KERNELS     ms_render {med(parts, 'ms_render'):9.3f}  k_probe_rays {med(parts, 'ms_raygen'):8.3f}  "
                f"reduce + prefilter {med(parts, 'ms_accumulate'):9.3f}  the render pass (the rest) {rest:9.3f}")
            say(line("k_probe_radiance_prefilter alone", pf, f"{np.median(pf) / rest:6.2f} x the render pass"))
            del sums, out
    finally:
        ds.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_radiance.txt"))
    opt = ap.parse_args()
    import torch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/probe_radiance.py --calls {opt.calls} on {torch.cuda.get_device_name(0)}")
    maps_part(opt.calls, say)
    points_part(opt.calls, say)
    bake_part(opt.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
