"""Probe relocation measurements (fw_relocate_probes, fw_probe_survey, the placed lookups); what the two modes print is
kept as sections 3 and 4 of profiles/probe_place.txt (its other sections come from the assembly, the tests and bench.py, as its header
says).  Nothing here is a gate.

    python tools/probe_place.py artefact          cornell, an 8 x 8 x 8 grid over the room: the mean absolute error (linear colour, all
                                                  pixels) of Renderer.render_probe_lit against a 4096-spp path-traced frame of the same
                                                  view (every surface of cornell is diffuse), with the probes where the grid put them and
                                                  with relocation (sh baked at the moved positions), each with and without depth maps; how
                                                  many probes moved and how many ended inactive.
    python tools/probe_place.py split [--reps N]  one fw_relocate_probes call (4 + 1 steps) over a large set under FW_FLAG_TIME_KERNELS:
                                                  k_probe_rays (ms_raygen), the walks (ms_extend), k_probe_survey + k_probe_relocate_step
                                                  (ms_accumulate), medians of N (default 5) after a warm-up, beside the untimed call; then
                                                  fw_probe_survey alone on resident rays and hits by HIP events: its bytes per second at
                                                  44 B per ray beside a device-to-device copy of 256 MiB in the same process.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

W, H = 128, 128
GRID = ((30.0, 30.0, 30.0), (525.0, 525.0, 525.0), (8, 8, 8))
MIN_FRONT = 12.0


def artefact():
    scene, r = scenes.config("C2_cornell_box", W, H, 4096)
    r.seed(3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ref = ds.render(r).linear.astype(np.float64)
        r.samples(64)
        probes = api.ProbeSet.grid(*GRID, 256).seed(1)
        pd = api.ProbeDepth(8, 6, 900.0)
        rl = api.ProbeRelocation(MIN_FRONT, steps=4)
        pl, sv = r.relocate_probes(ds, probes, rl)
        neutral, _sv0 = r.relocate_probes(ds, probes, api.ProbeRelocation(MIN_FRONT, steps=0))      # classified where the grid put them
        print(f"workload: cornell {W} x {H}, grid {GRID[2]} from {GRID[0]} to {GRID[1]}, D = 256, 64 paths per direction, 4 rounds; "
              f"min_front {MIN_FRONT}, max_offset {tuple(round(v, 2) for v in rl.resolved(probes).max_offset)}, 4 + 1 steps; reference 4096 spp")
        print(f"probes: {probes.n_probes}; inside geometry where the grid put them: {int((neutral[:, 3] == 0).sum())}; moved: "
              f"{int(np.any(pl[:, 0:3] != 0, axis=1).sum())}; inactive after relocation: {int((pl[:, 3] == 0).sum())}; "
              f"largest |offset| {np.abs(pl[:, 0:3]).max():.2f}; back hits in the last survey: {int(sv[:, 2, 0].sum())}")
        for name, pset, placement in (("nominal grid", probes, None), ("relocated", probes.moved(pl), pl)):
            sh, _s = r.bake_probes(ds, pset, 4)
            moments, _d = r.bake_probe_depth(ds, pset, pd, 4)
            for vis in (False, True):
                kw = dict(depth=pd, moments=moments, normal_bias=2.0) if vis else {}
                lit = r.render_probe_lit(ds, probes, sh, aov_samples=8, placement=placement, **kw).linear.astype(np.float64)
                err = np.abs(lit - ref)
                print(f"  {name:13s} {'with depth maps' if vis else 'wrap only      '}  mean |error| {err.mean():.5f}   "
                      f"99th percentile {np.percentile(err, 99):.4f}   mean of the reference {ref.mean():.5f}")
    finally:
        ds.close()


def split(reps):
    import torch
    scene, r = scenes.config("C2_cornell_box", W, H, 1)
    r.seed(3)
    s = r.settings
    probes = api.ProbeSet.grid(GRID[0], GRID[1], (32, 32, 32), 256).seed(1)
    n, D = probes.n_probes, probes.directions
    rl = api.ProbeRelocation(MIN_FRONT, steps=4)
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)
    try:
        call = lambda flags: ds.relocate_probes(probes, rl, seed=s["seed"], use_bvh=s["use_bvh"], flags=flags)[2]      # noqa: E731
        call(0)
        plain, timed = [], []
        for _ in range(reps):
            plain.append(call(0))
            timed.append(call(A.FW_FLAG_TIME_KERNELS))
        rays = _lib.probe_rays(probes, 0, out=torch.empty((n * D, 6), dtype=torch.float32, device=dev))
        hits = ds.trace(rays, s["use_bvh"], seed=s["seed"])
        out = torch.empty((n, 3, 4), dtype=torch.float32, device=dev)
        a, b = torch.empty(64 << 20, dtype=torch.float32, device=dev), torch.empty(64 << 20, dtype=torch.float32, device=dev)
        _lib.probe_survey(rays, hits, D, out=out)
        b.copy_(a)
        survey_ms, copy_ms = [], []
        for _ in range(reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            ev[0].record()
            _lib.probe_survey(rays, hits, D, out=out)          # (returns with the stream drained: the events bracket launch and wait)
            ev[1].record()
            ev[2].record()
            b.copy_(a)
            ev[3].record()
            torch.cuda.synchronize()
            survey_ms.append(ev[0].elapsed_time(ev[1]))
            copy_ms.append(ev[2].elapsed_time(ev[3]))
    finally:
        ds.close()
    med = lambda rows, key: float(np.median([x[key] for x in rows]))      # noqa: E731
    print(f"workload: cornell, {n} probes x D = {D} = {n * D} rays per step, 4 + 1 steps = {plain[0]['rays']} rays traced; {reps} repetitions after "
          f"one warm-up, medians")
    print(f"fw_relocate_probes             ms_render {med(plain, 'ms_render'):8.3f}  ms_wall {med(plain, 'ms_wall'):8.3f}  "
          f"(all ms_render: {' '.join('%.3f' % x['ms_render'] for x in plain)})")
    print(f"  under FW_FLAG_TIME_KERNELS   ms_render {med(timed, 'ms_render'):8.3f}  k_probe_rays {med(timed, 'ms_raygen'):7.3f}  "
          f"walks {med(timed, 'ms_extend'):7.3f}  k_probe_survey + k_probe_relocate_step {med(timed, 'ms_accumulate'):7.3f}  "
          f"(all of the last: {' '.join('%.3f' % x['ms_accumulate'] for x in timed)})")
    t, c = float(np.median(survey_ms)), float(np.median(copy_ms))
    print(f"  fw_probe_survey alone, {n * D} resident rays: median {t:.3f} ms by events around the call = {n * D * 44 / t / 1e6:.1f} GB/s at 44 B per ray "
          f"(24 B of ray, 20 B of the 48-byte hit); device-to-device copy of 256 MiB: {2 * (256 << 20) / c / 1e6:.1f} GB/s read + written "
          f"(median {c:.3f} ms)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("artefact", "split"))
    ap.add_argument("--reps", type=int, default=None)
    opt = ap.parse_args()
    if opt.mode == "artefact":
        artefact()
    else:
        split(5 if opt.reps is None else opt.reps)


if __name__ == "__main__":
    main()
