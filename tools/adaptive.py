"""Adaptive sampling measurements: for cornell_box 512x512 and suzanne 960x540, cap 1024, min 16, at several tolerances:
the rounds and their active pixels, the sample fraction sum(n_p) / (W*H*1024), and the wall time of fw_render_adaptive against fw_render at
1024 spp in the same process, alternated, `--reps` times each.  Every output goes to host memory in both calls.

    python tools/adaptive.py [--reps 5] [--tols 0.05,0.02,0.01] [--mins 16] [--json out.json]
    python tools/adaptive.py --profile        one adaptive render per scene and tolerance, nothing else (for rocprofv3 --kernel-trace --stats)

k_accumulate_adaptive's bytes for a kernel-time roofline: 16 B per sample record read, plus 32 B per pixel and launch read and 32 B
written (sums and squares); accumulate_bytes() estimates them from the sample count, the round sizes and the batches."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _lib, scenes  # noqa: E402

CASES = [("C2_cornell_box", 512, 512), ("C3_suzanne", 960, 540)]
CAP = 1024


def accumulate_bytes(stats, rounds):
    """k_accumulate_adaptive's bytes: 16 B per sample record read, and 32 B per pixel read + 32 B written per launch (one launch per batch;
    the pixels of a round are spread over its batches evenly in this estimate: n_batches / rounds launches per round)"""
    return 16 * stats["samples"] + 64 * sum(rounds) * stats["n_batches"] / max(1, len(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tols", default="0.05,0.02,0.01")
    ap.add_argument("--json", default=None)
    ap.add_argument("--mins", default="16", help="min_samples values to run, comma-separated")
    ap.add_argument("--profile", action="store_true")
    opt = ap.parse_args()
    tols = [float(t) for t in opt.tols.split(",")]
    mins = [int(m) for m in opt.mins.split(",")]
    _lib.init(0)
    results = []
    for name, w, h in CASES:
        scene, renderer = scenes.config(name, w, h, CAP)
        ds = _lib.DeviceScene(scene.to_desc())
        fixed_rays = ds.render(renderer).stats["rays"]         # (also the warm-up: arena, code objects)
        for mn, tol in [(m, t) for m in mins for t in tols]:
            res = ds.render_adaptive(renderer, tol, mn)
            rounds = res.rounds
            frac = res.stats["samples"] / (w * h * CAP)
            row = dict(scene=name, width=w, height=h, tol=tol, min_samples=mn, rounds=rounds, sample_fraction=frac, n_batches=res.stats["n_batches"],
                       mean_spp=res.stats["samples"] / (w * h), accumulate_bytes=accumulate_bytes(res.stats, rounds))
            at_min = res.moments[:, 3] == mn
            row.update(stopped_at_min=float(at_min.mean()), stopped_at_min_all_black=float((at_min & (res.accum[:, :3] == 0).all(1)).mean()),
                       at_cap=float((res.moments[:, 3] == CAP).mean()), ray_fraction=res.stats["rays"] / fixed_rays)
            if not opt.profile:
                t_ad, t_fix, ms_ad, ms_fix = [], [], [], []
                for _ in range(opt.reps):                      # alternated in one process
                    t0 = time.perf_counter()
                    a = ds.render_adaptive(renderer, tol, mn)
                    t_ad.append((time.perf_counter() - t0) * 1e3)
                    ms_ad.append(a.stats["ms_render"])
                    t0 = time.perf_counter()
                    f = ds.render(renderer)
                    t_fix.append((time.perf_counter() - t0) * 1e3)
                    ms_fix.append(f.stats["ms_render"])
                row.update(wall_adaptive_ms=t_ad, wall_fixed_ms=t_fix, render_adaptive_ms=ms_ad, render_fixed_ms=ms_fix,
                           speedup_median=statistics.median(t_fix) / statistics.median(t_ad))
            results.append(row)
            print(json.dumps(row), flush=True)
        ds.close()
    if opt.json:
        with open(opt.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
