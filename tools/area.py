"""Area-light measurements (fw_bake_area, FW_GATHER_NO_LIGHTS); the results are kept in profiles/area.txt.  Nothing here
is a gate.  Workload: cornell (C2_cornell_box) from its own camera; probes on §9z's grid — 6 x 6 x 6 over (30, 30, 30) .. (525, 525,
525), 256 directions, 16 samples, 4 rounds, 16 x 16 depth moments — baked in the call.

    python tools/area.py [--reps N] [--samples S] [--directions D]
        Part 1: fw_render_aovs' records of a 1920 x 1080 frame stay on the device; fw_bake_area (S = 16 shadow rays per pixel and
        light, cornell has one lamp) and fw_bake_gather (D = 64, plain lookup) alternated on them with one round under
        FW_FLAG_TIME_KERNELS: rays = ms_raygen, walks = ms_extend, after the trace = ms_accumulate (fw_bake_area: k_hit_surface +
        k_area_reduce); run 0 warms both up, then N (default 3) runs each.
        Part 2: fw_area_rays and fw_area_reduce as public calls on one chunk of 2^17 points x 16 = 2^21 entries, device tensors,
        device events around each call (its launch and final synchronisation included), median and minimum of 20.
        Part 3: RMSE of the 256 x 256 previews against fw_render at 4096 spp, linear frames clipped to [0, 1], with visibility and
        normal bias 2 as §9z measured them: the plain preview, --probe-gather 64, and --probe-gather 64 --area-light 16.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

W, H = 1920, 1080


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--directions", type=int, default=64)
    opt = ap.parse_args()
    S, D = opt.samples, opt.directions
    scene, r = scenes.config("C2_cornell_box", W, H, 1)
    r.seed(3)
    s = r.settings
    dev = torch.device("cuda", 0)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        probes = api.ProbeSet.grid((30.0, 30.0, 30.0), (525.0, 525.0, 525.0), (6, 6, 6), 256)
        baker = api.Renderer.default().samples(16).use_bvh(True).seed(1)
        sh, _sums = baker.bake_probes(ds, probes, 4)
        pd = api.ProbeDepth(16, 6, 800.0)
        moments, _dsums = baker.bake_probe_depth(ds, probes, pd, 4)
        grid = api.ProbeGrid.of(probes, True)
        d_sh = torch.from_numpy(sh).to(dev)
        rec = ds.area_lights()
        print(f"sampled lights: {rec.shape[0]} (objects {rec[:, 0].astype(int).tolist()}, kinds {rec[:, 1].astype(int).tolist()})")
        # ---- part 1
        aov = torch.empty((W * H, 12), dtype=torch.float32, device=dev)
        ds.aovs(r, 1, out=aov)
        on = aov[:, 3] > 0
        print(f"records: {W} x {H} cornell, {int(on.sum())} pixels on surfaces, 1 round, FW_FLAG_TIME_KERNELS")
        area, gather = api.AreaLight(S, 0.5).seed(1), api.FinalGather(D, 0.5).seed(1)
        kw = dict(rounds=1, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"] | A.FW_FLAG_TIME_KERNELS)
        pos, nrm = aov[:, 8:11], aov[:, 4:7]
        for k in range(opt.reps + 1):
            for name in (f"fw_bake_area S={S}  ", f"fw_bake_gather D={D}"):
                if "area" in name:
                    out, _s, st = ds.bake_area(area, pos, nrm, None, **kw)
                else:
                    _o, _s, st = ds.bake_gather(gather, grid, d_sh, pos, nrm, None, **kw)
                print(f"run {k} {name}: ms_render {st['ms_render']:.2f} (rays {st['ms_raygen']:.2f}, walks {st['ms_extend']:.2f}, after the trace "
                      f"{st['ms_accumulate']:.2f}), wall {st['ms_wall']:.2f}, rays traced {st['rays']}, batches {st['n_batches']}")
        print(f"fw_bake_area: mean visible share on surfaces {float(out[on][:, 3].mean()):.4f}, mean irradiance {out[on][:, 0:3].mean(dim=0).cpu().numpy()}")
        # ---- part 2
        n = 1 << 17
        ids = torch.nonzero(on).flatten()[:n].to(torch.int32).contiguous()
        n = int(ids.numel())
        M = rec.shape[0] * S
        o_r = torch.empty((n * M, 6), dtype=torch.float32, device=dev)
        o_w = torch.empty((n * M,), dtype=torch.float32, device=dev)
        _lib.area_rays(area, rec, pos, nrm, ids, 0, out=o_r, weights=o_w)
        hits = ds.trace(o_r, True, seed=1)
        surf = ds.hit_surface(o_r, hits)
        sums = torch.zeros((W * H, 4), dtype=torch.float32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        print(f"one chunk of {n} points x {M} entries = {n * M} entries, each call with its launch and its final synchronisation, median (min) of 20:")
        for name, call, nbytes, what in (
                ("fw_area_rays  ", lambda: _lib.area_rays(area, rec, pos, nrm, ids, 0, out=o_r, weights=o_w), 24 + 4, "24 + 4 B written per entry"),
                ("fw_area_reduce", lambda: _lib.area_reduce(o_w, hits, surf, rec, S, sums, ids), 4 + 4 + 32,
                 "4 + 4 + 32 B read per entry (the weight, the object word of a 48 B hit, two float4 of a 64 B record)")):
            call()
            ms = []
            for _ in range(20):
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            print(f"  {name} {np.median(ms):.3f} ({min(ms):.3f}) ms: {n * M * nbytes / np.median(ms) / 1e6:.0f} GB/s over {what}")
    finally:
        ds.close()
    # ---- part 3
    scene, r = scenes.config("C2_cornell_box", 256, 256, 4096)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        full = np.asarray(ds.render(r).linear).reshape(-1, 3).astype(np.float64)
        ref, lamp = np.clip(full, 0.0, 1.0), np.any(full >= 1.0, axis=1)
        kw = dict(aov_samples=8, depth=pd, moments=moments, normal_bias=2.0)
        g = api.FinalGather(D, 1e-3).seed(0)
        frames = [("--probe-lit", {}), (f"--probe-lit --probe-gather {D}", dict(gather=g)),
                  (f"--probe-lit --probe-gather {D} --area-light {S}", dict(gather=g, area=api.AreaLight(S, 1e-3).seed(0))),
                  (f"--probe-lit --probe-gather {D},4 --area-light {S},4", dict(gather=g, gather_rounds=4, area=api.AreaLight(S, 1e-3).seed(0), area_rounds=4))]
        print(f"RMSE against fw_render 256 x 256 at 4096 spp, linear frames clipped to [0, 1] (and without the {int(lamp.sum())} pixels where the reference is >= 1):")
        for name, extra in frames:
            lit = np.clip(r.render_probe_lit(ds, probes, sh, **kw, **extra).linear.reshape(-1, 3).astype(np.float64), 0.0, 1.0)
            print(f"  {name:52s} {float(np.sqrt(np.mean((lit - ref) ** 2))):.4f}   ({float(np.sqrt(np.mean((lit[~lamp] - ref[~lamp]) ** 2))):.4f})")
    finally:
        ds.close()


if __name__ == "__main__":
    main()
