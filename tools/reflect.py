"""Reflection-gather measurements (fw_bake_reflect); the results are kept in profiles/reflect.txt.  Nothing here is a
gate.  Workload: fw_render_aovs' records of cornell at 1920 x 1080 from its own camera, resident on the device; probes on a 6 x 6 x 6
grid baked in the call.  Cornell has no conductor, so every pixel on a surface is given the same (F0, rho) = (0.9, 0.9, 0.9, RHO): the
bake reads spec per point and does not look at the receiver's material.  The view is the camera's sample-0 rays.

    python tools/reflect.py [--reps N] [--directions D] [--rho RHO]
        fw_bake_gather and fw_bake_reflect alternated on the same records with the same D (default 16), bias, seed and one round under
        FW_FLAG_TIME_KERNELS: rays = ms_raygen (k_ao_rays / k_reflect_rays), walks = ms_extend, after the trace = ms_accumulate
        (k_hit_surface + the probe lookup + the reduction); run 0 warms both up, then N (default 3) runs each.  Then k_reflect_rays and
        k_ao_rays alone on one chunk of 2^17 points through the public calls, device events around each call (its launch and final
        synchronisation included), median and minimum of 20.
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
    ap.add_argument("--directions", type=int, default=16)
    ap.add_argument("--rho", type=float, default=0.3)
    opt = ap.parse_args()
    D = opt.directions
    scene, r = scenes.config("C2_cornell_box", W, H, 1)
    r.seed(3)
    s = r.settings
    dev = torch.device("cuda", 0)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        probes = api.ProbeSet.grid((30.0, 30.0, 30.0), (525.0, 525.0, 525.0), (6, 6, 6), 256)
        baker = api.Renderer.default().samples(16).use_bvh(True).seed(1)
        sh, _sums = baker.bake_probes(ds, probes, 4)
        grid = api.ProbeGrid.of(probes, True)
        d_sh = torch.from_numpy(sh).to(dev)
        aov = torch.empty((W * H, 12), dtype=torch.float32, device=dev)
        ds.aovs(r, 1, out=aov)
        rays = torch.from_numpy(ds.camera_rays(r, 0)).to(dev)
        on = aov[:, 3] > 0
        spec = torch.zeros((W * H, 4), dtype=torch.float32, device=dev)
        spec[on] = torch.tensor([0.9, 0.9, 0.9, opt.rho], dtype=torch.float32, device=dev)
        n_on = int(on.sum())
        print(f"records: {W} x {H} cornell, {n_on} pixels on surfaces, every one glossy at rho = {opt.rho}, D = {D}, 1 round, FW_FLAG_TIME_KERNELS")
        gather = api.FinalGather(D, 0.5).seed(1)
        reflect = api.ReflectionGather(D).bias(0.5).seed(1)
        kw = dict(rounds=1, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"] | A.FW_FLAG_TIME_KERNELS)
        pos, nrm, view = aov[:, 8:11], aov[:, 4:7], rays[:, 3:6]
        for k in range(opt.reps + 1):
            for name in ("fw_bake_gather ", "fw_bake_reflect"):
                if name.strip() == "fw_bake_gather":
                    _o, _s, st = ds.bake_gather(gather, grid, d_sh, pos, nrm, None, **kw)
                else:
                    out, _s, st = ds.bake_reflect(reflect, grid, d_sh, pos, nrm, view, spec, None, **kw)
                print(f"run {k} {name}: ms_render {st['ms_render']:.2f} (rays {st['ms_raygen']:.2f}, walks {st['ms_extend']:.2f}, after the trace "
                      f"{st['ms_accumulate']:.2f}), wall {st['ms_wall']:.2f}, rays traced {st['rays']}, batches {st['n_batches']}")
        alive = float(out[on][:, 3].mean())
        print(f"fw_bake_reflect: mean share of alive rays on surfaces {alive:.4f}, mean reflected radiance {out[on][:, 0:3].mean(dim=0).cpu().numpy()}")
        # the two ray kernels alone, one chunk
        n = 1 << 17
        ids = torch.nonzero(on).flatten()[:n].to(torch.int32).contiguous()
        n = int(ids.numel())
        o_r = torch.empty((n * D, 6), dtype=torch.float32, device=dev)
        o_w = torch.empty((n * D, 2), dtype=torch.float32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ao = gather.ao()
        print(f"one chunk of {n} points x {D} rays = {n * D} rays, each call with its launch and its final synchronisation, median (min) of 20:")
        for name, call in (("fw_ao_rays     ", lambda: _lib.ao_rays(ao, pos, nrm, ids, 0, out=o_r)),
                           ("fw_reflect_rays", lambda: _lib.reflect_rays(reflect, pos, nrm, view, spec, ids, 0, out=o_r, weights=o_w))):
            call()
            ms = []
            for _ in range(20):
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            print(f"  {name} {np.median(ms):.3f} ({min(ms):.3f}) ms: {n * D / np.median(ms) / 1e6:.2f} G rays per second")
    finally:
        ds.close()


if __name__ == "__main__":
    main()
