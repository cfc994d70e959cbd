"""fw_render_rays measurements: fw_render_rays on device camera rays against fw_render_progressive over the same sample
chunks (both with device accum and outputs, so both sides make the same calls), and one single-call comparison with fw_render.  The
rays are made once, on the device (fw_camera_rays, outside the timed region); each side's time is the sum of its calls' device time
(fw_stats.ms_render) per frame and the synchronised host wall time, medians over alternated frames.  Prints one JSON line per case.

    python tools/render_rays.py --case c2        cornell_box 512x512 @1024 in chunks of 64
    python tools/render_rays.py --case c3        suzanne 960x540 @256 in chunks of 64
    python tools/render_rays.py --case single    cornell_box 512x512 @64, one call against fw_render
    python tools/render_rays.py --case pano      hdri_test, a 2048x1024 panorama from its camera @64 (one call; no counterpart)
    [--reps 5] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, scenes  # noqa: E402
from firework_amd.api import panorama_rays  # noqa: E402

CASES = {"c2": ("C2_cornell_box", 512, 512, 1024, 64), "c3": ("C3_suzanne", 960, 540, 256, 64),
         "single": ("C2_cornell_box", 512, 512, 64, 64), "pano": ("C4a_hdri_test", 2048, 1024, 64, 64)}


def device_camera_rays(lib, r, first, n, stream):
    """(n, W*H, 6) float32 device tensor: fw_camera_rays of samples first .. first + n - 1"""
    s = r.settings
    out = torch.empty((n, s["width"] * s["height"], 6), dtype=torch.float32, device="cuda")
    for k in range(n):
        p = r.to_params(None)
        p.outputs_on_device = 1
        p.stream = C.c_void_p(stream)
        _lib._check(lib, lib.fw_camera_rays(C.byref(p), 0, first + k, C.c_void_p(out[k].data_ptr())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    opt = ap.parse_args()
    name, w, h, spp, chunk = CASES[opt.case]
    lib = _lib.load(preload=True, device=0)
    scene, r = scenes.config(name, w, h, spp)
    s = r.settings
    n = w * h
    ds = _lib.DeviceScene(scene.to_desc())
    stream = torch.cuda.current_stream().cuda_stream
    outs = [torch.empty((n, 3), dtype=dt, device="cuda") for dt in (torch.uint8, torch.float32, torch.float32)]
    ptrs = [C.c_void_p(t.data_ptr()) for t in outs]

    if opt.case == "pano":
        rays = torch.stack([torch.from_numpy(panorama_rays(r._camera._cam_pos, w, h, k, seed=s["seed"])) for k in range(spp)]).cuda()
        chunks = [(0, spp, rays)]
    else:
        chunks = [(lo, min(chunk, spp - lo), device_camera_rays(lib, r, lo, min(chunk, spp - lo), stream)) for lo in range(0, spp, chunk)]
    torch.cuda.synchronize()

    def rays_frame():
        acc = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        dev_ms = 0.0
        for lo, k, rays in chunks:
            res = ds.render_rays(rays, k, lo, acc, seed=s["seed"], use_bvh=s["use_bvh"], gamma=s["gamma"])
            dev_ms += res.stats["ms_render"]
        return dev_ms, res

    def render_frame():
        if opt.case == "single":
            p = r.to_params(None)
            p.outputs_on_device = 1
            p.stream = C.c_void_p(stream)
            st = A.fw_stats()
            _lib._check(lib, lib.fw_render(ds.handle, C.byref(p), ptrs[0], ptrs[1], ptrs[2], C.byref(st)))
            return st.ms_render, outs[0].clone()
        acc = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        dev_ms = 0.0
        for lo, k, _ in chunks:
            p = r.to_params(None)
            p.samples = k
            p.outputs_on_device = 1
            p.stream = C.c_void_p(stream)
            st = A.fw_stats()
            _lib._check(lib, lib.fw_render_progressive(ds.handle, C.byref(p), lo, C.c_void_p(acc.data_ptr()), ptrs[0], ptrs[1], ptrs[2], C.byref(st)))
            dev_ms += st.ms_render
        return dev_ms, outs[0].clone()

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev, out = f()
        torch.cuda.synchronize()
        return dev, (time.perf_counter() - t0) * 1e3, out

    timed(rays_frame)
    if opt.case != "pano":
        timed(render_frame)                                   # warm-up: arena, code objects
    d_rays, w_rays, d_ref, w_ref = [], [], [], []
    same = True
    for _ in range(opt.reps):
        if opt.case != "pano":
            d, wt, ref = timed(render_frame); d_ref.append(d); w_ref.append(wt)
        d, wt, res = timed(rays_frame); d_rays.append(d); w_rays.append(wt)
        if opt.case != "pano":
            same = same and bool(torch.equal(res.rgb8, ref))
    med = lambda x: round(statistics.median(x), 3) if x else None      # noqa: E731
    out = dict(case=opt.case, scene=name, width=w, height=h, spp=spp, chunk=chunk, calls=len(chunks), reps=opt.reps,
               rays_device_ms=med(d_rays), rays_wall_ms=med(w_rays),
               ref=("fw_render" if opt.case == "single" else "fw_render_progressive" if opt.case != "pano" else None),
               ref_device_ms=med(d_ref), ref_wall_ms=med(w_ref),
               ratio_device=(round(statistics.median(d_rays) / statistics.median(d_ref), 4) if d_ref else None),
               rays_device_all=[round(x, 2) for x in d_rays], ref_device_all=[round(x, 2) for x in d_ref],
               bit_identical=(same if opt.case != "pano" else None), rays=int(res.stats["rays"]))
    print(json.dumps(out))
    if opt.json:
        with open(opt.json, "a") as f:
            f.write(json.dumps(out) + "\n")
    ds.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
