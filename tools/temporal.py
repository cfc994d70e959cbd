"""Temporal accumulation measurements (fw_temporal); the results are kept in profiles/temporal.txt.

    python tools/temporal.py device [--calls N]     fw_temporal on device tensors at 1920x1080 under a one-pixel camera pan: time per call by
                                                    device events, beside fw_denoise (L = 5) on the same frame and a device-to-device copy
                                                    of 1 GiB on the same GPU.  For the kernel's own time run it under the profiler, alone:
                                                    rocprofv3 --kernel-trace --stats -d DIR -- python tools/temporal.py device
    python tools/temporal.py sequence [--reps N]    the 8-view cornell orbit at 256x256, 16 spp, end to end with and without temporal=True,
                                                    alternated, medians of the host clock around the whole sequence (it ends in device-to-host
                                                    copies); RMSE of the last view against 4096 spp for both.

Algorithmic bytes per pixel of fw_temporal: 76 (the current record: colour 12, moments 16, guides 48) + 76 (the history, every previous
pixel fetched once) + 32 (colour 12, moments 16, count 4) = 184.
"""
import argparse
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

BYTES_PER_PIXEL = 76 + 76 + 32


def _camera(pos, at, vfov=40.0):
    return api.CameraSettings.default().cam_pos(pos).look_at(at).field_of_view(vfov)


def _plane_frame(cam, w, h, rng, count):
    """a textured plane z = -5 through jittered pixel rays: (color, moments, aov), float32"""
    c = cam.to_abi()
    hh = np.tan(np.radians(c.vfov) / 2.0)
    hw = hh * w / h
    pos = np.array([c.cam_pos.x, c.cam_pos.y, c.cam_pos.z])
    n = w * h
    idx = np.arange(n)
    u = (idx % w + rng.uniform(0.3, 0.7, n)) / w
    v = (h - idx // w + rng.uniform(0.3, 0.7, n)) / h
    d = np.stack([(2 * u - 1) * hw, (2 * v - 1) * hh, -np.ones(n)], axis=1)          # the camera looks down -z
    X = pos[None] + (-5.0 - pos[2]) / d[:, 2:3] * d
    alb = 0.5 + 0.3 * np.sin(X[:, 0:1] * np.array([3.0, 4.0, 5.0]) + X[:, 1:2] * np.array([5.0, 3.0, 4.0]))
    aov = np.zeros((n, 12), np.float32)
    aov[:, 0:3], aov[:, 3], aov[:, 6] = alb, 1, 1
    aov[:, 7], aov[:, 8:11] = np.linalg.norm(X - pos[None], axis=1), X
    color = (alb * rng.uniform(0.6, 1.0, (n, 3))).astype(np.float32)
    mom = np.concatenate([count * color.astype(np.float64) ** 2 + 0.02, np.full((n, 1), count)], axis=1).astype(np.float32)
    return color, mom, aov


def device(calls):
    import torch
    w, h = 1920, 1080
    n = w * h
    rng = np.random.default_rng(1)
    prev = _camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    pixel = 2 * 5.0 * np.tan(np.radians(20.0)) / h                                    # a pixel's size on the plane
    cam = _camera((pixel, 0.0, 0.0), (pixel, 0.0, -1.0))                              # a one-pixel pan
    dev = torch.device("cuda", 0)
    cur = [torch.from_numpy(x).to(dev) for x in _plane_frame(cam, w, h, rng, 16.0)]
    hist = tuple(torch.from_numpy(x).to(dev) for x in _plane_frame(prev, w, h, rng, 48.0))

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    out = {}
    run = lambda: out.update(r=_lib.temporal(cur[0], cur[2], cur[1], hist, None, w, h, cam, prev, 16, 64.0))
    ms_tp = timed(run, calls)
    carried = float((out["r"][2] > 0).float().mean().item())
    ms_dn = timed(lambda: _lib.denoise(cur[0], cur[2], cur[1], w, h, 5, 2.2), max(1, calls // 4))
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    ms_cp = timed(lambda: b.copy_(a), 20)
    copy_rate = 2 * a.numel() * 4 / (ms_cp * 1e-3)
    alg = n * BYTES_PER_PIXEL
    print(f"fw_temporal 1920x1080, device tensors, one-pixel pan, history carried on {carried:.1%} of the pixels, {calls} calls")
    print(f"  per call (device events, allocation of the outputs and the host call included): {ms_tp:.4f} ms")
    print(f"  fw_denoise L=5 on the same frame, per call: {ms_dn:.4f} ms")
    print(f"  device-to-device copy of 1 GiB: {ms_cp:.4f} ms = {copy_rate / 1e12:.2f} TB/s read + written")
    print(f"  algorithmic bytes {alg / 1e6:.1f} MB ({BYTES_PER_PIXEL} B/pixel): {alg / copy_rate * 1e3:.4f} ms at the copy rate; "
          f"the call is {ms_tp / (alg / copy_rate * 1e3):.1f}x that, {alg / (ms_tp * 1e-3) / copy_rate:.1%} of the copy rate")


def sequence(reps):
    w = h = 256
    scene, r = scenes.config("C2_cornell_box", w, h, 16)
    cams = api.orbit_cameras(r._camera, 36)[:8]
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    try:
        for flag in (True, False):
            list(r.render_sequence(ds, cams, temporal=flag))                         # warm-up of every shape
        t = {True: [], False: []}
        last = {}
        for _ in range(reps):
            for flag in (True, False):
                t0 = time.perf_counter()
                last[flag] = list(r.render_sequence(ds, cams, temporal=flag))
                t[flag].append((time.perf_counter() - t0) * 1e3)
        rr = scenes.config("C2_cornell_box", w, h, 4096)[1]
        rr._camera = cams[-1]
        ref = ds.render(rr)
    finally:
        ds.close()
    rmse = lambda x: float(np.sqrt(np.mean((x.gamma.astype(np.float64) - ref.gamma) ** 2)))
    on, off = float(np.median(t[True])), float(np.median(t[False]))
    e_on, e_off, e_raw = rmse(last[True][-1]), rmse(last[False][-1]), rmse(last[False][-1].raw)
    print(f"cornell orbit, 8 views of 36 per turn, 256x256 @16 spp, L = 5, max_history {api.DEFAULT_MAX_HISTORY:g}; {reps} alternated runs")
    print(f"  sequence wall time, median: temporal {on:.2f} ms ({on / 8:.2f} per frame), without {off:.2f} ms ({off / 8:.2f} per frame): "
          f"{(on / off - 1):+.1%}")
    print(f"  spread: temporal {min(t[True]):.2f}..{max(t[True]):.2f} ms, without {min(t[False]):.2f}..{max(t[False]):.2f} ms")
    print(f"  RMSE of view 7 against 4096 spp (gamma floats): raw {e_raw:.5f}, filter alone {e_off:.5f}, temporal + filter {e_on:.5f}: "
          f"ratio {e_on / e_off:.4f}; mean carried-over count {last[True][-1].stats['history_mean']:.1f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "sequence"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    opt = ap.parse_args()
    if _lib.device_count() < 1:
        sys.exit("no GPU visible: these are measurements, there is no CPU path")
    device(opt.calls) if opt.mode == "device" else sequence(opt.reps)
