"""Camera-model measurements (fw_model_rays, fw_render_model); the results are kept in profiles/camera_models.txt.

    python tools/camera_models.py kernel [--calls N]   k_model_rays at 2048x1024 x 16 samples into a device tensor, each model: time per
                                                       fw_model_rays call by device events (host call and stream drain included), beside
                                                       a device-to-device copy of 1 GiB on the same GPU.  The kernel's own time comes only
                                                       from a run under the profiler, alone:
                                                       rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/camera_models.py kernel
    python tools/camera_models.py trace DIR [--calls N] that run's *_kernel_trace.csv, read back: k_model_rays' dispatches in the order `kernel`
                                                       made them (per model and jitter, 3 warm-up calls then N), medians of the N, as
                                                       24 B/ray against the 1 GiB copies' own kernel time in the same trace
    python tools/camera_models.py wall [--reps N]      hdri_test as a 2048x1024 panorama at 64 spp, end to end (host clock; both paths end
                                                       in device-to-host copies of the frame): the host path — api.panorama_rays in numpy,
                                                       copied to the device, Renderer.render_camera_model — and Renderer.render_model,
                                                       alternated, medians; and the summed device time (fw_stats.ms_render) of both.

The kernel reads nothing and writes 24 B per ray.
"""
import argparse
import functools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _lib, api, scenes  # noqa: E402

W, H = 2048, 1024


def _models(samples_seed=1):
    cam = api.CameraSettings.default().cam_pos((3.0, 30.0, 50.0)).look_at((0.5, -1.0, 2.0))
    return dict(panorama=api.CameraModel.panorama(cam._cam_pos, W, H).seed(samples_seed),
                orthographic=api.CameraModel.orthographic(cam, 7.5, W, H).seed(samples_seed),
                fisheye=api.CameraModel.fisheye(cam, 180.0, W, H).seed(samples_seed))


def kernel(calls):
    import torch
    dev = torch.device("cuda", 0)
    n_samples = 16
    out = torch.empty((n_samples, W * H, 6), dtype=torch.float32, device=dev)

    def timed(fn, reps):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    ms_cp = timed(lambda: b.copy_(a), 20)
    copy_rate = 2 * a.numel() * 4 / (ms_cp * 1e-3)
    del a, b
    rays = n_samples * W * H
    print(f"k_model_rays {W}x{H} x {n_samples} samples = {rays / 1e6:.1f} M rays, {rays * 24 / 1e6:.1f} MB written, {calls} calls per model")
    print(f"  device-to-device copy of 1 GiB: {ms_cp:.4f} ms = {copy_rate / 1e12:.2f} TB/s read + written")
    print(f"  24 B/ray at the copy rate: {rays * 24 / copy_rate * 1e3:.4f} ms")
    print("  per call below: device events around fw_model_rays calls, each of which drains the stream — the host call and the drain are")
    print("  included; the kernel's own time comes only from the separate rocprofv3 --kernel-trace --stats run")
    for name, m in _models().items():
        for jitter in (True, False):
            m.jitter(jitter)
            ms = timed(lambda: _lib.model_rays(m, 0, n_samples, out=out), calls)       # (the call drains the stream: host latency included)
            print(f"  {name:13s} jitter {int(jitter)}: {ms:.4f} ms per call = {rays / ms / 1e6:.2f} G rays/s, {rays * 24 / (ms * 1e-3) / 1e12:.3f} TB/s written, "
                  f"{rays * 24 / (ms * 1e-3) / copy_rate:.1%} of the copy rate")


WARMUP = 3


def trace(directory, calls):
    """the kernel's own times from the profiler's trace of one `kernel` run: dispatches in start order, grouped as `kernel` issued them"""
    import csv
    import glob
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        sys.exit(f"expected one *kernel_trace.csv under {directory}, found {len(paths)}")
    with open(paths[0], newline="") as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    gen = [d for _, d, name in rows if "k_model_rays" in name]
    groups = [(name, jitter) for name in _models() for jitter in (1, 0)]
    if len(gen) != len(groups) * (WARMUP + calls):
        sys.exit(f"{len(gen)} k_model_rays dispatches, expected {len(groups)} x ({WARMUP} + {calls}): pass the run's --calls")
    first_gen = next(t for t, _, name in rows if "k_model_rays" in name)
    copies = [d for t, d, name in rows if t < first_gen and "copyBuffer" in name and d > 50_000]        # the 1 GiB copies, not torch's small ones
    rays = 16 * W * H
    print(f"k_model_rays {W}x{H} x 16 samples = {rays / 1e6:.1f} M rays, {rays * 24 / 1e6:.1f} MB written; kernel times from {os.path.basename(paths[0])}")
    copy_rate = None
    if copies:
        us_cp = float(np.median(copies)) / 1e3
        copy_rate = 2 * (1 << 30) / (us_cp * 1e-6)
        print(f"  device-to-device copy of 1 GiB ({len(copies)} dispatches of {sorted(set(n for _, d, n in rows if 'copyBuffer' in n and d > 50_000))}): "
              f"median {us_cp:.1f} us = {copy_rate / 1e12:.2f} TB/s read + written; 24 B/ray at that rate: {rays * 24 / copy_rate * 1e6:.1f} us")
    else:
        print("  no copy kernel in the trace (the copy went through a DMA engine): use the copy rate `kernel` printed in the same run")
    for i, (name, jitter) in enumerate(groups):
        d = np.array(gen[i * (WARMUP + calls) + WARMUP:(i + 1) * (WARMUP + calls)], dtype=np.float64) / 1e3
        us = float(np.median(d))
        rate = rays * 24 / (us * 1e-6)
        share = f", {rate / copy_rate:.1%} of the copy rate" if copy_rate else ""
        print(f"  {name:13s} jitter {jitter}: median {us:.1f} us ({d.min():.1f}..{d.max():.1f}) = {rays / us / 1e3:.2f} G rays/s, {rate / 1e12:.3f} TB/s written{share}")


def wall(reps):
    spp = 64
    scene, r = scenes.config("C4a_hdri_test", W, H, spp)
    pos = r._camera._cam_pos
    ds = _lib.DeviceScene(scene.to_desc(), 0)
    chunk = max(1, min(64, (1 << 30) // (W * H * 24)))          # the host path's chunk: rays below 1 GiB, as the CLI had it

    def host_path():
        """Renderer.render_camera_model over api.panorama_rays(..., device=0) — the path the CLI had — with the device times of its
        fw_render_rays calls summed (DeviceScene.render_rays is wrapped for the duration of the call to read each chunk's fw_stats)"""
        model = functools.partial(api.panorama_rays, pos, W, H, seed=r.settings["seed"], device=0)
        dev_ms = []
        inner = ds.render_rays

        def counted(*a, **kw):
            res = inner(*a, **kw)
            dev_ms.append(res.stats["ms_render"])
            return res

        ds.render_rays = counted
        try:
            res = r.render_camera_model(ds, model, spp, chunk=chunk)
        finally:
            del ds.render_rays
        return res.rgb8.cpu().numpy(), float(sum(dev_ms))

    def device_path(on_device=True):
        """Renderer.render_model with device outputs, as the host path has them (the u8 frame is copied back, as there); with host
        outputs every chunk is the fw_render_rays call of that chunk and moves the (W*H, 4) sums to the device and back"""
        res = r.render_model(ds, api.CameraModel.panorama(pos, W, H).seed(r.settings["seed"]), spp, on_device=on_device)
        return (res.rgb8.cpu().numpy() if on_device else res.rgb8), res.stats["ms_render"]

    try:
        device_path()
        paths = (("host", host_path), ("device", device_path), ("device_host_out", functools.partial(device_path, False)))
        t = {name: [] for name, _ in paths}
        d = {name: [] for name, _ in paths}
        img = {}
        for _ in range(reps):
            for name, fn in paths:
                t0 = time.perf_counter()
                img[name], ms = fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
                d[name].append(ms)
                print(f"  run {len(t[name])} {name}: wall {t[name][-1]:.1f} ms, device {ms:.2f} ms", flush=True)
    finally:
        ds.close()
    th, dh = float(np.median(t["host"])), float(np.median(d["host"]))
    print(f"hdri_test {W}x{H} panorama @{spp} spp, {reps} alternated runs, medians")
    print(f"  numpy rays + render_camera_model (chunks of {chunk}): wall {th:.1f} ms ({min(t['host']):.1f}..{max(t['host']):.1f}), "
          f"device time (fw_stats.ms_render summed) {dh:.2f} ms")
    for name, what in (("device", "render_model, device outputs"), ("device_host_out", "render_model, host outputs")):
        tw, dd = float(np.median(t[name])), float(np.median(d[name]))
        diff = int((img["host"] != img[name]).any(axis=1).sum())
        print(f"  {what}: wall {tw:.1f} ms ({min(t[name]):.1f}..{max(t[name]):.1f}) = {th / tw:.0f}x faster; device time {dd:.2f} ms "
              f"(generator included) = {dd / dh:.3f}x the host path's; pixels whose rgb8 differs from the host path's: {diff} of {W * H}")

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "trace", "wall"))
    ap.add_argument("directory", nargs="?", help="trace: the profiler's output directory")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    opt = ap.parse_args()
    if opt.mode == "trace":
        trace(opt.directory, opt.calls)
        sys.exit(0)
    if _lib.device_count() < 1:
        sys.exit("no GPU visible: these are measurements, there is no CPU path")
    kernel(opt.calls) if opt.mode == "kernel" else wall(opt.reps)
