"""Direct-light measurements (fw_bake_direct, Renderer.render_probe_lit with direct); the results are kept in
profiles/direct.txt.  Nothing here is a gate.  Workload: cornell at 1920 x 1080 from its own camera, its first-hit records resident, Ln
point, spot and directional lights under the ceiling, one round.

    python tools/direct.py split [--reps N]    fw_bake_direct on the resident records with 1, 3 and 64 lights: device events around the
                                               call, and the call's own ms_render; under FW_FLAG_TIME_KERNELS k_direct_rays (ms_raygen),
                                               the walks (ms_extend) and k_direct_reduce (ms_accumulate).  Medians of N (default 7) after
                                               two warm-ups; the kernels' achieved bytes per second beside a device-to-device copy of 256
                                               MiB measured in the same process.
    python tools/direct.py paths [--reps N]    the same bake with 1 and 3 lights against the host path — numpy api.direct_rays,
                                               fw_trace_rays with host arrays, numpy api.direct_reduce over slabs of points — alternated,
                                               host first, by the wall clock with the device drained: N (default 3) runs each after one
                                               warm-up (a host run takes seconds); the two results are compared.
    python tools/direct.py probe_lit [--reps N] Renderer.render_probe_lit on scenes/three_lights.yml at 1920 x 1080 with and without
                                               direct, alternated, wall clock with the device drained, medians of N (default 7) after two
                                               warm-ups.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402
from firework_amd.api import DirectionalLight, DirectLight, PointLight, SpotLight  # noqa: E402

W, H = 1920, 1080
SLAB = 65536                      # points per slab of the host path's numpy statements


def lights(n):
    """n lights of the three kinds in turn on a grid under cornell's ceiling (the room is 555 wide)"""
    side = int(np.ceil(np.sqrt(n)))
    out = []
    for i in range(n):
        x, z = 60.0 + 435.0 * ((i % side) + 0.5) / side, 60.0 + 435.0 * ((i // side) + 0.5) / side
        if i % 3 == 0:
            out.append(PointLight((x, 500.0, z), (60000.0 / n, 50000.0 / n, 40000.0 / n)))
        elif i % 3 == 1:
            out.append(SpotLight((x, 520.0, z), (278.0 - x, -500.0, 278.0 - z), (90000.0 / n,) * 3, 25.0, 50.0))
        else:
            out.append(DirectionalLight((0.3 * (x - 278.0) / 278.0, -1.0, 0.4 * (z - 278.0) / 278.0), (2.0 / n, 1.5 / n, 1.0 / n)))
    return out


def _setup():
    scene, r = scenes.config("C2_cornell_box", W, H, 1)
    r.seed(3)
    return scene, r, DirectLight(1e-3, "renderer")


def _event_ms(fn):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def split(reps):
    import torch
    scene, r, d = _setup()
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)
    med = lambda rows, key: float(np.median([x[key] for x in rows]))      # noqa: E731
    try:
        aov = ds.aovs(r, 1, out=torch.empty((W * H, 12), dtype=torch.float32, device=dev))
        a, b = torch.empty(64 << 20, dtype=torch.float32, device=dev), torch.empty(64 << 20, dtype=torch.float32, device=dev)
        b.copy_(a)
        copy_ms = [_event_ms(lambda: b.copy_(a))[0] for _ in range(reps)]
        c = float(np.median(copy_ms))
        print(f"workload: cornell {W} x {H} records resident ({W * H} points), one round; {reps} repetitions after two warm-ups, medians")
        print(f"device-to-device copy of 256 MiB: {2 * (256 << 20) / c / 1e6:.1f} GB/s read + written (median {c:.3f} ms)")
        for Ln in (1, 3, 64):
            ds.set_lights(lights(Ln))
            call = lambda flags: ds.bake_direct(d, aov[:, 8:11], aov[:, 4:7], None, None, None, 1, seed=s["seed"], use_bvh=s["use_bvh"], flags=flags)[2]      # noqa: E731
            for _ in range(2):
                call(0)
                call(A.FW_FLAG_TIME_KERNELS)
            plain, timed, events = [], [], []
            for _ in range(reps):
                ms, st = _event_ms(lambda: call(0))
                events.append(ms)
                plain.append(st)
                timed.append(call(A.FW_FLAG_TIME_KERNELS))
            entries, traced = W * H * Ln, plain[0]["rays"]
            print(f"Ln = {Ln:2d}: {entries} entries of which {traced} traced; {plain[0]['n_batches']} trace batches")
            print(f"  fw_bake_direct                 device events {float(np.median(events)):8.3f} ms  ms_render {med(plain, 'ms_render'):8.3f}  ms_wall {med(plain, 'ms_wall'):8.3f}  "
                  f"(all events: {' '.join('%.3f' % x for x in events)})")
            g, x, a_ = med(timed, "ms_raygen"), med(timed, "ms_extend"), med(timed, "ms_accumulate")
            print(f"    under FW_FLAG_TIME_KERNELS   ms_render {med(timed, 'ms_render'):8.3f}  k_direct_rays {g:7.3f}  walks {x:7.3f}  k_direct_reduce {a_:7.3f}")
            print(f"    k_direct_rays: {entries * 24 / g / 1e6:.1f} GB/s written at 24 B per entry; k_direct_reduce: {entries * 32 / a_ / 1e6:.1f} GB/s at 32 B per entry "
                  f"(24 B of ray, 8 B of the hit's 48)")
    finally:
        ds.close()


def _host_path(ds, r, d, lts, rec):
    s = r.settings
    n, Ln = rec.shape[0], len(lts)
    sums = np.zeros((n, 8), np.float32)
    for q0 in range(0, n, SLAB):
        ids = np.arange(q0, min(n, q0 + SLAB), dtype=np.uint32)
        rays = api.direct_rays(d, lts, rec[:, 8:11], rec[:, 4:7], ids)
        hits = ds.trace(rays, s["use_bvh"], seed=s["seed"], key_base=q0 * Ln)
        sums[ids, 0:7] = api.direct_reduce(d, lts, rec[:, 8:11], rec[:, 4:7], rays, hits["t"], hits["object"], ids).astype(np.float32)
    return api.direct_resolve(sums, 1)


def paths(reps):
    import torch
    scene, r, d = _setup()
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    dev = torch.device("cuda", ds.device)
    try:
        aov = ds.aovs(r, 1, out=torch.empty((W * H, 12), dtype=torch.float32, device=dev))
        rec = aov.cpu().numpy()
        print(f"workload: cornell {W} x {H} records ({W * H} points), one round; alternated, host first, {reps} runs each after one warm-up, wall clock, "
              f"device drained; the device path starts and ends on the host like the host path (records uploaded, result copied back)")
        for Ln in (1, 3):
            lts = lights(Ln)
            ds.set_lights(lts)
            ms = dict(host=[], device=[])
            for k in range(reps + 1):                                                     # run 0 warms both up
                for name in ("host", "device"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name == "host":
                        host = _host_path(ds, r, d, lts, rec)
                    else:
                        out = ds.bake_direct(d, rec[:, 8:11], rec[:, 4:7], None, None, None, 1, seed=s["seed"], use_bvh=s["use_bvh"])[0]
                    torch.cuda.synchronize()
                    if k:
                        ms[name].append(1e3 * (time.perf_counter() - t0))
            differ = np.any(out.view(np.uint32) != host.view(np.uint32), axis=1)
            scale = np.maximum(np.abs(host), 1e-30)
            print(f"Ln = {Ln}:")
            for name, t in ms.items():
                print(f"  {name:7s} path  median {np.median(t):10.2f} ms   (all: {' '.join('%.2f' % x for x in t)})")
            print(f"  ratio host / device {np.median(ms['host']) / np.median(ms['device']):.1f}; the results differ at {int(differ.sum())} of {W * H} points "
                  f"(largest relative difference {float((np.abs(out - host) / scale)[differ].max()) if differ.any() else 0.0:.3e}: the device's rays are within "
                  f"one float32 ulp of numpy's)")
    finally:
        ds.close()


def probe_lit(reps):
    import torch
    from firework_amd import yaml_io
    from firework_amd.api import ProbeSet
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "three_lights.yml"))
    cam = api.CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = api.Renderer.default().width(W).height(H).samples(4).use_bvh(True).camera(cam).seed(0)
    probes = ProbeSet.grid((-24.0, 2.0, -12.0), (24.0, 12.0, 12.0), (4, 2, 4), 64)
    d = DirectLight()
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        sh, _ = r.bake_probes(ds, probes, 1)
        ms = dict(plain=[], direct=[])
        for k in range(reps + 2):
            for name in ("plain", "direct"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = r.render_probe_lit(ds, probes, sh, aov_samples=1, direct=d if name == "direct" else None)
                torch.cuda.synchronize()
                if k >= 2:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        st = r.direct_stats
    finally:
        ds.close()
    print(f"workload: scenes/three_lights.yml {W} x {H}, aov_samples 1, a 4 x 2 x 4 probe grid; alternated, {reps} runs each after two warm-ups, wall clock, "
          f"device drained, the frame copied to the host")
    for name, t in ms.items():
        print(f"  render_probe_lit {name:6s}  median {np.median(t):8.2f} ms   (all: {' '.join('%.2f' % x for x in t)})")
    print(f"  the direct term's fw_bake_direct: ms_render {st['ms_render']:.3f}, {st['rays']} rays traced; the rest of the difference is the camera rays, "
          f"their trace for materials, the frame's torch ops and a second fw_denoise resolve")
    assert res.linear.max() > 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("split", "paths", "probe_lit"))
    ap.add_argument("--reps", type=int, default=None)
    opt = ap.parse_args()
    if opt.mode == "split":
        split(7 if opt.reps is None else opt.reps)
    elif opt.mode == "paths":
        paths(3 if opt.reps is None else opt.reps)
    else:
        probe_lit(7 if opt.reps is None else opt.reps)


if __name__ == "__main__":
    main()
