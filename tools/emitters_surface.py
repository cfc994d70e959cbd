"""Measurements of every emitter sampled at surface points (fw_bake_emitters, FW_GATHER_NO_EMITTERS); the results are
kept in profiles/emitters_surface.txt.  Nothing here is a gate.

    python tools/emitters_surface.py [--reps N] [--samples S] [--parts abcd]
        (a) One lamp: fw_render_aovs' records of a 1920 x 1080 cornell frame stay on the device; fw_bake_emitters and fw_bake_area at
            S = 16 alternated on them with one round under FW_FLAG_TIME_KERNELS (rays = ms_raygen, walks = ms_extend, after the trace =
            ms_accumulate); run 0 warms both up, then N (default 3) runs each.  The rays are the same: the difference is the CDF search
            and the picked-record gather.
        (b) Many lights: tools/all_emitters.py's one bright sphere among 100 dim ones, 512 x 512 records; fw_bake_area at S = 1 (101
            rays per point) beside fw_bake_emitters at S = 101 (the same rays per point): device time, and RMSE of E against
            fw_bake_emitters at 64 x the rays with another seed; the equal-time RMSE is derived (RMSE x sqrt(time ratio)).
        (c) The final-gather split on tools/all_emitters.py's cornell with a 512-triangle mesh lamp, 256 x 256 against fw_render at 4096
            spp: the plain preview, --probe-gather 64, --probe-gather 64 --emitter-light 16, with and without the lamp's own pixels.
        (d) The search: k_emitters_rays over resident records and CDF (fw_bake_emitters' ms_raygen under FW_FLAG_TIME_KERNELS) for a mesh
            lamp of N = 1, 10^3 and 10^6 triangles, 2^17 points x 16 samples.  Run once with the product library (the LDS coarse table)
            and once with the A/B build and FIREWORK_EMITTERS_PLAIN_SEARCH=1 (one binary search over the whole CDF in global memory).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from firework_amd import _abi as A  # noqa: E402
from firework_amd import _lib, api, scenes  # noqa: E402

W, H = 1920, 1080


def timed(name, st):
    print(f"{name}: ms_render {st['ms_render']:.2f} (rays {st['ms_raygen']:.2f}, walks {st['ms_extend']:.2f}, after the trace "
          f"{st['ms_accumulate']:.2f}), wall {st['ms_wall']:.2f}, rays traced {st['rays']}, batches {st['n_batches']}")


def part_a(opt, torch, dev):
    S = opt.samples
    scene, r = scenes.config("C2_cornell_box", W, H, 1)
    r.seed(3)
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rec, _codes = ds.emitters()
        print(f"(a) entries: {rec.shape[0]} (kinds {rec[:, 1].astype(int).tolist()}); sampled lights: {ds.area_lights().shape[0]}")
        aov = torch.empty((W * H, 12), dtype=torch.float32, device=dev)
        ds.aovs(r, 1, out=aov)
        print(f"records: {W} x {H} cornell, {int((aov[:, 3] > 0).sum())} pixels on surfaces, 1 round, FW_FLAG_TIME_KERNELS")
        kw = dict(rounds=1, seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"] | A.FW_FLAG_TIME_KERNELS)
        pos, nrm = aov[:, 8:11], aov[:, 4:7]
        for k in range(opt.reps + 1):
            oa, _s, st = ds.bake_area(api.AreaLight(S, 0.5).seed(1), pos, nrm, None, **kw)
            timed(f"run {k} fw_bake_area S={S}    ", st)
            oe, _s, st = ds.bake_emitters(api.EmitterLights(S, 0.5).seed(1), pos, nrm, None, **kw)
            timed(f"run {k} fw_bake_emitters S={S}", st)
        print(f"the two outs equal bit for bit: {bool(torch.equal(oa.view(torch.int32), oe.view(torch.int32)))}")
    finally:
        ds.close()


def part_b(opt, torch, dev):
    import all_emitters
    scene, r = all_emitters.spheres(512, 512, 1)
    r.seed(3)
    s = r.settings
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        rec, _codes = ds.emitters()
        Ln = ds.area_lights().shape[0]
        aov = torch.empty((512 * 512, 12), dtype=torch.float32, device=dev)
        ds.aovs(r, 1, out=aov)
        on = (aov[:, 3] > 0).cpu().numpy()
        pos, nrm = aov[:, 8:11], aov[:, 4:7]
        kw = dict(seed=s["seed"], use_bvh=s["use_bvh"], flags=s["flags"] | A.FW_FLAG_TIME_KERNELS)
        ref, _s, _st = ds.bake_emitters(api.EmitterLights(64 * Ln, 1e-3).seed(77), pos, nrm, None, rounds=1, **kw)
        ref = ref.cpu().numpy()[on][:, 0:3].astype(np.float64)
        print(f"(b) {Ln} sampled lights, {rec.shape[0]} entries, 512 x 512 records, {int(on.sum())} pixels on surfaces; reference: fw_bake_emitters at "
              f"{64 * Ln} rays per point, seed 77; mean E {ref.mean():.4f}")
        rows = []
        for k in range(opt.reps + 1):
            oa, _s, sa = ds.bake_area(api.AreaLight(1, 1e-3).seed(1), pos, nrm, None, rounds=1, **kw)
            timed(f"run {k} fw_bake_area S=1 ({Ln} rays per point)      ", sa)
            oe, _s, se = ds.bake_emitters(api.EmitterLights(Ln, 1e-3).seed(1), pos, nrm, None, rounds=1, **kw)
            timed(f"run {k} fw_bake_emitters S={Ln} ({Ln} rays per point)", se)
            rows.append((sa["ms_render"], se["ms_render"]))
        rm = lambda o: float(np.sqrt(np.mean((o.cpu().numpy()[on][:, 0:3].astype(np.float64) - ref) ** 2)))
        ta, te = np.median([x[0] for x in rows[1:]]), np.median([x[1] for x in rows[1:]])
        ra, re_ = rm(oa), rm(oe)
        print(f"RMSE of E: fw_bake_area {ra:.5f} in {ta:.2f} ms, fw_bake_emitters {re_:.5f} in {te:.2f} ms")
        print(f"derived, not measured: at fw_bake_area's time fw_bake_emitters' RMSE would be {re_ * np.sqrt(te / ta):.5f} (RMSE x sqrt(time ratio))")
    finally:
        ds.close()


def part_c(opt, torch, dev):
    import all_emitters
    S = opt.samples
    scene, r = all_emitters.mesh_cornell(256, 256, 4096, 16)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        probes = api.ProbeSet.grid((30.0, 30.0, 30.0), (525.0, 525.0, 525.0), (6, 6, 6), 256)
        baker = api.Renderer.default().samples(16).use_bvh(True).seed(1)
        sh, _sums = baker.bake_probes(ds, probes, 4)
        pd = api.ProbeDepth(16, 6, 800.0)
        moments, _dsums = baker.bake_probe_depth(ds, probes, pd, 4)
        full = np.asarray(ds.render(r).linear).reshape(-1, 3).astype(np.float64)
        ref, lamp = np.clip(full, 0.0, 1.0), np.any(full >= 1.0, axis=1)
        kw = dict(aov_samples=8, depth=pd, moments=moments, normal_bias=2.0)
        g = api.FinalGather(64, 1e-3).seed(0)
        frames = [("--probe-lit", {}), ("--probe-lit --probe-gather 64", dict(gather=g)),
                  (f"--probe-lit --probe-gather 64 --emitter-light {S}", dict(gather=g, emitters=api.EmitterLights(S, 1e-3).seed(0)))]
        print(f"(c) cornell with a {ds.emitters()[0].shape[0]}-triangle mesh lamp; RMSE against fw_render 256 x 256 at 4096 spp, linear frames clipped to "
              f"[0, 1] (and without the {int(lamp.sum())} pixels where the reference is >= 1):")
        for name, extra in frames:
            lit = np.clip(r.render_probe_lit(ds, probes, sh, **kw, **extra).linear.reshape(-1, 3).astype(np.float64), 0.0, 1.0)
            print(f"  {name:52s} {float(np.sqrt(np.mean((lit - ref) ** 2))):.4f}   ({float(np.sqrt(np.mean((lit[~lamp] - ref[~lamp]) ** 2))):.4f})")
    finally:
        ds.close()


def part_d(opt, torch, dev):
    """k_emitters_rays over resident records and CDF: fw_bake_emitters' ms_raygen under FW_FLAG_TIME_KERNELS on a floor under a mesh lamp of
    N triangles.  Which search runs is the library's: the product has the LDS coarse table; the A/B build (FIREWORK_LIB=.../lib_ab.so)
    with FIREWORK_EMITTERS_PLAIN_SEARCH set runs one binary search over the whole CDF in global memory instead."""
    from firework_amd.api import EmissiveMat, LambertianMat, RenderObject, Scene, TriangleMesh, XZRect
    rng = np.random.default_rng(1)
    n, S = 1 << 17, 16
    pos = torch.from_numpy(np.stack([rng.uniform(-8, 8, n), np.zeros(n), rng.uniform(-8, 8, n)], 1).astype(np.float32)).to(dev)
    nrm = torch.from_numpy(np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (n, 1))).to(dev)
    which = ("plain global search" if os.environ.get("FIREWORK_EMITTERS_PLAIN_SEARCH") else "LDS coarse table") + ", library " + os.path.basename(_lib.LIB_PATH if not os.environ.get("FIREWORK_LIB") else os.environ["FIREWORK_LIB"])
    print(f"(d) k_emitters_rays ({which}): {n} points x {S} samples = {n * S} entries per round, records and CDF resident, ms_raygen of fw_bake_emitters, median (min) of {opt.reps * 3} rounds:")
    for N in (1, 1000, 1000000):
        g = max(1, int(np.ceil(np.sqrt(N / 2.0))))
        xs = np.linspace(-4.0, 4.0, g + 1)
        X, Z = np.meshgrid(xs, xs, indexing="ij")
        verts = np.stack([X, np.full_like(X, 6.0), Z], -1).reshape(-1, 3).astype(np.float32)
        i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
        a, b = (i * (g + 1) + j).ravel(), ((i + 1) * (g + 1) + j).ravel()
        idx = np.stack([a, b, b + 1, a, b + 1, a + 1], -1).reshape(-1, 3)[:N].ravel().astype(np.uint32)
        scene = Scene.new()
        scene.add_object(RenderObject.new(XZRect.new(-10, 10, -10, 10, 0, scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5))))))
        scene.add_object(RenderObject.new(TriangleMesh(verts, idx, material=scene.add_material(EmissiveMat.with_color((5.0, 5.0, 5.0))))))
        ds = _lib.DeviceScene(scene.to_desc())
        try:
            em = api.EmitterLights(S, 1e-3).seed(1)
            ms = []
            for k in range(opt.reps * 3 + 1):
                out, _s, st = ds.bake_emitters(em, pos, nrm, None, rounds=1, first_round=0, flags=A.FW_FLAG_TIME_KERNELS)
                if k:
                    ms.append(st["ms_raygen"])
            print(f"  N = {ds.emitters()[0].shape[0]:7d}: rays {np.median(ms):.3f} ({min(ms):.3f}) ms, {n * S / np.median(ms) / 1e6:.2f} G entries/s; walks {st['ms_extend']:.2f} ms, "
                  f"mean E {float(out[:, 0].mean()):.4f}")
        finally:
            ds.close()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--parts", default="abcd")
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    for p, f in (("a", part_a), ("b", part_b), ("c", part_c), ("d", part_d)):
        if p in opt.parts:
            f(opt, torch, dev)


if __name__ == "__main__":
    main()
