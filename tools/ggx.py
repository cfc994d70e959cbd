"""GgxMat (FW_MAT_GGX): what its kernels cost and what they show.

    python tools/ggx.py [--repeats 5] [--out profiles/ggx.txt]

Cost: cornell 512x512 @1024 with its two boxes switched to GgxMat (roughness 0.3) against plain cornell, both under FW_FLAG_LIGHT_SAMPLING:
each case rendered once to warm up and then `--repeats` times under FW_FLAG_TIME_KERNELS, the cases alternated inside one process (the shade
kernels' speed differs from process to process, so separate runs are never compared); min / median / max of device time.
Demonstration: scenes/ggx_lights.yml from the command line's camera at 480x270: the RMSE of a 64-spp frame against a 16 384-spp frame of
itself, and the same scene with every GgxMat replaced by a MetalMat of equal albedo and roughness at 16 384 spp: an image difference (the
highlights MetalMat cannot show), not a noise figure."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def with_flags(r, flags, **settings):
    from firework_amd.api import Renderer
    rr = Renderer.default()
    rr.settings = dict(r.settings)
    rr.settings.update(settings)
    rr._camera = r._camera
    rr.settings["flags"] = flags
    return rr


def cost(opt):
    from firework_amd import _abi as A
    from firework_amd import _lib, scenes
    from firework_amd.api import GgxMat
    LS, TIME = A.FW_FLAG_LIGHT_SAMPLING, A.FW_FLAG_TIME_KERNELS
    scene, r = scenes.config("C2_cornell_box", 512, 512, 1024)
    plain = _lib.DeviceScene(scene.to_desc())
    g = scene.add_material(GgxMat.new((0.73, 0.73, 0.73), 0.3))
    for ro in scene.render_objects[6:8]:
        ro.obj.material = g
    glossy = _lib.DeviceScene(scene.to_desc())
    cases = [("plain cornell, bit 4", plain), ("GgxMat boxes, bit 4", glossy)]
    rows = {name: [] for name, _ in cases}
    for name, ds in cases:
        ds.render(with_flags(r, LS | TIME))
    for _ in range(opt.repeats):
        for name, ds in cases:
            st = ds.render(with_flags(r, LS | TIME)).stats
            rows[name].append((st["ms_render"], st["ms_extend"], st["ms_shade"], st["rays"]))
    lines = [f"cornell 512x512 @1024 under FW_FLAG_LIGHT_SAMPLING, {opt.repeats} timed frames per case, alternated in one process (ms of device time:",
             "min / median / max; ms_extend and ms_shade are sums over the two lanes, which overlap)", "",
             f"{'case':22s} {'ms_render':>26s} {'ms_extend (median)':>20s} {'ms_shade (median)':>20s} {'rays':>14s}"]
    med = {}
    for name, _ in cases:
        t = sorted(x[0] for x in rows[name])
        e = sorted(x[1] for x in rows[name])[len(t) // 2]
        s = sorted(x[2] for x in rows[name])[len(t) // 2]
        med[name] = t[len(t) // 2]
        lines.append(f"{name:22s} {t[0]:8.2f} /{t[len(t) // 2]:8.2f} /{t[-1]:8.2f} {e:20.2f} {s:20.2f} {rows[name][0][3]:14d}")
    a, b = med["GgxMat boxes, bit 4"], med["plain cornell, bit 4"]
    lines += ["", f"GgxMat boxes / plain cornell: {a / b:.3f}x of the frame's device time (medians {a:.2f} against {b:.2f} ms); the two frames trace",
              "different paths (a glossy box scatters elsewhere and ends some paths), so the ratio is of frames, not of kernels alone"]
    return lines


def demo(opt):
    from firework_amd import _lib, yaml_io
    from firework_amd.api import CameraSettings, GgxMat, MetalMat, Renderer
    W, H = 480, 270
    cam = CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().width(W).height(H).samples(64).use_bvh(True).camera(cam)
    scene = yaml_io.load_scene(os.path.join(ROOT, "scenes", "ggx_lights.yml"))
    ds = _lib.DeviceScene(scene.to_desc())
    ref = ds.render(with_flags(r, 0, samples=16384, seed=99)).linear.astype(np.float64)
    low = ds.render(with_flags(r, 0, samples=64, seed=1)).linear.astype(np.float64)
    scene.materials = [MetalMat.new(m.albedo, m.roughness) if isinstance(m, GgxMat) else m for m in scene.materials]
    metal = _lib.DeviceScene(scene.to_desc()).render(with_flags(r, 0, samples=16384, seed=99)).linear.astype(np.float64)
    rmse = float(np.sqrt(np.mean((low - ref) ** 2)))
    lum = lambda im: im.mean(-1)
    diff = lum(ref) - lum(metal)
    on = lum(ref) > 4.0 * np.median(lum(ref))                    # the highlight pixels of the GgxMat frame
    return ["", f"scenes/ggx_lights.yml, {W}x{H}, the command line's camera:",
            f"  64 spp against 16 384 spp of itself: RMSE {rmse:.4f} (mean luminance of the reference {lum(ref).mean():.4f})",
            f"  GgxMat against MetalMat of equal albedo and roughness, both at 16 384 spp (an image difference, not noise): mean luminance {lum(ref).mean():.4f} against "
            f"{lum(metal).mean():.4f}; brightest pixel {lum(ref).max():.2f} against {lum(metal).max():.2f}; {int(on.sum())} pixels of the GgxMat frame are above 4 x its",
            f"  median luminance (the highlights), and over them the MetalMat frame is lower by {diff[on].mean():.3f} on average ({lum(ref)[on].mean():.3f} against {lum(metal)[on].mean():.3f});",
            f"  RMS difference of the two frames {float(np.sqrt(np.mean((ref - metal) ** 2))):.4f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["cost", "demo"], default=None)
    opt = ap.parse_args()
    lines = []
    if opt.only != "demo":
        lines += cost(opt)
    if opt.only != "cost":
        lines += demo(opt)
    print("\n".join(lines))
    with open(opt.out or os.path.join(ROOT, "profiles", "ggx.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
