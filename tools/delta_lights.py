"""Delta-light cost (fw_scene_set_lights): device time of cornell 512x512 @1024 with one point light added (no flag: the lights
alone, one shadow ray per Lambertian vertex) against the FW_FLAG_LIGHT_SAMPLING frame of plain cornell, which has the same frame layout and
also casts one shadow ray per vertex; and of both together (bit 4 with the point light).

    python tools/delta_lights.py [--repeats 5] [--out profiles/delta_lights.txt]
        every case rendered once to warm up and then `--repeats` times under FW_FLAG_TIME_KERNELS, the cases alternated inside one process, so
        that the spread of a case's own repeats is on the page.  Writes the table, and nothing else, to --out.
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/delta_lights.py --phases [--frames 3]
        no timing flags: `--frames` frames of bit 4 on plain cornell, then as many of the point light alone, in ONE process (the shade
        kernels' speed differs from process to process on some machines, so two runs of their own cannot be compared).
    python tools/delta_lights.py --trace DIR/.../NAME_kernel_trace.csv [--out profiles/delta_lights_trace.txt]
        per-kernel totals of that trace for each of the two phases: the second phase starts at the first k_raygen after the last k_shade_ls."""
import argparse
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINT_POS, POINT_I = (278.0, 400.0, 278.0), (60000.0, 50000.0, 40000.0)


def frame(ds, r, flags):
    from firework_amd.api import Renderer
    rr = Renderer.default()
    rr.settings = dict(r.settings)
    rr._camera = r._camera
    rr.settings["flags"] = flags
    return ds.render(rr)


def scenes_pair():
    from firework_amd import _lib, scenes
    from firework_amd.api import PointLight
    scene, r = scenes.config("C2_cornell_box", 512, 512, 1024)
    plain = _lib.DeviceScene(scene.to_desc())
    lit = _lib.DeviceScene(scene.to_desc())
    lit.set_lights([PointLight(POINT_POS, POINT_I)])
    return plain, lit, r


def timed(opt):
    from firework_amd import _abi as A
    LS, TIME = A.FW_FLAG_LIGHT_SAMPLING, A.FW_FLAG_TIME_KERNELS
    plain, lit, r = scenes_pair()
    cases = [("default, no lights", plain, 0), ("bit 4, no lights", plain, LS), ("point light alone", lit, 0), ("bit 4 + point light", lit, LS)]
    rows = {name: [] for name, _, _ in cases}
    for name, ds, fl in cases:
        frame(ds, r, fl | TIME)
    for _ in range(opt.repeats):
        for name, ds, fl in cases:
            st = frame(ds, r, fl | TIME).stats
            rows[name].append((st["ms_render"], st["ms_extend"], st["ms_shade"]))
    lines = [f"cornell 512x512 @1024, {opt.repeats} timed frames per case, alternated in one process (ms of device time: min / median / max;",
             "ms_extend and ms_shade are sums over the two lanes, which overlap)", "",
             f"{'case':22s} {'ms_render':>26s} {'ms_extend (median)':>20s} {'ms_shade (median)':>20s}"]
    med = {}
    for name, _, _ in cases:
        t = sorted(x[0] for x in rows[name])
        e = sorted(x[1] for x in rows[name])[len(t) // 2]
        s = sorted(x[2] for x in rows[name])[len(t) // 2]
        med[name] = (t[len(t) // 2], t[0], t[-1])
        lines.append(f"{name:22s} {t[0]:8.2f} /{t[len(t) // 2]:8.2f} /{t[-1]:8.2f} {e:20.2f} {s:20.2f}")
    a, b = med["point light alone"], med["bit 4, no lights"]
    lines += ["", f"point light alone / bit 4 without lights: {a[0] / b[0]:.3f}x (median {a[0]:.2f} against {b[0]:.2f} ms; the bit-4 frame's own repeats span "
              f"{b[1]:.2f} .. {b[2]:.2f} ms)"]
    return lines


def phases(opt):
    from firework_amd import _abi as A
    plain, lit, r = scenes_pair()
    for ds, fl in ((plain, A.FW_FLAG_LIGHT_SAMPLING), (lit, 0)):
        for _ in range(opt.frames):
            frame(ds, r, fl)
    return None


def trace(opt):
    rows = list(csv.DictReader(open(opt.trace)))
    col = lambda key: next(c for c in rows[0] if key in c.lower())          # (column names differ a little between profiler versions)
    cn, cs, ce = col("kernel_name"), col("start"), col("end")
    name = lambda r: re.sub(r"^void |\(.*", "", r[cn])
    start, end = (lambda r: int(r[cs])), (lambda r: int(r[ce]))
    last_ls = max(start(r) for r in rows if name(r).startswith("fw::k_shade_ls"))
    cut = min(start(r) for r in rows if name(r).startswith("fw::k_raygen") and start(r) > last_ls)
    tot = [{}, {}]
    for r in rows:
        d = tot[start(r) >= cut]
        c = d.setdefault(name(r), [0, 0])
        c[0] += 1
        c[1] += end(r) - start(r)
    lines = ["rocprofv3 --kernel-trace of `tools/delta_lights.py --phases`: cornell 512x512 @1024, the frames of bit 4 on plain cornell and then as many of",
             "one point light without a flag, in one process; per-kernel totals of each phase (kernels above 0.5 % of their phase)", ""]
    for k, label in enumerate(("bit 4, no lights", "point light alone")):
        all_ns = sum(v[1] for v in tot[k].values())
        lines.append(f"{label}: all kernels {all_ns / 1e6:.2f} ms")
        for n, (calls, ns) in sorted(tot[k].items(), key=lambda x: -x[1][1]):
            if ns >= 0.005 * all_ns:
                lines.append(f"  {n:46s} calls {calls:5d}  total {ns / 1e6:9.2f} ms  {100 * ns / all_ns:5.1f} %")
        lines.append("")
    return lines[:-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    lines = phases(opt) if opt.phases else trace(opt) if opt.trace else timed(opt)
    if lines is None:
        return
    out = opt.out or os.path.join(ROOT, "profiles", "delta_lights_trace.txt" if opt.trace else "delta_lights.txt")
    print("\n".join(lines))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
