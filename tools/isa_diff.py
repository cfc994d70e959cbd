"""Do two versions of fw_kernels.hip compile to the same kernels?   python tools/isa_diff.py OLD NEW [compiler flags, e.g. -DFW_AB=1]

OLD and NEW are source trees (their firework_amd/csrc/fw_kernels.hip is compiled device-only to assembly under /tmp, with the Makefile's
flags plus the extra ones, as tools/kernel_regs.py does) or .s files that were compiled already.  Every kernel's instruction stream
(comments and directives stripped, local labels renumbered in order of appearance) and its register / spill / LDS / scratch counts are
compared whole; nothing is searched for.  Prints one line per kernel, `same` or `differs` with the counts of both sides, and exits 1 if a
kernel differs or the two sets of kernels differ.  A refactoring that must not change the shipped kernels is checked with
    git worktree add /tmp/fw_parent HEAD~1 && python tools/isa_diff.py /tmp/fw_parent . && python tools/isa_diff.py /tmp/fw_parent . -DFW_AB=1"""
import os, re, shutil, subprocess, sys, tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only"]
COUNTS = ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def assembly(path, extra, tag):
    if os.path.isfile(path):
        return open(path).read()
    out = os.path.join(tempfile.gettempdir(), f"fw_isa_diff_{tag}.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-o", out, os.path.join(path, "firework_amd/csrc/fw_kernels.hip")] + extra, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{symbol: (instruction lines, {count name: value})} of every kernel in one assembly file"""
    meta = {}
    for block in re.split(r"\n  - \.agpr_count:", text[text.find("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\n\s+\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\n\s+\.{k}:\s+(\d+)", block).group(1)) for k in COUNTS}
    out = {}
    for name in meta:
        body = text[text.index(f"\n{name}:") + 1:text.index(f"\t.amdhsa_kernel {name}\n")]
        labels, lines = {}, []
        for line in body.split("\n")[1:]:
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue
            lines.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), line))
        out[name] = (lines, meta[name])
    return out


def n_instr(lines):
    return sum(not l.endswith(":") for l in lines)


def show(name, filt):
    if filt:
        name = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip() or name
    return re.sub(r"^void |\(.*", "", name)


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    extra = sys.argv[3:]
    a, b = kernels(assembly(sys.argv[1], extra, "old")), kernels(assembly(sys.argv[2], extra, "new"))
    filt = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin" + os.pathsep + os.environ.get("PATH", "")) or shutil.which("c++filt")
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{show(name, filt):60s} only in {'OLD' if name in a else 'NEW'}")
            bad += 1
        elif a[name] == b[name]:
            print(f"{show(name, filt):60s} same     {n_instr(a[name][0])} instructions")
        else:
            (la, ma), (lb, mb) = a[name], b[name]
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"{show(name, filt):60s} differs  instructions {n_instr(la)} -> {n_instr(lb)} (first difference at line {first} of the stream)  " +
                  "  ".join(f"{k} {ma[k]} -> {mb[k]}" for k in COUNTS))
            bad += 1
    print(f"{len(set(a) | set(b))} kernels ({len(a)} old, {len(b)} new), flags {' '.join(extra) or '(none)'}: {len(set(a) | set(b)) - bad} same, {bad} differ or are missing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
