"""Dev helper: the gfx950 assembly of the lane-per-task units, kernel by kernel, of two trees side by side.

    python3 tools/simt_isa_diff.py PARENT_TREE [CHANGE_TREE] > profiles/<name>_isa.txt

Compiles csrc/simt_kernel.hip and csrc/simt_factor_ahead.hip of both trees with the Makefile's flags plus --cuda-device-only -S
and prints, per kernel instantiation of the parent (those only the change has are listed with their resources): VGPRs, AGPRs, scratch, occupancy and code length of both, the difference of the mnemonic
histograms, and whether the sequence of s_waitcnt instructions (with their operands) is the same.  No GPU needed."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

UNITS = ("simt_kernel.hip", "simt_factor_ahead.hip")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from resource_util import makefile_flags  # noqa: E402  (the flags of this tree's Makefile, for both trees)

FIELDS = (("VGPRs", "NumVgprs"), ("AGPRs", "NumAgprs"), ("scratch", "ScratchSize"), ("occupancy", "Occupancy"), ("bytes", "codeLenInByte"))


def kernels_of(tree, unit, tmp):
    csrc = os.path.join(tree, "slam_plus_plus_amd", "csrc")
    path = os.path.join(tmp, "x.s")
    subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + makefile_flags(UNITS) + ["--cuda-device-only", "-S", "-o", path, os.path.join(csrc, unit)], check=True)
    kernels, name = {}, None
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
            kernels[name] = {"hist": collections.Counter(), "waits": []}
            continue
        if name is None:
            continue
        k = kernels[name]
        m = re.match(r"\s*; (\w+)(?:: | = )(\d+)\s*$", line)
        if m:
            k[m.group(1)] = int(m.group(2))
            continue
        if re.match(r"\s*\.(section|text)\b", line) and "codeLenInByte" in k:
            name = None
            continue
        m = re.match(r"\s+([a-z]\w+)\b(.*)", line)
        if m and "codeLenInByte" not in k:
            k["hist"][m.group(1)] += 1
            if m.group(1) == "s_waitcnt":
                k["waits"].append(m.group(2).split(";")[0].strip())
    return {n: k for n, k in kernels.items() if "codeLenInByte" in k and k.get("Occupancy") is not None and "_simt_" in n}


def demangled(names):
    """_ZN6slampp18factor_simt_kernelILi6ELi32ELi2ELb0EEEv... -> factor_simt_kernel<6,32,2,false> (integer and bool arguments only)"""
    out = {}
    for n in names:
        m = re.match(r"_ZN6slampp(\d+)", n)
        rest = n[m.end():]
        kernel, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
        args = re.match(r"I((?:L[ib]\d+E)+)E", rest)
        out[n] = kernel + "<" + ",".join(v if t == "i" else ("false", "true")[int(v)] for t, v in re.findall(r"L([ib])(\d+)E", args.group(1))) + ">" if args else n
    return out


def main():
    parent = sys.argv[1]
    change = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n_diff = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:
            a, b = kernels_of(parent, unit, tmp), kernels_of(change, unit, tmp)
            assert set(a) <= set(b), sorted(set(a) - set(b))    # (a change may add kernels: listed behind the others)
            names = demangled(sorted(b))
            print(f"== {unit}: {len(a)} kernels" + (f", {len(b) - len(a)} new" if len(b) > len(a) else ""))
            for n in sorted(set(b) - set(a), key=lambda n: names[n]):
                kb = b[n]
                print(f"{names[n]}  (new)\n    " + "  ".join(f"{label} {kb[key]}" for label, key in FIELDS)
                      + f"\n    instructions {sum(kb['hist'].values())}; s_waitcnt sequence ({len(kb['waits'])})")
            for n in sorted(a, key=lambda n: names[n]):
                ka, kb = a[n], b[n]
                res = "  ".join(f"{label} {ka[key]}" + ("" if ka[key] == kb[key] else f" -> {kb[key]}") for label, key in FIELDS)
                hist = {m: kb["hist"][m] - ka["hist"][m] for m in sorted(set(ka["hist"]) | set(kb["hist"])) if kb["hist"][m] != ka["hist"][m]}
                waits = "the same" if ka["waits"] == kb["waits"] else f"DIFFERENT ({len(ka['waits'])} -> {len(kb['waits'])})"
                print(f"{names[n]}\n    {res}\n    instructions {sum(ka['hist'].values())} -> {sum(kb['hist'].values())}, histogram "
                      + ("the same" if not hist else "differs: " + ", ".join(f"{m} {d:+d}" for m, d in hist.items()))
                      + f"; s_waitcnt sequence ({len(ka['waits'])}) {waits}")
                n_diff += bool(hist) or ka["waits"] != kb["waits"] or any(ka[key] != kb[key] for _, key in FIELDS)
    print(f"== {n_diff} kernels differ in one of these")


if __name__ == "__main__":
    main()
