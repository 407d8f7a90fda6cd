#!/usr/bin/env python3
"""usage: tools/kernel_compare.py parent.s new.s  -> per-kernel comparison of two device-only assembly files of dmx_engine.hip
(tools/kernel_resources.sh leaves one under /tmp/dmx_asm; build the other from the parent commit's source the same way).

Hard figures, which a refactor of device code must leave equal for every kernel: vgpr_count, vgpr_spill_count, sgpr_count,
group_segment_fixed_size, private_segment_fixed_size (the code object's metadata) and the number of v_*_f64 instructions.
Reported: every kernel whose histogram of mnemonics differs, with the differing mnemonics and counts.  Counts and metadata only —
registers are renamed and moves reordered by any edit, so the text of the two files is not compared.  Exit status 1 when a hard
figure differs or a kernel is missing on either side."""
import collections
import re
import subprocess
import sys

HARD = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    txt = open(path).read()
    md = txt[txt.index("amdhsa.kernels:"):]
    out = {}
    for blk in md.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in HARD}
    body = txt[:txt.index("amdhsa.kernels:")]
    for name, rec in out.items():
        m = re.search(rf"^{re.escape(name)}:.*?^\.Lfunc_end\d+:", body, re.S | re.M)
        hist = collections.Counter()
        for line in m.group(0).split("\n")[1:]:
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                hist[line.split()[0]] += 1
        rec["hist"] = hist
        rec["f64"] = sum(n for mn, n in hist.items() if mn.startswith("v_") and "_f64" in mn)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "") for n, d in zip(names, res)}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    dem = demangle(sorted(set(a) | set(b)))
    bad = 0
    for n in sorted(set(a) ^ set(b)):
        print(f"MISSING {'in new' if n in a else 'in parent'}: {dem[n]}")
        bad += 1
    differ = 0
    for n in sorted(set(a) & set(b), key=lambda n: dem[n]):
        ka, kb = a[n], b[n]
        hard = [f"{k} {ka[k]} -> {kb[k]}" for k in HARD + ("f64",) if ka[k] != kb[k]]
        if hard:
            bad += 1
            print(f"HARD {dem[n]}: " + ", ".join(hard))
        if ka["hist"] != kb["hist"]:
            differ += 1
            d = [f"{mn} {ka['hist'][mn]} -> {kb['hist'][mn]}" for mn in sorted(set(ka["hist"]) | set(kb["hist"]))
                 if ka["hist"][mn] != kb["hist"][mn]]
            print(f"hist {dem[n]}: " + ", ".join(d))
    print(f"{len(set(a) & set(b))} kernels compared; {bad} with a hard difference; {differ} with a differing histogram")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
