#!/usr/bin/env python3
"""Compare the compiled device code of two source trees, kernel by kernel (no GPU needed).

    scripts/asm_diff.py [--by-name] OLD_TREE NEW_TREE [UNIT.hip ...]

The units are every *.hip under pitchvis_amd/csrc that either tree has, or the ones named (the block-DFT path alone:
vqt_blockdft.hip blockdft_gemm.hip blockdft_dots.hip).  Each is compiled with the
HIPFLAGS of its own tree's Makefile plus -S --cuda-device-only, once without and once with -DPVQ_DEV_KNOBS.  The output is cut into
function bodies as tests/test_kernel_resources.py cuts it (label `_ZN3pvq...:` to `.Lfunc_end`); the per-function counters of local
labels (.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>, and the BB<n>_ of the loop comments) are replaced by a fixed string — they move when a
kernel before this one leaves the unit — together with the padding between a label and its comment, which follows the counter's
width; nothing else is normalised.  Prints, per flavour, the (unit, name) pairs on either side and whether each body is equal;
exits 1 if any body that both trees have differs, or if the two sides' names differ.

--by-name keys a body by its mangled name alone, for a change that moves kernels from one unit to another (a unit split): keyed by
(unit, name) a moved kernel shows up as "only in old" and "only in new" and is never compared.  In that mode a name that occurs in
two units of one tree is an error (which of the two bodies would be the kernel's?); the unit printed is the new tree's."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def hipflags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    return re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def csrc_of(tree):
    return os.path.join(tree, "pitchvis_amd", "csrc")


def bodies(tree, units, dev, tmp):
    csrc = csrc_of(tree)
    out = {}
    units = [u for u in units if os.path.exists(os.path.join(csrc, u))]

    def compile_unit(unit):
        cmd = [HIPCC] + hipflags(csrc) + (["-DPVQ_DEV_KNOBS"] if dev else [])
        subprocess.run(cmd + ["-S", "--cuda-device-only", os.path.join(csrc, unit), "-o", os.path.join(tmp, unit + ".s")], check=True, stderr=subprocess.DEVNULL)

    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(compile_unit, units))
    for unit in units:
        asm = os.path.join(tmp, unit + ".s")
        inside = None
        for line in open(asm).read().splitlines():
            m = re.match(r"(_ZN3pvq\w+):", line)
            if m:
                inside = (unit, m.group(1))
                assert inside not in out, inside
                out[inside] = []
            elif line.startswith(".Lfunc_end"):
                inside = None
            elif inside:
                line = re.sub(r"(\.LBB|\bBB|\.Ltmp|\.Lfunc_begin)\d+", r"\1#", line)
                out[inside].append(re.sub(r"^(\.LBB#_\d+:)\s+;", r"\1 ;", line))
    return out


def by_name(tree, out):
    """(unit, name) -> body as name -> (unit, body); exits if two units of the tree hold one name"""
    named = {}
    for (unit, name), body in sorted(out.items()):
        if name in named:
            sys.exit("%s: kernel %s occurs in two units, %s and %s" % (tree, name, named[name][0], unit))
        named[name] = (unit, body)
    return named


def main():
    args = sys.argv[1:]
    named = "--by-name" in args
    args = [a for a in args if a != "--by-name"]
    old, new = args[:2]
    units = args[2:] or sorted({f for t in (old, new) for f in os.listdir(csrc_of(t)) if f.endswith(".hip")})
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for dev in (False, True):
            a, b = bodies(old, units, dev, tmp), bodies(new, units, dev, tmp)
            if named:   # both sides under the unit the new tree has the kernel in (the old tree's, for a name only the old tree has)
                an, bn = by_name(old, a), by_name(new, b)
                a = {((bn.get(n) or an[n])[0], n): body for n, (_, body) in an.items()}
                b = {(unit, n): body for n, (unit, body) in bn.items()}
            differ += set(a) != set(b)
            print("== %s build: old %d kernels, new %d kernels" % ("dev (-DPVQ_DEV_KNOBS)" if dev else "prod", len(a), len(b)))
            print("new tree, kernels per unit: %s" % ", ".join("%s %d" % (u, sum(k[0] == u for k in b)) for u in units if os.path.exists(os.path.join(csrc_of(new), u))))
            print("only in old: %s" % sorted(set(a) - set(b)))
            print("only in new: %s" % sorted(set(b) - set(a)))
            for k in sorted(set(a) & set(b)):
                same = a[k] == b[k]
                differ += not same
                print("  %s %s  lines %d  sha256 %s  %s" % (k[0], k[1], len(b[k]), hashlib.sha256("\n".join(b[k]).encode()).hexdigest()[:16], "equal" if same else "DIFFERS"))
            print("names compared: %d; bodies equal: %d" % (len(set(a) & set(b)), sum(a[k] == b[k] for k in set(a) & set(b))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
