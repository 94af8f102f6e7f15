#!/usr/bin/env python3
"""Compare the compiled device code of the block-DFT kernels of two source trees, kernel by kernel (no GPU needed).

    scripts/blockdft_asm_diff.py OLD_TREE NEW_TREE

Each tree's block-DFT units (whichever of vqt_blockdft.hip, blockdft_gemm.hip, blockdft_dots.hip it has) are compiled with the
HIPFLAGS of its own Makefile plus -S --cuda-device-only, once without and once with -DPVQ_DEV_KNOBS.  The output is cut into
function bodies as tests/test_kernel_resources.py cuts it (label `_ZN3pvq...:` to `.Lfunc_end`); the per-function counters of local
labels (.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>, and the BB<n>_ of the loop comments) are replaced by a fixed string — they move when a
kernel before this one leaves the unit — together with the padding between a label and its comment, which follows the counter's
width; nothing else is normalised.  Prints, per flavour, the names on either side and whether each body is equal; exits 1 if
any body that both trees have differs."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

UNITS = ("vqt_blockdft.hip", "blockdft_gemm.hip", "blockdft_dots.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def hipflags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    return re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def bodies(tree, dev, tmp):
    csrc = os.path.join(tree, "pitchvis_amd", "csrc")
    out = {}
    for unit in UNITS:
        src = os.path.join(csrc, unit)
        if not os.path.exists(src):
            continue
        asm = os.path.join(tmp, unit + ".s")
        cmd = [HIPCC] + hipflags(csrc) + (["-DPVQ_DEV_KNOBS"] if dev else []) + ["-S", "--cuda-device-only", src, "-o", asm]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        inside = None
        for line in open(asm).read().splitlines():
            m = re.match(r"(_ZN3pvq\w+):", line)
            if m:
                inside = m.group(1)
                assert inside not in out, inside
                out[inside] = []
            elif line.startswith(".Lfunc_end"):
                inside = None
            elif inside:
                line = re.sub(r"(\.LBB|\bBB|\.Ltmp|\.Lfunc_begin)\d+", r"\1#", line)
                out[inside].append(re.sub(r"^(\.LBB#_\d+:)\s+;", r"\1 ;", line))
    return out


def main():
    old, new = sys.argv[1:3]
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for dev in (False, True):
            a, b = bodies(old, dev, tmp), bodies(new, dev, tmp)
            print("== %s build: old %d kernels, new %d kernels" % ("dev (-DPVQ_DEV_KNOBS)" if dev else "prod", len(a), len(b)))
            print("only in old: %s" % sorted(set(a) - set(b)))
            print("only in new: %s" % sorted(set(b) - set(a)))
            for k in sorted(set(a) & set(b)):
                same = a[k] == b[k]
                differ += not same
                print("  %s  lines %d  sha256 %s  %s" % (k, len(b[k]), hashlib.sha256("\n".join(b[k]).encode()).hexdigest()[:16], "equal" if same else "DIFFERS"))
            print("names compared: %d; bodies equal: %d" % (len(set(a) & set(b)), sum(a[k] == b[k] for k in set(a) & set(b))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
