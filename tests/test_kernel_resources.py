"""Occupancy guard for the hand-written kernels (no GPU needed: hipcc cross-compiles and reports register use).
The fused GEMM + tree kernel runs two 512-thread workgroups per CU = four waves per SIMD, which holds only up to 128
vector registers per lane; one register more silently halves its occupancy (measured: 0.36 -> 0.42 ms per launch)."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_register_budgets_of_the_block_dft_kernels(tmp_path):
    # the block-DFT path's three units (vqt_blockdft.hip: host side; blockdft_gemm.hip; blockdft_dots.hip), usage and bodies merged over them
    units = ("vqt_blockdft.hip", "blockdft_gemm.hip", "blockdft_dots.hip")
    usage = {}
    for unit in units:
        src = os.path.join(ROOT, "pitchvis_amd", "csrc", unit)
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage",
                            "-c", src, "-o", str(tmp_path / "x.o")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        name = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                assert name not in usage, name
                usage[name] = {}
            m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
            if m and name:
                usage[name][m.group(1).split(" ")[0]] = int(m.group(2))

    def find(sub):
        hits = [v for k, v in usage.items() if sub in k]
        assert hits, (sub, list(usage))
        return hits

    for u in find("blockdft_gemm_treeILi256") + find("blockdft_gemm_treeILi128") + find("blockdft_gemm_tree_bf16x3ILi256"):
        # two 512-thread workgroups per CU; a few dwords of the tile set-up (stream-edge variant) may spill, the K loop bodies may not
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128 and u["ScratchSize"] <= 64, u
    asm = tmp_path / "x.s"
    body, in_unit = {}, {}
    for unit in units:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                            os.path.join(ROOT, "pitchvis_amd", "csrc", unit), "-o", str(asm)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        inside = None
        in_unit[unit] = set()
        for line in asm.read_text().splitlines():
            m = re.match(r"(_ZN3pvq\w+):", line)
            if m:
                inside = m.group(1)
                assert inside not in body, inside
                body[inside] = []
                in_unit[unit].add(inside)
            elif line.startswith(".Lfunc_end"):
                inside = None
            elif inside:
                body[inside].append(line)
    # The product build holds exactly the kernels its dispatch can reach (launch_blockdft_gemm_fused / _gemm_unfused / _tree_finish in
    # blockdft_gemm.hip, launch_blockdft_dots in blockdft_dots.hip): the form that only a developer knob selects — the 16-bin kernel
    # product on 64-frame tiles (blockdft_banddots_db<MT = 2, NW = 8>) — compiles under -DPVQ_DEV_KNOBS alone.  (blockdft_gemm_tree3,
    # which was such a form too, has been removed.)
    reachable = {
        "_ZN3pvq18blockdft_gemm_treeILi256ELi256EEEvNS_12GemmTreeArgsE", "_ZN3pvq18blockdft_gemm_treeILi256ELi0EEEvNS_12GemmTreeArgsE",
        "_ZN3pvq18blockdft_gemm_treeILi128ELi0EEEvNS_12GemmTreeArgsE", "_ZN3pvq25blockdft_gemm_tree_bf16x3ILi256EEEvNS_12GemmTreeArgsE",
        "_ZN3pvq17blockdft_gemm_genILi256EEEvNS_12GemmTreeArgsE", "_ZN3pvq17blockdft_gemm_genILi128EEEvNS_12GemmTreeArgsE",
        "_ZN3pvq20blockdft_tree_finishENS_10FinishArgsE",
        "_ZN3pvq18blockdft_gemm_rowsILi256EEEvNS_8GemmArgsE",
        "_ZN3pvq16blockdft_combineILi128ELi16ELi64EEEvNS_11CombineArgsE", "_ZN3pvq16blockdft_combineILi128ELi16ELi256EEEvNS_11CombineArgsE",
        "_ZN3pvq22blockdft_banddots4c_dbILi8ELi4ELi260ELi2EEEvNS_8BandArgsE", "_ZN3pvq22blockdft_banddots4c_dbILi8ELi4ELi308ELi2EEEvNS_8BandArgsE",
        "_ZN3pvq22blockdft_banddots4c_dbILi8ELi4ELi372ELi1EEEvNS_8BandArgsE", "_ZN3pvq22blockdft_banddots4c_dbILi8ELi4ELi596ELi1EEEvNS_8BandArgsE",
        "_ZN3pvq22blockdft_banddots4c_dbILi8ELi4ELi852ELi1EEEvNS_8BandArgsE", "_ZN3pvq22blockdft_banddots4c_dbILi8ELi4ELi1028ELi1EEEvNS_8BandArgsE",
        "_ZN3pvq20blockdft_banddots_dbILi1ELi8EEEvNS_8BandArgsE",   # above 1 020 bins
        "_ZN3pvq27blockdft_banddots_db_bf16x3ILi2ELi4EEEvNS_8BandArgsE", "_ZN3pvq27blockdft_banddots_db_bf16x3ILi1ELi4EEEvNS_8BandArgsE",
    }
    assert set(body) == reachable, (sorted(set(body) - reachable), sorted(reachable - set(body)))
    assert not any("tree3" in k or "blockdft_banddots_dbILi2ELi8E" in k for k in body)
    # each stage's kernels in its own unit, none in the host unit
    assert in_unit["blockdft_gemm.hip"] == {k for k in reachable if "banddots" not in k} and len(in_unit["blockdft_gemm.hip"]) == 10
    assert in_unit["blockdft_dots.hip"] == {k for k in reachable if "banddots" in k} and len(in_unit["blockdft_dots.hip"]) == 9
    assert in_unit["vqt_blockdft.hip"] == set()
    checked = 0
    for name, lines in body.items():
        if "blockdft_gemm_treeILi" not in name and "blockdft_gemm_tree_bf16x3" not in name:   # the shipped kernels (not the opt-in experiments)
            continue
        blocks, cur = [], []
        for l in lines:
            if l.startswith(".LBB"):
                blocks.append(cur)
                cur = []
            cur.append(l)
        blocks.append(cur)
        with_mfma = [b for b in blocks if any("v_mfma" in l for l in b)]
        assert with_mfma, name
        for b in with_mfma:   # a basic block that issues matrix instructions (the K loop bodies) must not touch scratch
            assert not any(re.match(r"\s+scratch_", l) for l in b), (name, "scratch access inside the K loop", b[0])
        checked += 1
    assert checked >= 3
    # Every register written by a vector-memory load is covered by an s_waitcnt vmcnt before it is read, on every path, and every
    # LDS-DMA before the next barrier (tests/isa_vmcnt.py: a dataflow over the compiled code).  The K loop's operand prefetch used to
    # sit in a uniform `if`: not a correctness problem (the compiler then waits for MORE: vmcnt(4) / vmcnt(0) right after issuing
    # the loads, i.e. no prefetch distance at all), but round 2's removed split-in-registers loop showed wrong rows with that shape and
    # its cause was never found — so the shipped kernels' waits are now checked mechanically, and the hand-placed
    # `s_waitcnt vmcnt(8)` of the fp32 kernel's prologue with them.
    import isa_vmcnt
    n_checked = 0
    for name, lines in body.items():
        if "blockdft_" not in name:
            continue
        bad = isa_vmcnt.check(lines)
        assert not bad, (name, bad[:5])
        n_checked += 1
    assert n_checked >= 8
    # the fp32 K loops keep the operand loads of the NEXT stage in flight under the MFMAs of this one: a wait in a K loop body must never
    # cover the group of loads issued last before it (vmcnt(N), N >= that group's size: 8 loads per double k group in the 32-column
    # loop, 4 per stage in the 64-column one) — a wait for fewer means the loop runs without its prefetch distance
    for name, lines in body.items():
        if "blockdft_gemm_treeILi256ELi0" not in name:   # (the instantiation that knows its hop has its 32-column K loop fully unrolled: no loop body to look at; the dataflow check above covers it)
            continue
        blocks, cur = [], []
        for l in lines:
            t = l.split(";")[0].strip()
            if t.startswith(".LBB"):
                blocks.append(cur)
                cur = []
            elif t:
                cur.append(t)
        blocks.append(cur)
        hits, groups = 0, set()
        for b in blocks:   # a K loop body: issues operand loads and MFMAs, and loops back to itself
            n_loads = sum(t.startswith("buffer_load_dwordx4") for t in b)
            if n_loads < 8 or not any(t.startswith("v_mfma") for t in b) or not any(t.startswith("s_cbranch") for t in b):
                continue
            cyc = b + b   # (the loads at the end of the body precede the waits at its top)
            for i in range(len(b), len(cyc)):
                if not (cyc[i].startswith("s_waitcnt") and "vmcnt" in cyc[i]):
                    continue
                n = int(re.search(r"vmcnt\((\d+)\)", cyc[i]).group(1))
                group, j = 0, i - 1
                while j >= 0 and not (group and cyc[j].startswith("v_mfma")):
                    group += cyc[j].startswith("buffer_load_dwordx4")
                    j -= 1
                assert group in (4, 8) and n >= group, (name, cyc[i], group)
                groups.add(group)
                hits += 1
        assert hits >= 4 and groups == {4, 8}, (hits, groups)
    for u in find("blockdft_banddots4c_dbILi8ELi4ELi260ELi2"):
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128 and u["ScratchSize"] == 0, u    # 8 waves x 2 workgroups per CU
