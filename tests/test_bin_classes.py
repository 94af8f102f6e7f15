"""The table of tests/test_bin_classes_gpu.py against the kernels' dispatch rules, without a GPU.

The rules by which four stages pick a kernel instantiation from the bin count are restated here; the thresholds are read out of
the sources and must equal the restatement.  Every row of the table must land in the classes it claims (its bin count from the
host plan, its paths from the block-DFT path's applicability rule), and every class must have rows at both of its edges, or the
table must say why an edge cannot be built.  A class added or moved later without a row at its edges fails here."""
import os
import re

import numpy as np
import pytest

import pitchvis_amd as P
from helpers import geom_pair
from test_bin_classes_gpu import AB_MAX_OCTAVES, AB_ROWS, BD, EDGE_NOTES, FFT, VQT_ROWS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pitchvis_amd", "csrc")

# ---- the restatement: (highest bin count, class) in ascending order --------------------------------------------------------------
KP_FP32 = [(256, "lds260"), (304, "lds308"), (368, "lds372"), (592, "lds596"), (848, "lds852"), (1020, "lds1028"), (1024, "db1x8")]
KP_BF16 = [(256, "bf2x4"), (1024, "bf1x4")]
PEAK_NK = [(256, 4), (320, 5), (384, 6), (512, 8), (640, 10), (768, 12), (1024, 16)]   # lean kernel; DENSE: n > 64 (NK - 1)
PEAK_GENERIC_NK = [(256, 4), (512, 8), (768, 12), (1024, 16)]
PEAK_THR_LDS_MAX = 768            # thresholds kept in LDS up to here, and not with the register distance rule (distance 2 ... 4)
PEAK_REG_DIST = (2, 4)
AB_NK = [(256, 4), (384, 6), (512, 8), (640, 10), (768, 12), (1024, 16)]
FFT_DB = [(1024, "fftdb"), (4096, "fftdb-wide")]
MIN_BINS = 3
BLOCKDFT_MAX_BINS, HOP_MIN, HOP_MAX, CB_MAX_NB = 1024, 64, 4096, 256


def min_distance(bpo):
    """a.dist = lround((float) bpo * 0.4f / 12.0f)"""
    return int(np.round(np.float32(bpo) * np.float32(0.4) / np.float32(12.0)))


def _pick(table, n):
    return next(c for hi, c in table if n <= hi)


def _nk_class(prefix, table, n, bpo):
    nk = _pick(table, n)
    return f"{prefix}{nk}{'d' if n > 64 * (nk - 1) else 's'}-{'dist' if min_distance(bpo) > 1 else 'nodist'}"


def blockdft_applies(n_bins, windows, hop):
    """Vqt::blockdft_applicable for a power-of-two hop (the table uses no other)"""
    return (n_bins <= BLOCKDFT_MAX_BINS and HOP_MIN <= hop <= HOP_MAX and hop & (hop - 1) == 0
            and all(w % hop == 0 and w // hop <= CB_MAX_NB for w in windows))


def classes_of_vqt_row(n, bpo, paths):
    out = {_pick(FFT_DB, n)}
    if BD[1] in paths:
        out |= {_pick(KP_FP32, n), _pick(KP_BF16, n)}
    if n <= 1024:
        out.add(_nk_class("pk", PEAK_NK, n, bpo))
    return out


def classes_of_ab_row(n, bpo):
    return {_nk_class("ab", AB_NK, n, bpo), _nk_class("pk", PEAK_NK, n, bpo)}


def all_classes():
    """(class, lowest, highest bin count, DIST or None)"""
    out = []
    for table in (KP_FP32, KP_BF16, FFT_DB):
        lo = MIN_BINS
        for hi, c in table:
            out.append((c, lo, hi, None))
            lo = hi + 1
    for prefix, table in (("pk", PEAK_NK), ("ab", AB_NK)):
        lo = MIN_BINS
        for hi, nk in table:
            cut = 64 * (nk - 1)
            for d, name in ((False, "nodist"), (True, "dist")):
                if lo <= cut:
                    out.append((f"{prefix}{nk}s-{name}", lo, min(hi, cut), d))
                if hi > cut:
                    out.append((f"{prefix}{nk}d-{name}", max(lo, cut + 1), hi, d))
            lo = hi + 1
    return out


def ab_buildable(n, dist):
    """an AnalysisBatch range of n bins with DIST = dist: octaves x bpo, octaves <= AB_MAX_OCTAVES"""
    return any(n % o == 0 and (min_distance(n // o) > 1) == dist for o in range(1, AB_MAX_OCTAVES + 1))


# ---- the rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", VQT_ROWS, ids=lambda r: f"{r[4]}-{r[0] / 1000:g}k")
def test_vqt_rows_build_and_land_in_their_classes(row):
    sr, fmin, octaves, bpo, bins, hop, claims, paths = row
    pp, _ = geom_pair(sr, fmin, octaves, bpo)
    v = P.Vqt.new(pp, -1)   # the host plan
    assert v.n_bins == bins
    windows = [g.window_size() for g in v.kernel().window_groups]
    assert tuple(paths) == (BD if blockdft_applies(bins, windows, hop) else (FFT,)), windows
    assert set(claims) == classes_of_vqt_row(bins, bpo, paths)


@pytest.mark.parametrize("row", AB_ROWS, ids=lambda r: f"{r[2]}")
def test_analysis_rows_land_in_their_classes(row):
    octaves, bpo, bins, claims = row
    assert octaves * bpo == bins and 1 <= octaves <= AB_MAX_OCTAVES
    assert set(claims) == classes_of_ab_row(bins, bpo)


def test_the_table_has_rows_at_every_class_edge():
    have = {}
    for r in VQT_ROWS:
        for c in classes_of_vqt_row(r[4], r[3], r[7]):
            have.setdefault(c, set()).add(r[4])
    for r in AB_ROWS:
        for c in classes_of_ab_row(r[2], r[1]):
            have.setdefault(c, set()).add(r[2])
    rows_at_some_edge = 0
    used_notes = set()
    for name, lo, hi, dist in all_classes():
        got = have.get(name, set())
        assert got, f"class {name} ({lo} ... {hi} bins) has no row"
        for edge in (lo, hi):
            if edge in got:
                rows_at_some_edge += 1
                continue
            assert (name, edge) in EDGE_NOTES, f"class {name}: no row at {edge} bins and no note why"
            used_notes.add((name, edge))
            stand_in, why = EDGE_NOTES[(name, edge)]
            assert why and stand_in in got and lo <= stand_in <= hi, (name, edge, stand_in)
            if dist is not None:   # the edge really cannot be built, and the stand-in is the nearest count that can
                step = 1 if edge == lo else -1
                assert not any(ab_buildable(n, dist) for n in range(edge, stand_in, step)), (name, edge)
                assert ab_buildable(stand_in, dist), (name, stand_in)
    assert used_notes == set(EDGE_NOTES), set(EDGE_NOTES) - used_notes   # no stale note
    assert rows_at_some_edge > 0


# ---- the sources say what the restatement says -----------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _ints(m):
    return tuple(int(x) for x in m.groups())


def test_kernel_product_thresholds_match_the_restatement():
    # (the block-DFT path's three units and their shared header: the launches; the path's host planning)
    s = "".join(_src(f) for f in ("vqt_blockdft.hip", "blockdft_gemm.hip", "blockdft_dots.hip", "blockdft_device.hpp", "blockdft_plan.cpp", "blockdft_plan.hpp"))
    ldb2 = int(re.search(r"constexpr int BAND_LDB2 = (\d+);", s).group(1))
    ldb3 = int(re.search(r"constexpr int BAND_LDB3 = (\d+);", s).group(1))
    assert (ldb2, ldb3) == (260, 308)
    # 64-frame tiles: n_bins_pad (a multiple of 64) <= 256, or the fp32 8-bin form up to BAND_LDB3 - 4 bins
    m = re.search(r"const bool wide308 = !gemm_split_bf16_ && t->n_bins_pad > (\d+) && nb <= BAND_LDB3 - (\d+);", s)
    assert m and (int(m.group(1)), ldb3 - int(m.group(2))) == (256, 304)
    m = re.search(r"const bool wide = t->n_bins_pad <= (\d+) \|\| wide308;", s)
    assert m and int(m.group(1)) == 256
    assert re.search(r"t\.n_bins_pad = \(nb \+ 63\) / 64 \* 64;", s)
    m = re.search(r"const int ldb_c = nb <= (\d+) \? (\d+) : nb <= (\d+) \? (\d+) : nb <= (\d+) \? (\d+) : (\d+);", s)
    assert m, "the kernel product's LDS stride classes moved"
    v = _ints(m)
    strided = [(v[0], f"lds{v[1]}"), (v[2], f"lds{v[3]}"), (v[4], f"lds{v[5]}")]
    m = re.search(r"\} else if \(dots16_env \|\| nb > (\d+) - (\d+)\) \{\s*hipLaunchKernelGGL\(\(blockdft_banddots_db<1, 8>\)", s)
    assert m
    last_strided = int(m.group(1)) - int(m.group(2))
    restated = [(256, f"lds{ldb2}"), (ldb3 - 4, f"lds{ldb3}")] + strided + [(last_strided, f"lds{v[6]}"), (1024, "db1x8")]
    assert restated == KP_FP32
    # every stride holds its class's bins
    for (hi, c) in KP_FP32[:-1]:
        assert int(c[3:]) >= hi + 4, c
    assert re.search(r"hipLaunchKernelGGL\(\(blockdft_banddots_db_bf16x3<2, 4>\)", s) and re.search(r"hipLaunchKernelGGL\(\(blockdft_banddots_db_bf16x3<1, 4>\)", s)
    m = re.search(r"if \(plan\.params\.range\.n_buckets\(\) > (\d+)\) return false;", s)
    assert m and int(m.group(1)) == BLOCKDFT_MAX_BINS
    assert "bool Vqt::blockdft_applicable(size_t hop) const { return has_device() && blockdft_plan_applicable(plan_, hop); }" in s
    m = re.search(r"if \(hop < (\d+) \|\| hop % (\d+) != 0 \|\| hop > (\d+)\) return false;", s)
    assert m and _ints(m) == (HOP_MIN, 64, HOP_MAX)
    m = re.search(r"constexpr int CB_MAX_NB = (\d+);", s)
    assert m and int(m.group(1)) == CB_MAX_NB


def test_peak_thresholds_match_the_restatement():
    s = _src("peaks_frames.hip")
    body = s[s.index("pvq_status launch_peaks_frames("):]
    body = body[:body.index("\n}\n")]
    for flag in ("true", "false"):
        chain = re.findall(r"a\.n_bins <= (\d+)\) launch_lean\(integral_constant<int, (\d+)>\{\}, std::" + flag + r"_type\{\}\)", body)
        last = re.findall(r"else launch_lean\(integral_constant<int, (\d+)>\{\}, std::" + flag + r"_type\{\}\)", body)
        assert [(int(a), int(b)) for a, b in chain] + [(1024, int(last[0]))] == PEAK_NK, flag
    assert re.search(r"if \(a\.dist > 1\) \{", body)
    assert re.search(r"if \(a\.n_bins > 64 \* \(NK - 1\)\)\s*hipLaunchKernelGGL\(\(peaks_frames_lean<NK, D, \(NK <= 6 \? 2 : 1\), true>\)", body)
    gen = re.findall(r"if \(a\.n_bins <= (\d+)\)\s*hipLaunchKernelGGL\(peaks_frames_generic<(\d+)>", body)
    gen_last = re.search(r"else\s*hipLaunchKernelGGL\(peaks_frames_generic<(\d+)>", body)
    assert [(int(a), int(b)) for a, b in gen] + [(1024, int(gen_last.group(1)))] == PEAK_GENERIC_NK
    m = re.search(r"\+ \(n_bins <= (\d+) && !\(dist > 1 && dist <= (\d+)\) \? 2 \* npad \* sizeof\(float\) : 0\);", s)
    assert m and (int(m.group(1)), (2, int(m.group(2)))) == (PEAK_THR_LDS_MAX, PEAK_REG_DIST)
    m = re.search(r"const bool thr_lds = NK <= (\d+) && !\(DISTANCE && a\.dist <= (\d+)\);", s)
    assert m and (64 * int(m.group(1)), int(m.group(2))) == (PEAK_THR_LDS_MAX, PEAK_REG_DIST[1])
    assert "a.dist = (int)std::lround((float)a.bpo * 0.4f / 12.0f);" in s
    assert "return a.n_bins >= 3 && a.n_bins <= 1024;" in s


def test_analysis_batch_thresholds_match_the_restatement():
    s = _src("analysis_batch.hip")
    for macro in ("PVQ_AB_REC", "PVQ_AB_LAUNCH"):
        m = re.search(r"pvq_status lst = ((?:a\.n_bins <= \d+ \? " + macro + r"\(\d+\)\s*:\s*)+)" + macro + r"\((\d+)\);", s)
        assert m, macro
        chain = [(int(a), int(b)) for a, b in re.findall(r"a\.n_bins <= (\d+) \? " + macro + r"\((\d+)\)", m.group(1))]
        assert chain + [(1024, int(m.group(2)))] == AB_NK, macro
        assert re.search(r"#define " + macro + r"\(NK\) \(a\.n_bins > 64 \* \(NK - 1\) \?", s), macro
    assert re.search(r"\(dist \? launch\(ab_frames<NK, true, true>\) : launch\(ab_frames<NK, false, true>\)\)", s)
    m = re.search(r"if \(n < (\d+) \|\| n > (\d+)\) \{\s*set_last_error\(\"unsupported: the batched AnalysisState", s)
    assert m and _ints(m) == (MIN_BINS, 1024)


def test_fft_epilogue_thresholds_match_the_restatement():
    """the dB epilogue of T threads holds max(4, 1024 / T) bins per thread; above 1 024 bins the FFT path takes 512 or 1 024
    threads per frame (db_rows_batch<1024> behind the batch kernels), beyond 4 096 it refuses"""
    s = _src("fft_path.hip")
    assert "constexpr int PER = 1024 / T < 4 ? 4 : 1024 / T;" in s
    m = re.search(r"constexpr int FFT_MAX_BINS = (\d+);", s)
    assert m and int(m.group(1)) == FFT_DB[-1][0]
    m = re.search(r"return n_bins <= \(1024 / T < 4 \? 4 \* T : (\d+)\) \? T : n_bins <= (\d+) \? \(T > 512 \? T : 512\) : 1024;", s)
    assert m and _ints(m) == (FFT_DB[0][0], 2048)
    assert re.search(r"if \(fft_db_threads\(256, a\.n_bins\) == 256\)\s*hipLaunchKernelGGL\(db_rows_batch<256>", s)
    assert re.search(r"else[^\n]*\n\s*hipLaunchKernelGGL\(db_rows_batch<1024>", s)

    def per_t(T, n):   # the restated fft_db_threads
        return T if n <= max(1024, 4 * T) else (max(T, 512) if n <= 2048 else 1024)
    for T in (128, 256, 512, 1024):
        for n in (3, 1024, 1025, 2048, 2049, 4096):
            t = per_t(T, n)
            assert max(4, 1024 // t) * t >= n and t >= T, (T, n)
