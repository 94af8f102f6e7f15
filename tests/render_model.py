"""REFERENCE MODEL (test infrastructure only) of the viewer's per-frame products that depend on AnalysisState alone: a literal
NumPy-f32 restatement of pitchvis_viewer/src/display_system/update.rs:961-1065 (update_spectrogram_system's match, both
SpectrogramModes) and :1102-1131 (update_chroma_system's chroma), as sequential loops, line for line; written independently of
pitchvis_amd/csrc.  The colour mapping, the LED frame and `as u8` are oracle/consumers.py's, unchanged.  Parity with the Rust
binaries is UNPINNED like theirs (no toolchain; the `lab` crate is restated, not vendored)."""
from __future__ import annotations

import math

import numpy as np

from oracle.consumers import _as_u8, calculate_color, led_frame  # noqa: F401  (led_frame: re-exported for the tests)

f32 = np.float32
VQT, PEAKS = 0, 1                                                     # SpectrogramMode
# pitchvis_colors/src/lib.rs:19-36, :56-57
COLORS = np.array([
    [0.85, 0.36, 0.36], [0.01, 0.52, 0.71], [0.97, 0.76, 0.05], [0.45, 0.34, 0.63], [0.47, 0.77, 0.22], [0.78, 0.32, 0.52],
    [0.00, 0.64, 0.56], [0.95, 0.54, 0.23], [0.30, 0.37, 0.64], [1.00, 0.96, 0.03], [0.57, 0.30, 0.55], [0.12, 0.71, 0.34],
], f32)
GRAY_LEVEL, EASING_POW = 60.0, 1.3


def _fmax(a, b):
    """f32::max: a NaN operand is ignored"""
    return f32(np.fmax(f32(a), f32(b)))


def _clamp(v, lo, hi):
    """f32::clamp: a NaN passes through"""
    v = f32(v)
    if v < f32(lo):
        return f32(lo)
    if v > f32(hi):
        return f32(hi)
    return v


def _texel(x):
    """`(x * 255.0 * 1.2).clamp(0.0, 255.0) as u8` (update.rs:998-1001, :1053-1059)"""
    return _as_u8(_clamp(f32(f32(f32(x) * f32(255.0)) * f32(1.2)), 0.0, 255.0))


def _rem(a, b):
    """f32 `%`: the remainder with the sign of the dividend, exact"""
    return f32(math.fmod(float(f32(a)), float(f32(b))))


def _as_usize(v):
    """`as usize`: saturating, NaN -> 0, truncating"""
    v = float(v)
    if not (v > 0.0):
        return 0
    return int(min(v, 2.0 ** 63))


def spectrogram_row(mode, n_buckets, bpo, x_vqt_smoothed=None, peaks_continuous=(), colors=COLORS, gray_level=GRAY_LEVEL,
                    easing_pow=EASING_POW):
    """update.rs:961-1065: the row written at write_index, uint8 [n_buckets][4] (the line is all zeros before: update.rs:1068-1078
    cleared it one frame earlier)"""
    width = n_buckets
    row = np.zeros((width, 4), np.uint8)
    with np.errstate(all="ignore"):
        if mode == VQT:
            vqt_data = np.asarray(x_vqt_smoothed, f32)
            max_val = f32(0.0)                                            # update.rs:967
            for v in vqt_data:
                max_val = _fmax(max_val, v)
            for bin_idx in range(width):                                  # update.rs:970
                value_db = vqt_data[bin_idx]
                if max_val > 0.0:                                         # update.rs:974-979
                    normalized = f32(value_db / f32(max_val + f32(0.001)))
                    brightness = _clamp(f32(f32(f32(1.0) - f32(np.power(f32(f32(1.0) - normalized), f32(2.0)))) * f32(1.5)), 0.0, 1.0)
                else:
                    brightness = f32(0.0)
                buckets_per_semitone = bpo // 12                          # update.rs:982-984
                semitone_offset = f32(bpo - 3 * buckets_per_semitone)
                r, g, b = calculate_color(bpo, _rem(f32(f32(bin_idx) + semitone_offset), f32(bpo)), colors, gray_level, easing_pow)
                row[bin_idx, 0] = _texel(r)                               # update.rs:998-1001
                row[bin_idx, 1] = _texel(g)
                row[bin_idx, 2] = _texel(b)
                row[bin_idx, 3] = _texel(brightness)
        else:
            PEAK_RADIUS = f32(2.0)                                        # update.rs:1007
            max_size = f32(0.0)                                           # update.rs:1010-1014
            for _, size in peaks_continuous:
                max_size = _fmax(max_size, size)
            if max_size > 0.0:                                            # update.rs:1016
                for center, size in peaks_continuous:
                    center, size = f32(center), f32(size)
                    brightness = _clamp(f32(f32(f32(1.0) - f32(np.power(f32(f32(1.0) - f32(size / max_size)), f32(2.0)))) * f32(1.5)),
                                        0.0, 1.0)                         # update.rs:1022-1023
                    buckets_per_semitone = bpo // 12
                    semitone_offset = f32(bpo - 3 * buckets_per_semitone)
                    r, g, b = calculate_color(bpo, _rem(f32(center + semitone_offset), f32(bpo)), colors, gray_level, easing_pow)
                    min_bin = _as_usize(_fmax(np.floor(f32(center - PEAK_RADIUS)), 0.0))                  # update.rs:1038
                    max_bin = _as_usize(f32(np.fmin(np.ceil(f32(center + PEAK_RADIUS)), f32(width))))     # update.rs:1039
                    for bin_idx in range(min_bin, max_bin):               # update.rs:1041
                        distance = f32(abs(f32(f32(bin_idx) - center)))
                        if distance <= PEAK_RADIUS:
                            falloff = f32(np.exp(f32(f32(f32(-distance) * distance) / f32(PEAK_RADIUS * PEAK_RADIUS * f32(0.5)))))
                            pixel_brightness = f32(brightness * falloff)
                            row[bin_idx, 0] = _texel(r)                   # update.rs:1053-1059
                            row[bin_idx, 1] = _texel(g)
                            row[bin_idx, 2] = _texel(b)
                            row[bin_idx, 3] = _texel(pixel_brightness)
    return row


def bin_0_pitch_class(min_freq):
    """update.rs:1108-1110"""
    C4_FREQ = f32(261.626)
    semitones_from_c4 = f32(f32(12.0) * f32(np.log2(f32(f32(min_freq) / C4_FREQ))))
    r = float(semitones_from_c4)
    rounded = math.floor(r + 0.5) if r >= 0 else -math.floor(-r + 0.5)    # f32::round: half away from zero
    return (int(math.fmod(rounded, 12)) + 12) % 12                        # i32 `%` truncates toward zero


def chroma_row(min_freq, n_buckets, bpo, x_vqt_smoothed):
    """update.rs:1102-1131: float32 [12]"""
    x = np.asarray(x_vqt_smoothed, f32)
    chroma = [f32(0.0)] * 12                                              # update.rs:1103
    b0 = bin_0_pitch_class(min_freq)
    with np.errstate(all="ignore"):
        for bin_idx in range(n_buckets):                                  # update.rs:1112
            q = float(f32(f32(bin_idx * 12) / f32(bpo)))
            semitone = int(math.floor(q + 0.5))                           # .round() as usize of a non-negative value
            pitch_class = (semitone + b0) % 12                            # update.rs:1118
            power = f32(np.power(f32(10.0), f32(x[bin_idx] / f32(10.0)))) # update.rs:1121
            chroma[pitch_class] = f32(chroma[pitch_class] + power)
        max_chroma = f32(0.0)                                             # update.rs:1126
        for c in chroma:
            max_chroma = _fmax(max_chroma, c)
        if max_chroma > 0.0:                                              # update.rs:1127-1131
            chroma = [f32(c / max_chroma) for c in chroma]
    return np.asarray(chroma, f32)


def oracle_rows(min_freq, octaves, bpo, n_rows, seed, db_frames=None, every=3):
    """Rows to render: the `pub` fields of oracle.analysis_state.OracleAnalysisState after each of a run of frames.  db_frames
    [n][n_bins] (dB frames of a transform); None: synthetic dB-like frames (a noise floor, notes that start, hold, glide and stop,
    a silent stretch).  Returns (smoothed [n_rows][n_bins] f32, peaks: per row a list of (center, size))."""
    from oracle.analysis_state import OracleAnalysisState
    n_bins = octaves * bpo
    if db_frames is None:
        rng = np.random.default_rng(seed)
        nf = n_rows * every
        db_frames = (rng.random((nf, n_bins), dtype=np.float32) * 6.0).astype(f32)
        for _ in range(6):
            b0, t0 = int(rng.integers(3, n_bins - 3)), int(rng.integers(0, max(1, nf - 10)))
            t1 = min(nf, t0 + int(rng.integers(10, 60)))
            lvl = float(rng.uniform(18.0, 50.0))
            for t in range(t0, t1):
                b = int(np.clip(b0 + (t - t0) // 17, 2, n_bins - 3))
                db_frames[t, b] = lvl + 0.3 * np.sin(t / 7.0)
                db_frames[t, b - 1] = max(db_frames[t, b - 1], lvl - 9.0)
                db_frames[t, b + 1] = max(db_frames[t, b + 1], lvl - 11.0)
        db_frames[nf // 2:nf // 2 + 4] = 0.0
    st = OracleAnalysisState(min_freq, octaves, bpo)
    smoothed, peaks = [], []
    for f in range(min(len(db_frames), n_rows * every)):
        st.preprocess(db_frames[f], 33_333_333)
        if f % every == every - 1:
            smoothed.append(np.array([e.y for e in st.smoothed], f32))
            peaks.append(list(zip(st.centers.astype(f32).tolist(), st.sizes.astype(f32).tolist())))
    return np.asarray(smoothed, f32), peaks


def compare_u8(got, want):
    """(largest difference in levels, share of bytes that differ) of two uint8 arrays"""
    d = np.abs(np.asarray(got).astype(np.int32) - np.asarray(want).astype(np.int32))
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0
