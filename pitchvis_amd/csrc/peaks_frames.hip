// peaks_frames.hip — the frame-parallel peak kernels for MI355X (gfx950 / CDNA4) and their launcher.
// Hot path being replaced: the stateless peak pipeline of AnalysisState::preprocess (reference analysis.rs:332-361,
// analysis_modules/peak_detection.rs:26-241), over dB frames that sit in global memory.
//
// Kernel inventory (wave64; the per-frame routines are peaks_device.hpp's):
//   peaks_frames_lean<NK, DISTANCE, PK_FPW, DENSE>  a workgroup of 4 waves, PK_FPW frames per wave: local maxima, prominence walks,
//                           bass/general split; then sub-bin refinement and bass promotion over the workgroup's pooled peaks.  A frame
//                           with a plateau peak of three or more samples is flagged in `redo`.
//   peaks_frames_generic<NK>  one wavefront per frame, the flagged frames only (or every frame): the plateau-aware routine.
// launch_peaks_frames runs the two one behind the other; the batch paths (Vqt::peaks_stage, the timed SLOT_PEAKS stage) and the
// pre-pass of AnalysisBatch (analysis_batch.hip) call it.  Vqt::make_peak_params fills the kernels' argument struct.
#include "vqt_engine.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "device_tables.hpp"
#include "peaks_device.hpp"

// No implicit FMA contraction in this unit's own code (fft_path.hip says why).  Behind peaks_device.hpp, whose routines set their own.
#pragma clang fp contract(off)

namespace pvq {

constexpr int PK_WAVES = 4;

// Common case (no plateau peak of three or more samples in the frame): the lean routine.  A frame it cannot take is
// flagged for peaks_frames_generic, which is launched right behind it.
// A workgroup (4 waves) takes PK_FPW frames per wave and pass: each wave finds the peaks of its frames (peak lists in LDS),
// then the continuous outputs of all 4 x PK_FPW frames are refined side by side, one lane per peak over the pooled list:
// a frame has ~17 peaks, so refining per frame left three quarters of the lanes idle through ~400 vector instructions;
// pooled, enhance_peaks_continuous runs on full waves and promote_bass_peaks_with_harmonics (only the few peaks at or
// below highest_bassnote need it, but any one of them made the whole wave walk through it) runs once over the pooled
// bass peaks.
// PK_FPW frames per wave and pass: 2 up to 384 bins; 1 beyond, where a second frame per wave would cost more occupancy
// (LDS) than the denser refinement gives back
// bass peaks one frame can hold: their centre is at most highest_bassnote, so their bin at most highest_bassnote + 1,
// and peaks are never adjacent
__host__ __device__ inline int peaks_bass_cap(int n_bins, int highest_bassnote) {
    const int npad = (n_bins + 63) / 64 * 64;
    const int by_bins = (highest_bassnote < n_bins ? highest_bassnote : n_bins) / 2 + 3;
    return by_bins < npad / 2 ? by_bins : npad / 2;
}
__host__ __device__ inline size_t peaks_lean_lds_bytes(int n_bins, int dist, int PK_FPW, int highest_bassnote) {
    const size_t PK_FPG = (size_t)PK_WAVES * PK_FPW;
    const size_t npad = (size_t)((n_bins + 63) / 64 * 64);
    return PK_FPG * sizeof(float) * (npad + 2 * PK_PAD)          // frames, +INF sentinels on both sides
           + PK_FPG * peaks_lean_scratch_bytes(n_bins, dist)     // per-frame scratch of the peak search
           + 2 * PK_FPG * npad                                   // peak lists: npad / 2 u16 per frame
           + ((2 * PK_FPG * (size_t)peaks_bass_cap(n_bins, highest_bassnote) + 3) & ~(size_t)3)   // pooled bass list: u16 (frame << 10 | slot)
           + 2 * PK_FPG * sizeof(uint32_t) + 16                  // per-frame peak counts, bass counter
           + (n_bins <= 768 && !(dist > 1 && dist <= 4) ? 2 * npad * sizeof(float) : 0);   // thresholds of the candidate test (NK <= 12; not with the register distance rule)
}

template <int NK, bool DISTANCE, int PK_FPW, bool DENSE>   // DENSE: 64 (NK - 1) < n_bins <= 64 NK (the host's promise): every chunk test but the last one's folds away
__global__ __attribute__((amdgpu_flat_work_group_size(256, 256), amdgpu_waves_per_eu(NK <= 8 ? 7 : 4, 8))) void peaks_frames_lean(const float* __restrict__ db, int n_frames, PeakParamsDev a,
                                                                       uint8_t* __restrict__ redo, int frame0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pk_smem[];
    constexpr int PK_FPG = PK_WAVES * PK_FPW;     // frames per workgroup and pass
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    if constexpr (DENSE) __builtin_assume(a.n_bins > 64 * (NK - 1) && a.n_bins <= 64 * NK);
    const int n = a.n_bins;
    const int npad = (n + 63) / 64 * 64;
    const int row = npad + 2 * PK_PAD;
    float* rows = reinterpret_cast<float*>(pk_smem);                                   // [PK_FPG][row]
    const int sb = (int)peaks_lean_scratch_bytes(n, a.dist);                           // scratch of one frame
    unsigned char* scratch0 = pk_smem + PK_FPG * sizeof(float) * row;                  // [PK_FPG][sb]
    uint16_t* plists = reinterpret_cast<uint16_t*>(scratch0 + PK_FPG * sb);
    const int pl_cap = npad / 2;                                                       // peaks are never adjacent
    uint16_t* bass = plists + PK_FPG * pl_cap;                                         // [PK_FPG * bass_cap]
    const int bass_cap = peaks_bass_cap(n, a.highest_bassnote);
    uint32_t* counts = reinterpret_cast<uint32_t*>(pk_smem + ((reinterpret_cast<unsigned char*>(bass + PK_FPG * bass_cap) - pk_smem + 3) & ~(size_t)3));   // [PK_FPG]
    uint32_t* n_bass = counts + PK_FPG;
    float* thrH = reinterpret_cast<float*>(n_bass + 1);                                // [npad] per-bin height / prominence thresholds of the candidate test
    float* thrP = thrH + npad;
    // the wave's first frames are asked for before the workgroup fills its threshold table and meets at the barrier: the loads fly meanwhile
    float pre[PK_FPW][NK <= 12 ? NK : 1];
    if (NK <= 12) {
#pragma unroll
        for (int g = 0; g < PK_FPW; ++g) {
            const int frame = frame0 + blockIdx.x * PK_FPG + wv * PK_FPW + g;
            const float* src = db + (size_t)(frame < n_frames ? frame : 0) * n;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = (k << 6) + lane;
                pre[g][k] = ((k << 6) < n) ? src[i < n ? i : n - 1] : 0.0f;
            }
        }
    }
    const bool thr_lds = NK <= 12 && !(DISTANCE && a.dist <= 4);   // (beyond 768 bins, and on the list of the register distance rule, peaks_lean_scan computes them on the fly)
    if (thr_lds) {
        peaks_lean_thresholds(thrH, thrP, a, tid, PK_WAVES * 64);
        __syncthreads();
    }
    // sentinels of this wave's rows
    for (int g = 0; g < PK_FPW; ++g) {
        float* xs = rows + (wv * PK_FPW + g) * row;
        for (int i = lane; i < PK_PAD; i += 64) xs[i] = __builtin_huge_valf();
        for (int i = n + lane; i < npad + PK_PAD; i += 64) xs[PK_PAD + i] = __builtin_huge_valf();
    }
    // ONE pass per workgroup (the host launches a workgroup per PK_FPG frames; more than 2^20 workgroups' worth of frames go in further
    // launches): written as a loop over passes, the compiler hoisted ~150 instructions of loop-invariant lane masks and addresses into
    // a preamble and spilled them to lanes — for a loop that ran once.
    {
        const int base = frame0 + blockIdx.x * PK_FPG;
        if (tid == 0) *n_bass = 0;
        // 1. peak search: each wave scans its PK_FPW frames one after the other, then walks their candidates side by side
        uint32_t n_cand[PK_FPW], np[PK_FPW];
        bool done[PK_FPW];
        size_t frames[PK_FPW];
#pragma unroll
        for (int g = 0; g < PK_FPW; ++g) {
            const int fi = wv * PK_FPW + g;
            const int frame = base + fi;
            n_cand[g] = 0;
            done[g] = false;
            frames[g] = (size_t)frame;
            if (frame < n_frames) {
                float* x = rows + fi * row + PK_PAD;
                const float* src = db + (size_t)frame * n;
                if (NK <= 12) {
#pragma unroll
                    for (int k = 0; k < NK; ++k) {   // the frame into its row (the tail of its last 64 stays +INF)
                        if ((k << 6) >= n) break;
                        const int i = (k << 6) + lane;
                        x[i] = i < n ? pre[g][k] : __builtin_huge_valf();
                    }
                } else {
                    for (int i = lane; i < n; i += 64) x[i] = src[i];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                done[g] = peaks_lean_scan<NK, DISTANCE>(x, scratch0 + fi * sb, thr_lds ? thrH : nullptr, thrP, n_cand[g], a, lane);
                if (lane == 0) redo[frame] = done[g] ? 0 : 1;   // the generic kernel produces that frame's outputs, the continuous ones included
            }
        }
        peaks_lean_walk<NK, PK_FPW>(rows + wv * PK_FPW * row + PK_PAD, row, scratch0 + wv * PK_FPW * sb, sb, plists + wv * PK_FPW * pl_cap, pl_cap,
                                    n_cand, np, done, frames, a, lane);
#pragma unroll
        for (int g = 0; g < PK_FPW; ++g)
            if (lane == 0) counts[wv * PK_FPW + g] = np[g] < a.max_peaks ? np[g] : a.max_peaks;
        if (!a.center) return;   // uniform: mask / count only
        __syncthreads();
        // 2. enhance_peaks_continuous over the pooled peaks, one lane each; bass peaks are handed to step 3
        uint32_t pre[PK_FPG + 1];
        pre[0] = 0;
#pragma unroll
        for (int f = 0; f < PK_FPG; ++f) pre[f + 1] = pre[f] + counts[f];
        const uint32_t total = pre[PK_FPG];
        for (uint32_t p0 = 0; p0 < total; p0 += 256) {
            const uint32_t p = p0 + tid;
            if (p0 + (wv << 6) >= total) break;   // nothing for this wave
            bool is_bass = false;
            int fi = 0;
            uint32_t slot = 0;
            if (p < total) {
#pragma unroll
                for (int f = 1; f < PK_FPG; ++f) fi += (p >= pre[f]) ? 1 : 0;
            }
            uint32_t start = 0;
#pragma unroll
            for (int f = 0; f < PK_FPG; ++f) start = (fi == f) ? pre[f] : start;
            slot = p - start;
            if (p < total) {
                const float* x = rows + fi * row + PK_PAD;
                float ctr, sz;
                pk_enhance(x, (int)plists[fi * pl_cap + slot], a, ctr, sz);
                const size_t o = (size_t)(base + fi) * a.max_peaks + slot;
                a.center[o] = ctr;
                is_bass = !(ctr > (float)a.highest_bassnote);
                if (!is_bass) a.size[o] = sz;
            }
            const unsigned long long bm = __ballot(is_bass);
            if (bm) {
                uint32_t off = 0;
                if (lane == 0) off = atomicAdd(n_bass, (uint32_t)__popcll(bm));
                off = __builtin_amdgcn_readfirstlane(off);
                const uint32_t at = off + __popcll(bm & ((1ull << lane) - 1ull));
                if (is_bass && at < (uint32_t)(PK_FPG * bass_cap)) bass[at] = (uint16_t)((fi << 10) | slot);
            }
        }
        __syncthreads();
        // 3. promote_bass_peaks_with_harmonics over the pooled bass peaks (the centre is recomputed: cheaper than carrying it)
        const uint32_t nb_ = min(*n_bass, (uint32_t)(PK_FPG * bass_cap));
        for (uint32_t q = tid; q < nb_; q += 256) {
            const uint32_t e = bass[q];
            const int fi = (int)(e >> 10);
            const uint32_t slot = e & 1023u;
            const float* x = rows + fi * row + PK_PAD;
            float ctr, sz;
            pk_enhance(x, (int)plists[fi * pl_cap + slot], a, ctr, sz);
            pk_promote(x, a, ctr, sz);
            a.size[(size_t)(base + fi) * a.max_peaks + slot] = sz;
        }
    }
}

// Generic routine (plateau peaks, min_distance > 1).  redo == nullptr: every frame.
template <int NK>
__global__ __launch_bounds__(PK_WAVES * 64) void peaks_frames_generic(const float* __restrict__ db, int n_frames, PeakParamsDev a,
                                                                     const uint8_t* __restrict__ redo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pk_smem[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.n_bins;
    const int npad = (n + 63) / 64 * 64;
    const size_t per_wave = sizeof(float) * npad + peaks_scratch_bytes(n, a.dist);
    float* x = reinterpret_cast<float*>(pk_smem + wv * per_wave);
    unsigned char* scratch = reinterpret_cast<unsigned char*>(x + npad);
    auto one = [&](int frame) {
        const float* src = db + (size_t)frame * n;
        for (int i = lane; i < n; i += 64) x[i] = src[i];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        peaks_wave_nk<NK>(x, scratch, (size_t)frame, a, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    if (!redo) {
        for (int frame = blockIdx.x * PK_WAVES + wv; frame < n_frames; frame += gridDim.x * PK_WAVES) one(frame);
        return;
    }
    // sweep of the (mostly clear) flags: 64 per wave and step, one ballot, then only the flagged frames
    for (int base = (blockIdx.x * PK_WAVES + wv) * 64; base < n_frames; base += gridDim.x * PK_WAVES * 64) {
        unsigned long long m = __ballot(base + lane < n_frames && redo[base + lane] != 0);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            one(base + b);
        }
    }
}

bool Vqt::make_peak_params(const AnalysisParameters& ap, uint32_t* d_mask, uint32_t* d_count, float* d_center,
                           float* d_size, uint32_t max_peaks, PeakParamsDev& a) const {
    a.n_bins = (int)n_bins();
    a.bpo = (int)plan_.params.range.buckets_per_octave;
    a.min_freq = plan_.params.range.min_freq;
    a.lnf = dev_->d_lnf;
    a.peak_min_prominence = ap.peak_min_prominence;
    a.peak_min_height = ap.peak_min_height;
    a.bass_min_prominence = ap.bass_min_prominence;
    a.bass_min_height = ap.bass_min_height;
    a.highest_bassnote = (int)std::min<uint32_t>(ap.highest_bassnote, 0x7fffffffu);
    a.harmonic_threshold = ap.harmonic_threshold;
    a.dist = (int)std::lround((float)a.bpo * 0.4f / 12.0f);
    a.min_bin = ((a.bpo / 12) + 1) / 2;
    a.mask = d_mask;
    a.count = d_count;
    a.center = d_center;
    a.size = d_size;
    a.max_peaks = max_peaks;
    return a.n_bins >= 3 && a.n_bins <= 1024;
}

// the peak kernels as one timed stage (SLOT_PEAKS); callers check hipGetLastError where they always did
pvq_status Vqt::peaks_stage(const float* d_db, size_t n_frames, const PeakParamsDev& a, hipStream_t stream) {
    slot_begin(SLOT_PEAKS, stream);
    pvq_status st = ws_flags_.reserve(n_frames);
    if (st == PVQ_OK) st = launch_peaks_frames(d_db, n_frames, a, ws_flags_.as<uint8_t>(), stream);
    slot_end(SLOT_PEAKS, stream);
    return st;
}

// find_peaks over n_frames independent dB rows (the lean kernel, then the generic one over the few frames it flags in `redo`, n_frames bytes
// of device scratch): the frame kernels of the batch path, also the frame-parallel pre-pass of AnalysisBatch (analysis_batch.hip)
pvq_status launch_peaks_frames(const float* d_db, size_t n_frames, const PeakParamsDev& a, uint8_t* redo, hipStream_t stream) {
    const int npad = (a.n_bins + 63) / 64 * 64;
    const size_t lds_gen = PK_WAVES * (sizeof(float) * npad + peaks_scratch_bytes(a.n_bins, a.dist));
    // bins per lane: 4 (<= 256 bins), 8 (<= 512), 12 (<= 768) or 16 (<= 1024); the lean kernel also has 5 (<= 320), 6 (<= 384) and 10 (<= 640)
    auto launch_generic = [&](int g, const uint8_t* flags) {
        if (a.n_bins <= 256)
            hipLaunchKernelGGL(peaks_frames_generic<4>, dim3(g), dim3(PK_WAVES * 64), lds_gen, stream, d_db, (int)n_frames, a, flags);
        else if (a.n_bins <= 512)
            hipLaunchKernelGGL(peaks_frames_generic<8>, dim3(g), dim3(PK_WAVES * 64), lds_gen, stream, d_db, (int)n_frames, a, flags);
        else if (a.n_bins <= 768)
            hipLaunchKernelGGL(peaks_frames_generic<12>, dim3(g), dim3(PK_WAVES * 64), lds_gen, stream, d_db, (int)n_frames, a, flags);
        else
            hipLaunchKernelGGL(peaks_frames_generic<16>, dim3(g), dim3(PK_WAVES * 64), lds_gen, stream, d_db, (int)n_frames, a, flags);
    };
    const int sweep_grid = (int)std::min<size_t>(256, (n_frames + 64 * PK_WAVES - 1) / (64 * PK_WAVES));
    const int fpw = a.n_bins <= 384 ? 2 : 1;
    const size_t lds_lean = peaks_lean_lds_bytes(a.n_bins, a.dist, fpw, a.highest_bassnote);
    const size_t fpg = (size_t)PK_WAVES * fpw;   // frames per workgroup: one pass each
    auto launch_lean = [&](auto nk_c, auto dist_c) {
        constexpr int NK = decltype(nk_c)::value;
        constexpr bool D = decltype(dist_c)::value;
        for (size_t f0 = 0; f0 < n_frames; f0 += ((size_t)1 << 20) * fpg) {
            const int grid_lean = (int)std::min<size_t>((n_frames - f0 + fpg - 1) / fpg, (size_t)1 << 20);
            if (a.n_bins > 64 * (NK - 1))
                hipLaunchKernelGGL((peaks_frames_lean<NK, D, (NK <= 6 ? 2 : 1), true>), dim3(grid_lean), dim3(PK_WAVES * 64), lds_lean, stream, d_db, (int)n_frames, a, redo, (int)f0);
            else
                hipLaunchKernelGGL((peaks_frames_lean<NK, D, (NK <= 6 ? 2 : 1), false>), dim3(grid_lean), dim3(PK_WAVES * 64), lds_lean, stream, d_db, (int)n_frames, a, redo, (int)f0);
        }
    };
    using std::integral_constant;
    if (a.dist > 1) {
        if (a.n_bins <= 256) launch_lean(integral_constant<int, 4>{}, std::true_type{});
        else if (a.n_bins <= 320) launch_lean(integral_constant<int, 5>{}, std::true_type{});
        else if (a.n_bins <= 384) launch_lean(integral_constant<int, 6>{}, std::true_type{});
        else if (a.n_bins <= 512) launch_lean(integral_constant<int, 8>{}, std::true_type{});
        else if (a.n_bins <= 640) launch_lean(integral_constant<int, 10>{}, std::true_type{});   // (588 bins = 7 x 84: the reference's default geometry)
        else if (a.n_bins <= 768) launch_lean(integral_constant<int, 12>{}, std::true_type{});
        else launch_lean(integral_constant<int, 16>{}, std::true_type{});
    } else {
        if (a.n_bins <= 256) launch_lean(integral_constant<int, 4>{}, std::false_type{});
        else if (a.n_bins <= 320) launch_lean(integral_constant<int, 5>{}, std::false_type{});   // (288 bins = 8 x 36: BASELINE configs[2])
        else if (a.n_bins <= 384) launch_lean(integral_constant<int, 6>{}, std::false_type{});
        else if (a.n_bins <= 512) launch_lean(integral_constant<int, 8>{}, std::false_type{});
        else if (a.n_bins <= 640) launch_lean(integral_constant<int, 10>{}, std::false_type{});
        else if (a.n_bins <= 768) launch_lean(integral_constant<int, 12>{}, std::false_type{});
        else launch_lean(integral_constant<int, 16>{}, std::false_type{});
    }
    launch_generic(sweep_grid, redo);   // small grid: it only sweeps the (mostly clear) flags
    return PVQ_OK;
}

}  // namespace pvq
