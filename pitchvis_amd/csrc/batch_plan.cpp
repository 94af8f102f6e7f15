// batch_plan.cpp — host planning of one batch call: route, interleaved runs, staging of short streams (batch_plan.hpp)
#include "batch_plan.hpp"

#include <algorithm>
#include <cmath>

namespace pvq {

BatchRoute route_batch(pvq_algo algo, size_t r, bool takes_streams, size_t n_frames, size_t auto_min_frames) {
    if (algo == PVQ_ALGO_FFT) return BatchRoute::Fft;
    const bool forced = algo == PVQ_ALGO_BLOCKDFT;
    if (r == 0) return forced ? BatchRoute::RefuseNoHop : BatchRoute::Fft;
    if (!forced && n_frames < auto_min_frames) return BatchRoute::Fft;
    if (takes_streams) return BatchRoute::BlockStreams;
    // the unfused stages: the hop only as it is
    if (r == 1) return BatchRoute::BlockPerStream;
    return forced ? BatchRoute::RefuseUnfusedHop : BatchRoute::Fft;
}

// From how many frames on PVQ_ALGO_AUTO takes the block-DFT path (hop * r its block length).  A power-of-two hop: from 384 frames
// (and at least one tile row per grid).  A general hop is different:
// its tiles' K loops are hop * r / 2 deep, so a launch cannot end before ~180 us at 1 600 samples and ~300 us at 3 200 however few
// frames it holds, while the FFT path — a workgroup per frame, 512 of them side by side — takes 53 us for up to ~420 frames and
// 0.125 us per frame beyond (48 kHz / 252 bins; profiles/r04_small_batches.txt: 64 frames at hop 800 took 367 us on the block path
// against 64 on the FFT path).  The estimate below — both paths' time as floor + frames x slope, the slopes scaled by the geometry's
// FFT work and column count — puts the switch where the two lines cross: ~1 700 frames at hop 800 / 1 600, ~3 500 at 3 200.
size_t auto_block_min_frames(const HostPlan& plan, size_t hop, size_t r) {
    const size_t hop_eff = hop * r;
    bool divides = (hop_eff & (hop_eff - 1)) == 0;
    double fft_work = 0.0;   // sum over the window groups of W log2 W
    size_t cols = 0;         // spectrum columns the kernel reads (upper bound: every group's highest column)
    for (const WindowGroup& g : plan.kernel.window_groups) {
        const size_t w = g.window_size();
        divides = divides && w % hop_eff == 0;
        fft_work += (double)w * std::log2((double)w);
        uint32_t top = 0;
        for (uint32_t c : g.filter_bank.col_idx) top = c > top ? c : top;
        for (uint32_t c : g.negative_filter_bank.col_idx) top = c > top ? c : top;
        cols += top + 1;
    }
    // (a power-of-two hop: both paths' launches are short; the block path's two kernels cost 58-67 us up to ~1 000 frames at 48 kHz /
    // 252 bins, the FFT path — group-split for few frames, launch_fft_streams — 19 us for one frame, 42 for 256, 56 for 400)
    if (divides) return std::max<size_t>(64 * r, 384);
    // Both paths' time for n frames, in us, as measured on one box (profiles/r05_auto_rule.txt):
    //   FFT path     t_fft (n + 500): the per-window kernels (round 5: half the walk's time) ~ the FFT work + the row dots (bins)
    //   block path   max(floor, floor / 2 + t_block n): a launch pair cannot end before `floor` however few frames it holds; per frame the K loops'
    //                depth x columns + the kernel product (bins)
    // and the switch sits at the first n (in steps of 64 r) where the block path is the faster one.  At the reference's default geometry
    // (22 050 Hz, 588 bins) the per-window FFT kernels run level with the general-hop block path — 0.035 against 0.038 us per frame at hop 1 600 —
    // and AUTO stays on the FFT path at every size.
    const uint32_t n_bins = plan.params.range.n_buckets();
    double t_fft = 1.45e-7 * fft_work + 1.0e-5 * (double)n_bins;
    if (plan.params.n_fft > 0 && fft_work > 6.0e5) t_fft *= 1.15;                        // (a 32 768-sample window: 1 024 threads per frame, one workgroup per CU)
    const double floor_block = 58.0 + 0.075 * ((double)hop_eff - 256.0) + 18.0;           // us: shortest launch pair of the general-hop kernels
    const double t_block = 1.0e-5 * (double)hop_eff * ((double)cols / 871.0) + 3.2e-5 * (double)n_bins;   // (871: the column bound at 48 kHz / 252 bins, 602 of them read)
    const size_t lo = 64 * r;
    if (t_fft <= t_block) {   // the lines never cross beyond the floor: the switch, if any, lies where the FFT path reaches the block path's floor
        const double n = floor_block / t_fft - 500.0;
        return n > 0.0 && floor_block / 2 + t_block * n <= floor_block ? std::max(lo, (size_t)n) : ~(size_t)0 >> 1;
    }
    for (size_t n = lo; n < ((size_t)1 << 22); n += lo)
        if (std::max(floor_block, floor_block / 2 + t_block * (double)n) < t_fft * ((double)n + 500.0)) return n;
    return ~(size_t)0 >> 1;
}

std::vector<BdStream> rebase_runs(const StreamRun* st, size_t n_st, const float** base) {
    const float* lo = st[0].pcm;
    for (size_t i = 1; i < n_st; ++i)
        if (st[i].pcm < lo) lo = st[i].pcm;
    std::vector<BdStream> out(n_st);
    for (size_t i = 0; i < n_st; ++i) {
        const StreamRun& S = st[i];
        const long long off = (long long)(((intptr_t)S.pcm - (intptr_t)lo) / (intptr_t)sizeof(float));   // (as integers: the streams are separate allocations)
        out[i] = BdStream{off, S.first_end, S.n_samples, S.n_frames, S.out_row0, S.row_step, S.slots, S.n_slots, S.grid_i, S.slot_hash};
    }
    *base = lo;
    return out;
}

void append_interleaved_runs(std::vector<StreamRun>& runs, const float* pcm, size_t lead, size_t n_frames, size_t hop, size_t r, size_t row0) {
    for (size_t i = 0; i < r && i < n_frames; ++i)
        runs.push_back(StreamRun{pcm, lead + (i + 1) * hop, lead + n_frames * hop, (n_frames - i + r - 1) / r, row0 + i, r});
}

// SHORT streams are staged one behind the other into ONE buffer — each in a slot of whole 64 r-frame tiles, the zeroed gap behind
// it holding the next stream's history — and analysed as one long stream: a tile of the GEMM then never stops at a stream's end,
// no stream's first tile is a range-checked one (dword loads: twice the time, no 64-column pairing), and a stream shorter than a
// tile does not leave the rest of it empty.  The price is one copy of the PCM (1 KB per frame at hop 256 against the 9.6 KB of X
// traffic) and the gap frames (63 per stream at hop 256, 9 at hop 1 600), which are computed and dropped.  Long streams go as
// they are (segments of the launch, no copy).  Same bits either way: a frame's values do not depend on its place in a tile.
StreamStaging plan_stream_staging(const float* const* pcm, const size_t* lead_of, const size_t* n_frames, uint32_t n_streams, size_t stride, size_t hop,
                                  size_t r, size_t window_union, size_t stage_max) {
    StreamStaging out;
    const size_t G = staging_history_frames(window_union, hop);   // frames of history a stream's first frame needs
    const size_t A = 64 * r;                                       // slots start on whole tiles of every grid
    std::vector<uint32_t> shorts;
    for (uint32_t s = 0; s < n_streams; ++s) {
        if (n_frames[s] == 0) continue;
        if (n_streams > 1 && n_frames[s] <= stage_max)
            shorts.push_back(s);
        else
            append_interleaved_runs(out.longs, pcm[s], lead_of ? lead_of[s] : 0, n_frames[s], hop, r, (size_t)s * stride);
    }
    if (shorts.size() == 1) {   // a single short stream gains nothing from a copy
        const uint32_t s = shorts[0];
        append_interleaved_runs(out.longs, pcm[s], lead_of ? lead_of[s] : 0, n_frames[s], hop, r, (size_t)s * stride);
        shorts.clear();
    }
    // staged buffers of at most 144 K frames (one sub-batch of the block-DFT path) and 512 MiB each
    const size_t vcap = std::max<size_t>(A * 4, std::min<size_t>((size_t)147456, ((size_t)512 << 20) / (hop * sizeof(float))) / A * A);
    size_t at = 0;
    while (at < shorts.size()) {
        out.buffers.emplace_back();
        StagedBuffer& b = out.buffers.back();
        size_t F = (G + A - 1) / A * A;   // the first slot leaves room for the first stream's history too
        b.hash = 1469598103934665603ull;
        auto mix = [&](uint64_t x) { b.hash = (b.hash ^ x) * 1099511628211ull; };
        while (at < shorts.size()) {
            const uint32_t s = shorts[at];
            const size_t len = (n_frames[s] + G + A - 1) / A * A;
            if (!b.slots.empty() && F + len > vcap) break;
            const size_t lead = lead_of ? lead_of[s] : 0;
            const size_t h = std::min(lead, std::min(G * hop, F * hop));   // what of the stream's own history the gap before its slot holds
            b.slots.push_back(BdSlot{F, n_frames[s], (size_t)s * stride});
            const long long prev_end = b.pieces.empty() ? 0ll : b.pieces.back().dst_off + b.pieces.back().count;
            const long long count = (long long)(h + n_frames[s] * hop), dst_off = (long long)(F * hop - h);
            b.pieces.push_back(StagePiece{pcm[s] + (lead - h), count, dst_off, prev_end, dst_off + count});
            b.longest = std::max(b.longest, count);
            mix(F); mix(n_frames[s]); mix((uint64_t)s * stride);
            F += len;
            ++at;
        }
        b.frames = F;
        b.pieces.back().zero_to = (long long)(F * hop);   // (every sample of the buffer is written: a stream's data or a gap's zeros)
    }
    return out;
}

void append_staged_runs(std::vector<StreamRun>& runs, const StagedBuffer& b, const float* staged, size_t hop, size_t r) {
    const size_t first = runs.size();
    append_interleaved_runs(runs, staged, 0, b.frames, hop, r, 0);   // (a buffer holds at least one tile of every grid: r runs)
    for (size_t i = first; i < runs.size(); ++i) {
        StreamRun& S = runs[i];
        S.out_row0 = 0;   // (unused: the slots name the rows)
        S.slots = b.slots.data();
        S.n_slots = b.slots.size();
        S.grid_i = i - first;
        S.slot_hash = b.hash;
    }
}

}  // namespace pvq
