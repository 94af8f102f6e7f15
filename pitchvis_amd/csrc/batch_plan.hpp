// batch_plan.hpp — host planning of one batch call, the layer above blockdft_plan.hpp: which path a batch takes (Vqt::run_batch,
// Vqt::resolve_algo and Vqt::batch_streams_device ask the one function below), the interleaved runs of a stream whose hop the block-DFT
// path takes r-fold, and how the short streams of a many-streams call are staged one behind the other.  Plain data in, plain data out:
// no HIP, no environment (developer knobs arrive as arguments).  Compiled by g++ with the other host units and replayed under
// ASan / UBSan by tests/sanitize/host_main.cpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/pvq.h"
#include "blockdft_plan.hpp"

namespace pvq {

// ---- route -----------------------------------------------------------------------------------------------------------------------
enum class BatchRoute {
    Fft,               // the FFT path (any hop)
    BlockStreams,      // the block-DFT path through the stream launch: the fused kernels, every stream as r interleaved runs
    BlockPerStream,    // the block-DFT path one stream per call: the unfused stages, which take the hop only as it is (r == 1)
    RefuseNoHop,       // PVQ_ALGO_BLOCKDFT forced, but no r * hop (r = 1, 2, 4, 8, 16) is a hop the path takes
    RefuseUnfusedHop,  // PVQ_ALGO_BLOCKDFT forced at r > 1 on a geometry that runs the unfused stages
};
// r: Vqt::blockdft_hop_factor(hop) (0: none); takes_streams: whether the fused kernels take streams at hop * r (false at r == 0);
// n_frames: the frames of the call (all streams together); auto_min_frames: auto_block_min_frames(plan, hop, r), read under
// PVQ_ALGO_AUTO at r != 0 only.  The two paths agree to the parity bars, not bit for bit: a caller that pins the path of a larger
// call for its parts (Vqt::resolve_algo) must get what the run functions get, hence ONE function.
BatchRoute route_batch(pvq_algo algo, size_t r, bool takes_streams, size_t n_frames, size_t auto_min_frames);

// PVQ_ALGO_AUTO: the block-DFT path from this many frames on (hop * r its block length)
size_t auto_block_min_frames(const HostPlan& plan, size_t hop, size_t r);

// ---- runs ------------------------------------------------------------------------------------------------------------------------
// One run of frames for the block-DFT path: frame f' (of n_frames) ends at sample first_end + f' * hop of a buffer of n_samples valid
// samples at `pcm` (zeros before it and after it) and goes to output row out_row0 + f' * row_step.  A stream of a many-streams call is
// one run (first_end = n_lead + hop, row_step 1); a hop the path cannot take itself but whose r-fold it can (800 -> 1 600) is r
// interleaved runs of hop r * hop, run i holding the frames i, i + r, ... (first_end = n_lead + (i + 1) hop, row_step r).
// A run may also read a STAGED buffer that holds many short streams one behind the other, each in a slot of whole 64 r-frame tiles
// followed by a gap that is the next stream's history (plan_stream_staging): then `slots` says which output rows the run's frames
// are — frame t of the run is frame grid_i + row_step * t of the staged buffer — and out_row0 is unused.
struct StreamRun {
    const float* pcm;
    size_t first_end, n_samples, n_frames, out_row0, row_step;
    const BdSlot* slots = nullptr;
    size_t n_slots = 0, grid_i = 0;
    uint64_t slot_hash = 0;
};
// the runs as blockdft_plan.hpp takes them: every stream pointer as a sample offset from *base, the lowest of them (never read through)
std::vector<BdStream> rebase_runs(const StreamRun* st, size_t n_st, const float** base);
// A stream of n_frames frames (frame f ends at sample lead + (f + 1) hop, goes to output row row0 + f) as min(r, n_frames) interleaved
// runs of hop r * hop: run i holds the frames i, i + r, ... and writes the rows row0 + i, row0 + i + r, ...
void append_interleaved_runs(std::vector<StreamRun>& runs, const float* pcm, size_t lead, size_t n_frames, size_t hop, size_t r, size_t row0);

// ---- staging of many short streams -----------------------------------------------------------------------------------------------
// Piece p of a staged buffer copies `count` samples from its stream to position dst_off of the buffer and zeroes the gaps around it
// (read by the stage_streams kernel as it is laid out here, vqt_engine.hip).
struct StagePiece {
    const float* src;     // first sample to copy (the stream's pointer + what of its lead does not fit the gap)
    long long count;
    long long dst_off;    // samples from the start of the staging buffer
    long long zero_from;  // the gap before the piece, [zero_from, dst_off), is zeroed by it (the previous piece's end; 0 for the first)
    long long zero_to;    // ... and [dst_off + count, zero_to) behind it (the buffer's end for the last piece, nothing otherwise)
};
// One staged buffer of `frames` frames (frames * hop samples): each stream in a slot of whole 64 r-frame tiles, the zeroed gap
// before it holding what of its history fits.
struct StagedBuffer {
    std::vector<BdSlot> slots;
    std::vector<StagePiece> pieces;   // one per slot; together they write every sample of the buffer
    uint64_t hash = 0;                // of the slot layout (the tile-list cache's key for runs over the buffer)
    long long longest = 0;            // samples of the longest piece
    size_t frames = 0;
};
struct StreamStaging {
    std::vector<StreamRun> longs;         // streams that go as they are (segments of one launch, no copy)
    std::vector<StagedBuffer> buffers;   // filled and analysed one after the other
};
// Stream s holds lead[s] (0 when `lead` is null) + n_frames[s] * hop samples at pcm[s]; its frame f goes to output row s * stride + f.
// Streams of at most stage_max frames are staged, unless there is only one of them; a buffer holds at most 144 K frames and 512 MiB
// (a single slot may exceed that).  window_union: the samples a frame reads.
StreamStaging plan_stream_staging(const float* const* pcm, const size_t* lead, const size_t* n_frames, uint32_t n_streams, size_t stride, size_t hop,
                                  size_t r, size_t window_union, size_t stage_max);
inline size_t staging_history_frames(size_t window_union, size_t hop) { return window_union > hop ? (window_union - hop + hop - 1) / hop : 0; }
// the r runs over a staged buffer that lies at `staged`: run i holds the buffer's frames i, i + r, ...; the slots name their rows
void append_staged_runs(std::vector<StreamRun>& runs, const StagedBuffer& b, const float* staged, size_t hop, size_t r);

}  // namespace pvq
