// note_carry.hpp — what lets the note model's windows (note_model.hpp) continue from one call to the next: per stream the last
// t_frames - 1 dB frames it was given, and the count of all of them.  A caller that feeds frames as they arrive — one per call is
// the viewer's cadence (ml_system.rs:50-69) — gets a model row for every frame once a stream has seen t_frames - 1 of them, and
// the rows of all streams share tiles: a call of R model rows launches ceil(R / 128) tiles' worth of workgroups per layer.
//
// A call (NoteModel::rows_carry_device) is planned on the host from the counts alone (note_carry_plan, note_model_plan.cpp), one
// descriptor per stream goes to the device, and three small kernels (note_carry.hip) do the rest:
//   nc_stitch     per stream a buffer of 2 (t_frames - 1) frames: the tail, then the call's first frames; every head row's window
//                 (f < t_frames - 1) is one contiguous run of L floats in it
//   nc_rows       expands the descriptors into the row table the model's kernels gather through (NmRow), and the tile list
//   nc_tail_save  the stream's new tail, cut from the stitched buffer when the call is shorter than the tail, else from d_db —
//                 into the tail buffer, which nothing else of the call writes: no frame is shifted in place
// All of it is queued on the call's stream, and nothing is read back.  The descriptors travel from pinned host memory, so their copy
// is queued too; a slot of that memory is written again NC_RING calls later, and only a host that far ahead of the device waits (for
// that one copy).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "note_model_half.hpp"
#include "note_model_plan.hpp"

namespace pvq {

constexpr int NC_RING = 8;   // calls whose descriptors may be on their way at once

class NoteCarry {
   public:
    // for a model of these sizes on this device (device_id < 0: host-only, the counters alone)
    static pvq_status create(const NoteModelDims& d, int device_id, uint32_t n_streams, std::unique_ptr<NoteCarry>& out);
    ~NoteCarry();
    bool fits(const NoteModelDims& d, int device_id) const { return d.n_bins == n_bins_ && d.t_frames == t_frames_ && device_id == device_id_; }
    uint32_t n_streams() const { return n_streams_; }
    // stream_index < 0: every stream.  The stream's count returns to 0 and its tail to zeros (queued on `stream`).
    pvq_status reset(int64_t stream_index, hipStream_t stream);
    pvq_status frames_seen(uint32_t stream_index, uint64_t* out) const;

    // ---- the pieces of a call, in this order ----
    // the plan of the call from the counts (host only)
    pvq_status plan(const NoteModelDims& d, const size_t* n_frames, size_t stride_frames);
    const NcPlan& planned() const { return plan_; }
    // descriptors to the device, the stitched buffers, then the row table and the tiles (d_tiles: planned().tiles entries)
    pvq_status stage(const float* d_db, size_t stride_frames, NmTile* d_tiles, hipStream_t stream);
    const NmRow* rows() const { return rows_.as<NmRow>(); }
    // the new tails; the counts advance
    pvq_status commit(const float* d_db, size_t stride_frames, hipStream_t stream);

   private:
    NoteCarry() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0, n_bins_ = 0, t_frames_ = 0;
    std::vector<uint64_t> seen_;
    NcPlan plan_;
    DeviceBuffer desc_;     // [n_streams] NcStream
    NcStream* staged_ = nullptr;        // pinned: [NC_RING][n_streams], a slot per call in turn
    hipEvent_t copied_[NC_RING] = {};   // recorded behind a slot's copy
    bool in_flight_[NC_RING] = {};
    uint64_t calls_ = 0;
    DeviceBuffer tail_;     // [n_streams][t_frames - 1][n_bins] floats, right-aligned
    DeviceBuffer stitch_;   // [n_streams][2 (t_frames - 1)][n_bins] floats
    DeviceBuffer rows_;     // grow-only: [tiles * 128] NmRow
};

}  // namespace pvq
