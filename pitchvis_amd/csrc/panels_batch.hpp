// panels_batch.hpp — the debug panels (panels_host.hpp: spectrum line with peak discs, calmness histogram, scene calmness graph;
// update.rs:474-869) for MANY streams on the GPU.
//
// Two calls, split by what recurs (panels_batch.hip):
//   * rows_device — stateless like RenderBatch: a row is one frame of one stream, a wavefront builds its spectrum and histogram
//     meshes from the arrays pvq_analysis_batch_outputs describes.
//   * graph_device — the graph keeps a history, yet every frame's mesh is a function of the `capacity` values that end at that frame
//     of [history | the call's values]: one frame-parallel kernel writes the emitted frames' meshes from that halo, a small kernel
//     behind it moves every stream's history on into the handle's other buffer.  No recurrence over frames, no host synchronisation.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"

namespace pvq {

class PanelsBatch {
   public:
    // colors: 12 RGB triples (null: pitchvis_colors::COLORS).  The arguments are checked before any device is touched; bin counts
    // 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond); graph_capacity 2 .. 1024, 0: 300.  device_id < 0: a host-only object whose device calls
    // return PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const float* colors, float gray_level,
                             uint32_t n_streams, uint32_t graph_capacity, std::unique_ptr<PanelsBatch>& out);
    uint32_t n_bins() const { return n_bins_; }
    uint32_t n_streams() const { return n_streams_; }
    uint32_t graph_capacity() const { return capacity_; }
    // Every requested output for n_rows rows.  Asynchronous on `stream`; the tables are read-only after create, so calls on several
    // streams may overlap.
    pvq_status rows_device(size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center, const float* d_size,
                           const uint32_t* d_peak_count, uint32_t max_peaks, const float* d_calmness, const pvq_panels_outputs& outs,
                           hipStream_t stream);
    // Every stream's history advances by n_frames values of d_scene_calmness [n_streams][n_frames]; meshes for frames first_emitted ..
    // n_frames - 1.  Asynchronous on `stream`; one handle's calls are stream-ordered.
    pvq_status graph_device(size_t n_frames, const float* d_scene_calmness, size_t first_emitted, float* graph_pos, float* graph_rgba,
                            hipStream_t stream);
    // one stream's history after the last call, oldest first (synchronises the device)
    pvq_status get_history(uint32_t stream_index, float* out);

   private:
    PanelsBatch() = default;
    int device_id_ = -1;
    uint32_t n_bins_ = 0, bpo_ = 0, n_streams_ = 0, capacity_ = 0;
    DeviceBuffer tab_;           // PanelTables (panels_batch.hip)
    DeviceBuffer hist_;          // [2][n_streams][capacity] floats: the histories, and where the next call leaves them
    int cur_ = 0;                // which half holds the histories
};

}  // namespace pvq
