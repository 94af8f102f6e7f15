// render_batch.hpp — the viewer's and the LED strip's per-frame products for MANY rows on the GPU: one row is one frame of one stream.
//
// What turns an AnalysisState into something to look at is pure arithmetic on fields the batched analysis already leaves in device
// memory (pvq_analysis_batch_outputs, flattened to n_rows = n_streams * n_frames):
//   * the spectrogram texture row, both SpectrogramModes  — pitchvis_viewer/src/display_system/update.rs:961-1065
//   * the chroma strengths                                — update.rs:1102-1131
//   * the LED frame of the serial consumer                — pitchvis_serial/src/main.rs:122-175
// all coloured by pitchvis_colors::calculate_color (pitchvis_colors/src/lib.rs:86-117).  spectrogram_row / chroma_row / led_frame
// (consumers_host.cpp) stay the one-row host face; this is the batch face of the same arithmetic in the same f32 operation order
// (color_math.hpp is shared), stateless: the texture ring, its flip and the scroll offset stay with the caller.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"

namespace pvq {

class RenderBatch {
   public:
    // colors: 12 RGB triples in [0, 1] (null: pitchvis_colors::COLORS, lib.rs:19-36).  The geometry is checked before any device is
    // touched; it takes the bin counts the batched AnalysisState takes (3 .. 1024).  device_id < 0: a host-only object whose
    // rows_device returns PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave, const float* colors,
                             float gray_level, float easing_pow, std::unique_ptr<RenderBatch>& out);
    uint32_t n_bins() const { return n_bins_; }
    int device() const { return device_id_; }
    // Every requested output (a non-null pointer of outs) for n_rows rows.  d_x_vqt_smoothed [n_rows][n_bins]; d_center / d_size
    // [n_rows][max_peaks], d_peak_count [n_rows] (a count above max_peaks is taken as max_peaks).  Asynchronous on `stream`; the
    // object's tables are read-only after create, so calls on several streams may overlap.
    pvq_status rows_device(size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center, const float* d_size,
                           const uint32_t* d_peak_count, uint32_t max_peaks, const pvq_render_outputs& outs, hipStream_t stream);

   private:
    RenderBatch() = default;
    int device_id_ = -1;
    uint32_t n_bins_ = 0, bpo_ = 0;
    float gray_level_ = 0.0f, easing_pow_ = 0.0f, semitone_offset_ = 0.0f;
    DeviceBuffer tab_;   // RenderTables (render_batch.hip)
};

}  // namespace pvq
