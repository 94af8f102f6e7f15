// overlay_batch.hpp — the spectrogram quad and the chroma boxes (overlay_host.hpp) for MANY streams on the GPU: every (stream,
// frame) row of spectrogram texels and chroma strengths that RenderBatch leaves in device memory is blended, in place, over the
// row's finished picture [H][W][4] of linear f32 (BackdropBatch, then RasterBatch::frames_device(.., over = true)).  Stateful: the
// handle keeps every stream's last history_rows rows — n_streams * history_rows * n_bins * 4 bytes — and the number of frames seen.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "overlay_host.hpp"

namespace pvq {

class OverlayBatch {
   public:
    // The arguments are checked before any device is touched.  history_rows 0: the viewer's 200; ui_scale 0: 1; quad (cx, cy, ex,
    // ey) or null: the reference's; colors 12 RGB triples or null.  device_id < 0: a host-only object whose device calls return
    // PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, uint32_t history_rows, float viewport_height,
                             float ui_scale, const float* quad, const float* colors, uint32_t n_streams, uint32_t width, uint32_t height,
                             std::unique_ptr<OverlayBatch>& out);
    // n_frames frames of every stream, in order.  d_rows null: no quad, and the rings do not advance; d_chroma null: no boxes.
    // Asynchronous on `stream`; one handle's calls are stream-ordered.
    pvq_status frames_device(size_t n_frames, const uint8_t* d_rows, const float* d_chroma, float* d_image_inout, hipStream_t stream);
    // one stream's ring as the reference's texture would stand after the frames seen: out [history_rows][n_bins][4] (synchronises)
    pvq_status get_texture(uint32_t stream_index, uint8_t* out, uint32_t* write_index);
    uint32_t history_rows() const { return h_; }

   private:
    OverlayBatch() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0, n_bins_ = 0, h_ = 0, width_ = 0, height_ = 0;
    float vh_ = 0.0f, ui_scale_ = 1.0f;
    float quad_[4] = {0.0f, 0.0f, 1.0f, 1.0f};
    uint64_t seen_ = 0;      // frames of every stream drawn with rows so far
    uint32_t n_tiles_ = 0;
    DeviceBuffer ring_;      // [n_streams][history_rows][n_bins] texels; row k is the newest frame whose write index was k
    DeviceBuffer tables_;    // overlay::Tables
    DeviceBuffer tiles_;     // [n_tiles] overlay_tiles' list
};

}  // namespace pvq
