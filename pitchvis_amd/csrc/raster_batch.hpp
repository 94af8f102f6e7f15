// raster_batch.hpp — the pitch balls as pixels (raster_host.hpp) for MANY streams on the GPU: every (stream, frame) row of ball
// records that SceneBatch leaves in device memory becomes an image [H][W][4] of linear f32, without the records leaving the device.
//
// The handle keeps one thing between calls: params.time of every ball, which the viewer sets to the clock only for balls a peak
// keys in the frame (update.rs:239), so a fading ball's noise and pulses freeze.  The work is split by what recurs
// (raster_batch.hip): the time scan walks the frames, the lists and the tiles are frame-parallel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "raster_host.hpp"

namespace pvq {

class RasterBatch {
   public:
    // The arguments are checked before any device is touched; bin counts 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond), width and height
    // 1 .. 4096, viewport_height 0 (the reference's) or positive and finite.  device_id < 0: a host-only object whose frames_device
    // returns PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                             uint32_t n_streams, uint32_t width, uint32_t height, std::unique_ptr<RasterBatch>& out);
    uint32_t n_bins() const { return n_bins_; }
    float viewport_height() const { return vh_; }
    // n_frames frames of every stream.  Asynchronous on `stream`; one handle's calls are stream-ordered.  over: every row's balls
    // are blended over what d_image holds for that row (the backdrop stage's picture) instead of the clear colour.
    pvq_status frames_device(size_t n_frames, const pvq_raster_inputs& in, const float* elapsed_s, float* d_image, float* d_ball_time,
                             hipStream_t stream, bool over = false);
    // one stream's ball times after the last call (synchronises)
    pvq_status get_times(uint32_t stream_index, float* out);

   private:
    RasterBatch() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0, n_bins_ = 0, width_ = 0, height_ = 0;
    float vh_ = 0.0f;
    float clear_[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    DeviceBuffer time_;      // [n_streams][n_bins] floats: the state
    DeviceBuffer elapsed_;   // grow-only: [n_frames] floats of the call
    DeviceBuffer ws_;        // grow-only: the lists, times, marks and counts of one piece of a call
};

}  // namespace pvq
