// scene_batch.hpp — the pitch-ball scene (scene_host.hpp: balls, bass spiral, bloom; update.rs:38-426) for MANY streams on the GPU.
//
// Unlike RenderBatch the scene recurs over frames, so the handle keeps every stream's state between calls, like AnalysisBatch: one
// call advances all streams by n_frames frames, in order, from the arrays pvq_analysis_batch_outputs describes.  The work is split
// by what recurs (scene_batch.hip): a frame-parallel kernel turns every peak into a finished record, a wavefront per stream then
// fades the balls and applies the records frame after frame.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "scene_host.hpp"

namespace pvq {

class SceneBatch {
   public:
    // The arguments are checked before any device is touched; bin counts 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond).  device_id < 0: a
    // host-only object whose frames_device returns PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings* settings,
                             uint32_t n_streams, std::unique_ptr<SceneBatch>& out);
    uint32_t n_bins() const { return s_.n_bins; }
    uint32_t n_streams() const { return n_streams_; }
    uint32_t n_segments() const { return s_.n_segments; }
    // Every stream advances by n_frames frames.  Inputs [n_streams][n_frames][...] (device), frame_times_ns: host array or null.
    // d_ml_prob: [n_streams][ml_stride_frames][128] (device) for the `ml` branch, or null: the branch is off and the stride unread.
    // Asynchronous on `stream`; one handle's calls are stream-ordered.
    pvq_status frames_device(size_t n_frames, const pvq_scene_inputs& in, uint64_t frame_time_ns, const uint64_t* frame_times_ns,
                             const pvq_scene_outputs& outs, hipStream_t stream, const float* d_ml_prob = nullptr, size_t ml_stride_frames = 0);
    // one stream's state after the last call (synchronises the device); any pointer may be null
    pvq_status get_state(uint32_t stream_index, float* ball_xyzs, float* ball_rgba, float* ball_params, uint32_t* ball_visible,
                         uint32_t* bass_lit, float* bass_rgba, float* bloom);

   private:
    SceneBatch() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0;
    scene::Settings s_{};
    DeviceBuffer settings_;   // scene::Settings
    DeviceBuffer state_;      // [n_streams][STATE_FIELDS][n_bins] floats
    DeviceBuffer scalars_;    // [n_streams][8] floats: bass_lit (bits), bass rgba, bloom
    DeviceBuffer rec_;        // grow-only: [rows][max_peaks] PeakRecord, then [rows] row headers
    DeviceBuffer fade_;       // grow-only: [distinct frame times][n_bins + 1] floats: dropoff, z_step
    DeviceBuffer fade_row_;   // grow-only: [n_frames] u32: row of the table
    std::vector<uint64_t> fade_times_;   // the frame times the table on the device holds, row by row
};

}  // namespace pvq
