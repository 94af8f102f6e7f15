// condition_batch.hpp — the trainer's stream conditioning for MANY streams on the GPU: downmix, silence gate, MonoAgc.
//
// pitchvis_train conditions every rendered file before the transform (pitchvis_train/src/train.rs:286-301: left := (l + r) / 2, the
// gain frozen for a chunk whose sequential sum of squares is < 1e-6, dagc::MonoAgc::process over the chunk), one file per rayon worker
// (train.rs:146-163).  The AGC is a per-sample recurrence (dagc_fork/src/lib.rs:76-86), so a stream cannot be split over time; streams
// are independent, so here a LANE owns a stream and 64 streams share a wave.  train_condition_stream (consumers_host.cpp) stays the
// single-stream face; this is the batch face of the same arithmetic, in the same f32 operation order, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"

namespace pvq {

class AgcBatch {
   public:
    // n_streams MonoAgc::new(desired_output_rms, distortion_factor) (lib.rs:35-53).  The arguments are checked before any device is
    // touched (MonoAgc::valid, the reference's texts); device_id < 0: a host-only object whose condition_device returns PVQ_ERR_NO_DEVICE.
    static pvq_status create(int device_id, uint32_t n_streams, float desired_output_rms, float distortion_factor, std::unique_ptr<AgcBatch>& out);
    uint32_t n_streams() const { return n_streams_; }
    int device() const { return device_id_; }
    // train.rs:286-301 for every stream.  d_left / d_right / d_mono_out: HOST arrays of n_streams device pointers (d_right null, or an
    // entry null: mono); stream s has n_chunks[s] chunks of `chunk` samples.  d_gain_out (device, may be null): [n_streams][gain_stride],
    // agc.gain() after each chunk.  d_mono_out[s] == d_left[s] is allowed.  Asynchronous on `stream`; the calls of one object go to one
    // stream (or are ordered by the caller): they share its tables and every stream's gain.
    pvq_status condition_device(const float* const* d_left, const float* const* d_right, const size_t* n_chunks, size_t chunk,
                                float* const* d_mono_out, float* d_gain_out, size_t gain_stride, hipStream_t stream);
    // lib.rs:72 for every stream, after the last call (synchronises)
    pvq_status get_gains(float* gains);

   private:
    AgcBatch() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0;
    float desired_output_rms_ = 0.0f, distortion_factor_ = 0.0f;
    DeviceBuffer gain_;      // [n_streams] floats: MonoAgc::gain
    DeviceBuffer tab_;       // [n_streams] stream descriptors of the running call
    DeviceBuffer frozen_;    // grow-only: [max_chunks][n_streams] bytes: the gate of every chunk of the running call
};

}  // namespace pvq
