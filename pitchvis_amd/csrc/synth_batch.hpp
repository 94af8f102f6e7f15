// synth_batch.hpp — the synthesizer's audio rate (synth_math.hpp) for MANY streams on the GPU: a wavefront per stream, a lane per
// voice object (maximum_polyphony <= 64 is one wave).  The host plans every stream's blocks (synth_host.hpp: the control rate and
// every decision), the plan is uploaded, and the device replays it: oscillator, filter, gain products and the sum in the plan's
// record order, so left / right rows carry the bits of SynthState::render.  The rows stay in device memory: they are what
// AgcBatch::condition_device takes.  Between calls the handle keeps every lane's position and filter memory on the device and every
// stream's control state on the host: a render in two calls equals one call.
// With effects (enable_reverb_and_chorus: synth_fx_math.hpp) a second kernel replays the plan and its sends, and the handle also owns
// every stream's effect state on the device: the 24 reverb buffers, the 16 filter stores, the two chorus rings and a sample count.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "synth_host.hpp"

namespace pvq {

class SynthBatch {
   public:
    // The arguments are checked before any device is touched (SynthState::create's checks and texts; n_streams >= 1).
    // device_id < 0: a host-only object whose render_device returns PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, std::shared_ptr<const SynthBank> bank, uint32_t n_streams, int32_t sample_rate, uint32_t maximum_polyphony,
                             std::unique_ptr<SynthBatch>& out, bool effects = false);
    ~SynthBatch();
    uint32_t n_streams() const { return n_streams_; }
    // events / n_blocks [n_streams]; d_left / d_right: HOST arrays of n_streams device pointers to rows of n_blocks[s] * 64 floats
    // (4-byte aligned; nothing past them is written).  snapshot_blocks as SynthState::plan's, shared by the streams.  The planner
    // runs first, on at most 16 threads: a read outside wave_data is PVQ_ERR_INVALID_ARG before anything is launched (the handle is
    // then no longer usable).  Asynchronous on `stream`; the calls of one object go to one stream.
    pvq_status render_device(const SynthEvents* events, const size_t* n_blocks, float* const* d_left, float* const* d_right, const uint32_t* snapshot_blocks,
                             size_t n_snapshots, hipStream_t stream);
    // The last call's cost: out4 = the planner's host time, the host time spent laying the plan out for the upload, the device time of
    // the upload and of the replay kernel, all in ms (waits for the call's end); out_records: the voice-blocks it replayed.
    pvq_status last_times(float* out4, uint64_t* out_records);
    // the last call's snapshots of stream s
    const SynthPlan* plan_of(uint32_t s) const { return s < n_streams_ ? &plans_[s] : nullptr; }
    uint32_t active_voice_count(uint32_t s) const { return s < n_streams_ ? states_[s]->active_voice_count() : 0; }

   private:
    SynthBatch() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0;
    bool broken_ = false;
    bool effects_ = false;
    float master_volume_ = 0.5f;
    std::shared_ptr<const SynthBank> bank_;
    std::vector<std::unique_ptr<SynthState>> states_;
    std::vector<SynthPlan> plans_;
    std::vector<unsigned char> h_tab_;        // what the running call uploads: alive until the next call has waited for `uploaded_`
    std::vector<uint32_t> h_block_ptr_;
    std::vector<synth::Record> h_records_;
    std::vector<synth::Sends> h_sends_;
    hipEvent_t uploaded_ = nullptr, began_ = nullptr, ended_ = nullptr;   // around the upload and the kernel of the running call
    float plan_ms_ = 0.0f, stage_ms_ = 0.0f;
    bool timed_ = false;
    uint64_t last_records_ = 0;
    DeviceBuffer wave_;      // [n_wave] int16, padded to 16 bytes
    DeviceBuffer descs_;     // [n_ir] SampleDesc
    DeviceBuffer lanes_;     // [n_streams][2][64] 16-byte pieces: position and descriptor index; filter memory
    DeviceBuffer tab_;       // [n_streams] stream descriptors of the running call
    DeviceBuffer block_ptr_; // grow-only: every stream's [n_blocks + 1] record indices
    DeviceBuffer records_;   // grow-only: every stream's records
    DeviceBuffer sends_;     // grow-only: every stream's sends (effects)
    // effects: one allocation per kind, zeroed at create
    DeviceBuffer fx_layout_; // synth::FxLayout
    DeviceBuffer fx_table_;  // the chorus delay table
    DeviceBuffer fx_reverb_; // [n_streams][layout.total]
    DeviceBuffer fx_store_;  // [n_streams][16]
    DeviceBuffer fx_ring_;   // [n_streams][2][layout.ring]
    DeviceBuffer fx_count_;  // [n_streams] uint64: samples rendered
};

}  // namespace pvq
