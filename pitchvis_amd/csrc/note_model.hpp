// note_model.hpp — the trainer's note model (pitchvis_train/train.py:67-99; run per frame by pitchvis_viewer/src/ml_system.rs:24-69)
// for MANY rows on the GPU: a row is one frame of one stream, its input the window of t_frames dB frames ending there, read in
// place from the [n_streams][stride_frames][n_bins] buffer the batched transform writes.
//
// Two kernels, exact f32 on v_mfma_f32_16x16x4_f32 (note_model.hip):
//   nm_conv_fc1   conv + ReLU + pool computed in registers as the A operand of the first Linear; the [rows][n_features]
//                 activation never exists in memory
//   nm_dense<ACT> one launch per further Linear; the output layer writes logits, sigmoid and the 128-bit mask in its epilogue
// A handle created with PVQ_NOTE_BF16 or PVQ_NOTE_F16 runs the kernels of note_model_half.hip instead (note_model_half.hpp).  Either
// way NoteModel::rows_device is the one driver: the argument checks, the zeroed outputs, the tile list, the planned workspace
// (note_model_workspace), the loop over chunks of whole tiles that fit its limit.  Two things are per precision: how a dense layer
// is packed when it is uploaded, and the launches of one chunk.
// NoteModelHost (note_model_plan.hpp) is the one-row host face.  rows_carry_device is the same driver over a row table that
// note_carry.hip builds on the device: the four places of the kernels that name a row's window or output row read the table instead.
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

class NoteCarry;

class NoteModel {
   public:
    // sizes and pointers are checked before any device is touched, then (PVQ_NOTE_F16) the range of the dense weights.  device_id < 0:
    // a host-only object (infer works, rows_device returns PVQ_ERR_NO_DEVICE after its argument checks).
    static pvq_status create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                             std::unique_ptr<NoteModel>& out) {
        return create(device_id, params, weights, PVQ_NOTE_F32, out);
    }
    // precision: one of pvq_note_precision (the caller has checked that)
    static pvq_status create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                             pvq_note_precision precision, std::unique_ptr<NoteModel>& out);
    ~NoteModel();
    const NoteModelDims& dims() const { return host_.d; }
    pvq_note_precision precision() const { return host_.precision; }
    int device() const { return device_id_; }
    void infer(const float* window, float* out_prob) const { host_.infer(window, out_prob); }
    // n_frames: HOST array or null.  Asynchronous on `stream`; uses the handle's workspace, so one stream at a time.
    pvq_status rows_device(const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                           const pvq_note_model_outputs& outs, hipStream_t stream);
    // The same with windows that continue from the carry's last call (note_carry.hpp): n_frames[s] NEW frames per stream, row (s, f)
    // a model row when the stream has seen t_frames - 1 frames before it, the rows of all streams packed into shared tiles.
    pvq_status rows_carry_device(NoteCarry& carry, const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                                 const pvq_note_model_outputs& outs, hipStream_t stream);
    void set_workspace_limit(uint64_t bytes) { ws_limit_ = bytes; }

   private:
    NoteModel() = default;
    struct Layer {
        DeviceBuffer buf;     // the operand packed for the precision's kernel, then the f32 bias
        size_t bias_at = 0;   // byte offset of the bias, a multiple of 16
    };
    pvq_status upload(const float* W, const float* bias, uint32_t n, uint32_t k, bool conv_order, Layer& l);
    // the pieces of a row call (note_model.hip)
    pvq_status check_rows(const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames, const pvq_note_model_outputs& outs) const;
    pvq_status zero_outputs(size_t rows_all, const pvq_note_model_outputs& outs, hipStream_t stream);
    pvq_status prepare(size_t n_tiles, NmContext& c);
    pvq_status run(const NmContext& c, size_t n_tiles, const NmRow* d_rows, const float* d_db, size_t stride_frames,
                   const pvq_note_model_outputs& outs, hipStream_t stream);
    int device_id_ = -1;
    NoteModelHost host_;
    uint64_t ws_limit_ = 256ull << 20;
    DeviceBuffer conv_;          // floats: conv weights [16][5], then bias [16]
    Layer fc1_, out_;
    std::vector<Layer> layer_;   // the hidden layers
    DeviceBuffer ws_;            // grow-only: NmWorkspace
};

}  // namespace pvq
