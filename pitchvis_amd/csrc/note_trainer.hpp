// note_trainer.hpp — the trainer's optimisation step (pitchvis_train/train.py:108-162) for the note model of note_model.hpp, on the
// GPU: forward in training mode over a batch of rows gathered by index from a dataset in device memory, BCE loss, backward, Adam.
// The handle owns the parameters in PyTorch layout ([out][in]: they change every step, so the inference kernels' host-packed operand
// is of no use), their gradients and Adam's moments as four equal arenas (note_trainer_plan.hpp), and a workspace sized once from
// max_batch; a step allocates nothing.
//
// Kernels (note_trainer.hip), all matrix work exact f32 on v_mfma_f32_16x16x4_f32:
//   nt_features     conv + ReLU + pool of every gathered row -> feat [batch][n_features]
//   nt_gemm<MODE>   one 64 x 64 tile kernel in three operand orientations: NT  Z = H W^T (forward), NN  dH = dZ W (data gradient,
//                   W transposed while it is staged into LDS), TN  dW = dZ^T H (weight gradient, K = batch, tail rows read as zeros);
//                   bias / ReLU / dropout and the backward gate live in its epilogue.  A product with few tiles is split along K
//                   into partial sums that nt_gemm_finish adds in split order (a fixed order: nothing is accumulated atomically)
//   nt_loss, nt_loss_final   stable BCE from the logits, dZ of the output layer, the mean as a two-level sum in double
//   nt_bias_grad    column sums in a fixed order
//   nt_conv_grad, nt_conv_reduce   dFeat through pool and ReLU to the 96 conv gradients: per row, then over rows, fixed order
//   nt_adam         one launch over the arena
// A handle created with PVQ_NOTE_BF16 runs nt_features, nt_gemm and nt_bias_grad's work in note_trainer_half.hip instead (bf16 operands,
// f32 sums; the arenas, nt_loss, the conv gradient, nt_adam and the test pass's kernels are shared), picked by precision_ in forward and backward.
// The test pass (train.py:164-198) runs the same forward without dropout over chunks of at most max_batch rows, then
//   nt_test_rows    per row: the 128-bit masks of prediction (z > 0) and label (y > 0.5) by wave ballots, tp / fp / fn / correct by
//                   popcount, the row's loss as nt_loss's tree in double, the logits when asked; indexed by the position in idx
//   nt_test_batches one wave per test batch: its rows' records added, the loss in double in an order fixed by the row count
//   nt_test_pitches tp / fp / fn per output over all rows, from the masks
// An epoch (train.py:147-162) is a host loop of the step's launches on one stream: the split goes up once, note_epoch.hip writes its
// gathered order, each batch's slice reaches the step's index array by a device-to-device copy, and the batch losses come back in one read.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "note_trainer_half.hpp"
#include "note_trainer_plan.hpp"

namespace pvq {

class NoteTrainer {
   public:
    // every check runs before any device is touched.  device_id < 0: a host-only object (step returns PVQ_ERR_NO_DEVICE after its
    // argument checks, read returns it at once).
    static pvq_status create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                             const pvq_note_trainer_hyper* hyper, uint32_t max_batch, std::unique_ptr<NoteTrainer>& out) {
        return create(device_id, params, weights, hyper, max_batch, PVQ_NOTE_F32, out);
    }
    // precision: PVQ_NOTE_F32 (the entry above) or PVQ_NOTE_BF16 (note_trainer_half.hpp); anything else is refused with the other checks
    static pvq_status create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                             const pvq_note_trainer_hyper* hyper, uint32_t max_batch, pvq_note_precision precision, std::unique_ptr<NoteTrainer>& out);
    ~NoteTrainer();
    pvq_note_precision precision() const { return precision_; }
    const NoteModelDims& dims() const { return lay_.d; }
    size_t n_params() const { return lay_.n_params; }
    uint64_t steps() const { return steps_; }
    // idx: HOST array.  Asynchronous on `stream`; uses the handle's workspace, so one stream at a time.
    pvq_status step(int mode, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, uint32_t batch, float* d_loss,
                    float* d_logits, hipStream_t stream);
    // train.py:164-198 over idx[0 .. n_idx) (HOST) in test batches of `batch`; fills the HOST outputs, so it waits on `stream` at its end.
    // Leaves the counter, the weights, the gradients and the moments as they are.
    pvq_status test(const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx, uint32_t batch,
                    pvq_note_test_batch* out_batches, uint32_t* out_pitch, float* d_logits, hipStream_t stream);
    // train.py:147-162, one epoch over idx[0 .. n_idx) (HOST) in the order of note_epoch_math.hpp: every batch one PVQ_TRAIN_STEP with the
    // bits of step() on that batch at that counter.  Fills the HOST outputs (each may be null), so it waits on `stream` at its end.
    pvq_status epoch(const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx, uint32_t batch, uint64_t shuffle_seed,
                     uint64_t epoch, float* out_losses, double* out_mean_loss, hipStream_t stream);
    // the arena `what` names, n_params floats in state_dict order -> host.  Synchronises the device.
    pvq_status read(int what, float* out, size_t capacity);
    // host -> the arena `what` names, the inverse of read; a bf16 handle's shadow follows its weights.  Synchronises the device.
    pvq_status write(int what, const float* host, size_t count);
    pvq_status set_steps(uint64_t steps);

   private:
    NoteTrainer() = default;
    // rows -> pinned slot -> the workspace's index array, on `stream`
    pvq_status upload_idx(const uint32_t* idx, uint32_t rows, hipStream_t stream);
    // what step() queues once the workspace's index array holds the batch: forward, loss, and by `mode` backward, Adam, the shadow
    // refresh; PVQ_TRAIN_STEP advances the counter.  Shared by step() and epoch().
    pvq_status run_step(int mode, const float* d_db, const float* d_targets, uint32_t batch, float* d_loss, float* d_logits, hipStream_t stream);
    // train.py:87-99 on the rows the workspace's index array names: features, fc1, the hidden layers, the logits Z.  Queues only.
    void forward(const float* d_db, uint32_t batch, bool train, hipStream_t stream);
    // backward from nt_loss's dZ: every dense gradient of the arena and dfeat.  Queues only.
    void backward(uint32_t batch, hipStream_t stream);
    // the buffers of a bf16 step (precision_ == PVQ_NOTE_BF16)
    NthContext half_context() const;
    int device_id_ = -1;
    pvq_note_precision precision_ = PVQ_NOTE_F32;
    NoteTrainerLayout lay_;
    NoteTrainerHalfPlan half_;   // bf16 only
    DeviceBuffer shadow_;        //   the 16-bit copies of the dense weights, refreshed after every nt_adam
    DeviceBuffer ws16_;          //   the 16-bit workspace, sized once from max_batch
    pvq_note_trainer_hyper hyper_{};
    uint32_t max_batch_ = 0;
    uint64_t steps_ = 0;     // completed PVQ_TRAIN_STEP calls: Adam's t - 1, and the step the dropout mask is keyed by
    uint64_t calls_ = 0;     // picks the pinned slot
    DeviceBuffer arena_;     // floats: weights, gradients, m, v: 4 x n_params
    DeviceBuffer ws_;        // floats, sized once from max_batch
    float* ws(size_t at) const { return ws_.as<float>() + at; }   // at: one of the float offsets below
    uint32_t* h_idx_[2] = {nullptr, nullptr};   // pinned staging of idx, two slots so that a call may be queued behind a running one
    hipEvent_t idx_copied_[2] = {nullptr, nullptr};
    bool idx_pending_[2] = {false, false};
    // the test pass: per-row masks, counts and losses (grow-only), the batch records and pitch counts and their pinned copy
    DeviceBuffer test_rows_, test_out_;
    void* h_test_out_ = nullptr;
    size_t h_test_out_bytes_ = 0;
    // an epoch (NoteTrainerEpochPlan): the split, its gathered order and the batch losses (grow-only), the pinned staging of both ends
    DeviceBuffer epoch_buf_;
    uint32_t* h_epoch_ = nullptr;
    size_t h_epoch_bytes_ = 0;
    // float offsets into the workspace
    size_t ws_feat_ = 0, ws_dfeat_ = 0, ws_h_ = 0, ws_da_ = 0, ws_z_ = 0, ws_dz_ = 0, ws_convpart_ = 0, ws_rowloss_ = 0, ws_part_ = 0, ws_idx_ = 0;
};

}  // namespace pvq
