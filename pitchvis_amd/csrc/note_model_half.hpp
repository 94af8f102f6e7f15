// note_model_half.hpp — the note model (note_model.hpp) with its dense layers on the 16-bit matrix instructions of gfx950,
// v_mfma_f32_16x16x32_bf16 / _f16, under the rule of include/pvq.h: conv, ReLU and pool in f32, each pooled feature, dense weight
// and stored hidden activation rounded to the type once, f32 accumulation, f32 bias, ReLU, logits, sigmoid and mask.
//
// Two kernels (note_model_half.hip), one template parameter for the type:
//   nmh_features    conv + ReLU + pool once per row, rounded, written as [rows][pad32(n_features)] in the order k' = 16 p + c
//   nmh_dense<ACT>  one launch per Linear, fc1 included; the output layer writes logits, sigmoid and the 128-bit mask
// The workspace is note_model_half_workspace's (note_model_plan.hpp); rows are processed in chunks of whole tiles that fit its limit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "note_model_plan.hpp"

namespace pvq {

class NoteModelHalf {
   public:
    // precision: PVQ_NOTE_BF16 or PVQ_NOTE_F16.  Checks as NoteModel::create, then the f16 weight range; device_id < 0: host-only
    static pvq_status create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                             pvq_note_precision precision, std::unique_ptr<NoteModelHalf>& out);
    ~NoteModelHalf();
    const NoteModelDims& dims() const { return host_.d; }
    pvq_note_precision precision() const { return host_.precision; }
    void infer(const float* window, float* out_prob) const { host_.infer(window, out_prob); }
    // the contract of NoteModel::rows_device
    pvq_status rows_device(const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                           const pvq_note_model_outputs& outs, hipStream_t stream);
    void set_workspace_limit(uint64_t bytes) { ws_limit_ = bytes; }

   private:
    NoteModelHalf() = default;
    struct Layer {
        DeviceBuffer buf;     // the packed 16-bit operand, then the f32 bias
        size_t bias_at = 0;   // byte offset of the bias
    };
    pvq_status upload(const float* W, const float* bias, uint32_t n, uint32_t k, bool conv_order, Layer& l);
    int device_id_ = -1;
    NoteModelHost host_;
    uint64_t ws_limit_ = 256ull << 20;
    DeviceBuffer conv_;          // floats: conv weights [16][5], then bias [16]
    Layer fc1_, out_;
    std::vector<Layer> layer_;
    DeviceBuffer ws_;            // grow-only: NmHalfWorkspace
};

}  // namespace pvq
