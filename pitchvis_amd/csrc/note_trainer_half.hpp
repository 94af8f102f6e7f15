// note_trainer_half.hpp — the dense products of the note trainer's step (note_trainer.hpp) on v_mfma_f32_16x16x32_bf16, under the
// rule of include/pvq.h (pvq_note_trainer_create_precision): bf16 operands, f32 accumulation, f32 master weights, gradients and
// Adam moments.  NoteTrainer keeps its arenas, its f32 workspace, nt_loss, the conv gradient, nt_adam and the test pass; a
// PVQ_NOTE_BF16 handle calls the three functions below where an f32 handle runs nt_features / nt_gemm / nt_bias_grad.
//
// Every matrix a product reads is kept in 16 bits both ways round (note_trainer_plan.hpp, NoteTrainerHalfPlan): the instruction
// wants 8 consecutive k per lane from both operands, so with [row][k] copies of H, dZ / dA and W for the products over columns and
// [col][pad32(batch)] copies for the products over the batch all three products of a layer are the one NT form, read from global
// memory in 16-byte pieces and never transposed while staged.  Kernels (note_trainer_half.hip):
//   nth_features      nt_features writing rounded rows [batch][pad32(n_features)]
//   nth_gemm          C = A B^T, 64 x 64 tile, epilogues RAW / BIAS (f32 out) and HIDDEN / GATE (rounded once, stored both ways round);
//                     split along K by nth_splits into f32 partial sums that nth_gemm_finish adds in split order
//   nth_relayout      f32 or bf16 [R][C] -> bf16 [R][pad32(C)] and [C][pad32(R)] through LDS: the shadow weights after nt_adam (one
//                     launch over every dense weight), and per step the output layer's dZ and the transposed features
//   nth_bias_grad     nt_bias_grad's four row phases over the 16-bit dZ / dA
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pvq.h"
#include "note_trainer_plan.hpp"

namespace pvq {

// what a bf16 step works on: the handle's buffers, nothing owned
struct NthContext {
    const NoteTrainerLayout* lay = nullptr;
    const NoteTrainerHalfPlan* plan = nullptr;
    float* arena = nullptr;          // weights, gradients, m, v
    uint16_t* shadow = nullptr;      // plan->shadow_total 16-bit values
    uint16_t* ws16 = nullptr;        // plan->ws_total
    float* part = nullptr;           // NT_PART_FLOATS
    const uint32_t* d_idx = nullptr;
    float* Z = nullptr;              // [batch][128] logits
    float* dZ = nullptr;             // [batch][128], nt_loss's
    float* dfeat = nullptr;          // [batch][n_features]
    pvq_note_trainer_hyper hyper{};
    uint64_t steps = 0;
};

// the dense weights of the arena -> both shadow copies: at create and after every nt_adam
void nth_refresh_shadow(const NthContext& c, hipStream_t stream);
// features, fc1, the hidden layers, the logits Z of the rows d_idx names; train: dropout, and the transposed copies the backward reads
void nth_forward(const NthContext& c, const float* d_db, uint32_t batch, bool train, hipStream_t stream);
// from nt_loss's dZ to every dense gradient of the arena and dfeat
void nth_backward(const NthContext& c, uint32_t batch, hipStream_t stream);

}  // namespace pvq
