// note_model_half.hpp — the note model (note_model.hpp) with its dense layers on the 16-bit matrix instructions of gfx950,
// v_mfma_f32_16x16x32_bf16 / _f16, under the rule of include/pvq.h: conv, ReLU and pool in f32, each pooled feature, dense weight
// and stored hidden activation rounded to the type once, f32 accumulation, f32 bias, ReLU, logits, sigmoid and mask.
//
// Two kernels (note_model_half.hip), one template parameter for the type:
//   nmh_features    conv + ReLU + pool once per row, rounded, written as [rows][pad32(n_features)] in the order k' = 16 p + c
//   nmh_dense<ACT>  one launch per Linear, fc1 included; the output layer writes logits, sigmoid and the 128-bit mask
// NoteModel owns the buffers and drives a call; a PVQ_NOTE_BF16 / PVQ_NOTE_F16 handle calls nmh_chunk below for every chunk of tiles
// where an f32 handle launches nm_conv_fc1 / nm_dense.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pvq.h"
#include "note_model_plan.hpp"

namespace pvq {

constexpr int NM_MAX_DENSE = 10;   // dense layers of a model: fc1, up to 8 hidden layers (note_model_check), the output layer

// what the launches of one chunk of tiles work on, either path: the handle's buffers, nothing owned
struct NmContext {
    NoteModelDims d;
    pvq_note_precision precision = PVQ_NOTE_F32;
    const float* conv = nullptr;                // conv weights [16][5], then bias [16]
    const void* w[NM_MAX_DENSE] = {};           // the packed operand of fc1, of the d.layers hidden layers, of the output layer
    const float* bias[NM_MAX_DENSE] = {};       //   and their biases
    char* ws = nullptr;                         // the workspace
    NmWorkspace at;                             //   and where its pieces lie
};

// one row of a gathered call (note_carry.hip builds the table on the device): where its window of L floats begins, and the row of
// the outputs it writes.  Read by the kernels of both paths as laid out here.
struct alignas(16) NmRow {
    const float* x;
    uint64_t out_row;
};

// the 16-bit launches of the tiles d_tiles[0 .. nt): features, fc1, the hidden layers, the output layer into `outs`.  Queues only.
// d_rows: null, or the row table of these tiles (128 entries a tile).
void nmh_chunk(const NmContext& c, const NmTile* d_tiles, const NmRow* d_rows, uint32_t nt, const float* d_db, size_t stride_frames,
               const pvq_note_model_outputs& outs, hipStream_t stream);

}  // namespace pvq
