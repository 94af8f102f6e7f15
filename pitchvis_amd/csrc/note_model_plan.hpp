// note_model_plan.hpp — host side of the note model (note_model.hip): the derived sizes, the argument checks, the one-row f32
// forward, and the repacking of the dense weight matrices into the order the kernels' MFMA B operands are read in.  Plain data in,
// plain data out: no HIP, no device pointer, no environment (the blockdft_plan.cpp pattern).
//
// The model is pitchvis_train/train.py:67-99: Conv1d(1, 16, 5, stride 2) -> ReLU -> max_pool1d(2) -> flatten -> Linear -> ReLU ->
// layers x (Linear -> ReLU) -> Linear(., 128) -> sigmoid, over a window of t_frames dB frames.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pvq.h"

namespace pvq {

constexpr int NM_CH = 16;    // conv channels (train.py:75)
constexpr int NM_KW = 5;     // conv kernel width, stride 2, pool 2 (train.py:75,90)
constexpr int NM_OUT = 128;  // outputs (ml_system.rs:7)
constexpr int NM_BM = 128;   // rows of a workgroup tile: 4 waves x 2 MFMA row tiles of 16
constexpr int NM_BN = 64;    // columns of a workgroup tile: 4 MFMA column strips of 16, all held by every wave
constexpr int NM_KC = 16;    // K of a chunk: four 16x16x4 steps; the conv's 16 channels of one pooled position
constexpr int NM_PC = 4;     // chunks per K stage (one LDS buffer of the B operand: NM_PC * NM_BN * NM_KC floats = 16 KiB)

struct NoteModelDims {
    uint32_t n_bins = 0, t_frames = 0, mlp = 0, layers = 0;
    uint32_t L = 0, o_conv = 0, o_pool = 0, n_features = 0;
};

// one 128-row tile of one stream: rows f0 .. f0 + n_valid - 1 (frames), n_valid in 1 .. 128.  Read by the kernels as laid out here.
struct alignas(16) NmTile {
    uint32_t stream, f0, n_valid, pad;
};

// the ranges of include/pvq.h; err receives the text
pvq_status note_model_check(const pvq_note_model_params* p, const pvq_note_model_weights* w, NoteModelDims& d, std::string& err);

// W [n][k] row-major -> the B operand of a [rows][k] x [k][n] product, as the kernels read it:
//   packed[column tile ct][chunk kc][strip s][lane l][i] = W[64 ct + 16 s + (l & 15)][kmap(16 kc + 4 (l >> 4) + i)]
// lane l of a wave supplies column l & 15 and k index l >> 4 of a v_mfma_f32_16x16x4_f32; element i of its float4 is the operand of
// the chunk's i-th instruction.  Chunks are padded with zero chunks to a multiple of NM_PC, columns beyond n with zeros.
// conv_order: K is walked pooled position by pooled position, k' = 16 p + c standing for feature c * o_pool + p (fc1); else k' = k.
std::vector<float> note_model_pack_b(const float* W, uint32_t n, uint32_t k, bool conv_order, uint32_t o_pool);
inline uint32_t note_model_stages(uint32_t chunks) { return (chunks + NM_PC - 1) / NM_PC; }

// the tile list of a call, stream by stream (n_frames null: every stream has stride_frames)
std::vector<NmTile> note_model_tiles(const NoteModelDims& d, const size_t* n_frames, uint32_t n_streams, size_t stride_frames);

// the host copy of the weights and the one-row forward (ml_system.rs:24-69) in plain f32, sums in ascending index order
struct NoteModelHost {
    NoteModelDims d;
    std::vector<float> conv_w, conv_b, fc1_w, fc1_b, out_w, out_b;
    std::vector<std::vector<float>> layer_w, layer_b;
    void assign(const NoteModelDims& dims, const pvq_note_model_weights& w);
    void infer(const float* window, float* out_prob) const;
};

}  // namespace pvq
