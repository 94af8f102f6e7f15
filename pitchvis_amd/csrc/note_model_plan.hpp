// note_model_plan.hpp — host side of the note model (note_model.hip): the derived sizes, the argument checks, the one-row f32
// forward, and the repacking of the dense weight matrices into the order the kernels' MFMA B operands are read in.  Plain data in,
// plain data out: no HIP, no device pointer, no environment (the blockdft_plan.cpp pattern).
//
// The model is pitchvis_train/train.py:67-99: Conv1d(1, 16, 5, stride 2) -> ReLU -> max_pool1d(2) -> flatten -> Linear -> ReLU ->
// layers x (Linear -> ReLU) -> Linear(., 128) -> sigmoid, over a window of t_frames dB frames.
#pragma once

#include <algorithm>
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

// the host copy of the weights and the one-row forward (ml_system.rs:24-69) in plain f32, sums in ascending index order.  With a
// 16-bit precision the dense weights are rounded once in assign and infer follows the rule of include/pvq.h: the conv as the fmaf
// chain the kernels run, features and hidden activations rounded by note_round, f32 sums in ascending index order.
struct NoteModelHost {
    NoteModelDims d;
    pvq_note_precision precision = PVQ_NOTE_F32;
    std::vector<float> conv_w, conv_b, fc1_w, fc1_b, out_w, out_b;
    std::vector<std::vector<float>> layer_w, layer_b;
    void assign(const NoteModelDims& dims, const pvq_note_model_weights& w, pvq_note_precision prec = PVQ_NOTE_F32);
    void infer(const float* window, float* out_prob) const;
};

// ---- the 16-bit path (note_model_half.hip) ----
constexpr int NM_KC16 = 32;   // K of a chunk there: one v_mfma_f32_16x16x32_{bf16,f16}; a stage is NM_PC chunks, 16 KiB as above
inline uint32_t note_model_pad32(uint32_t k) { return (k + NM_KC16 - 1) / NM_KC16 * NM_KC16; }

// x rounded to nearest even to the type, as f32 (include/pvq.h pvq_note_round); PVQ_NOTE_F32: x
float note_round(pvq_note_precision prec, float x);
inline bool note_precision_known(int prec) { return prec == PVQ_NOTE_F32 || prec == PVQ_NOTE_BF16 || prec == PVQ_NOTE_F16; }
// the 16 bits of a value note_round returned (bf16: the upper half of the f32; f16: the IEEE binary16 encoding)
uint16_t note_bits16(pvq_note_precision prec, float rounded);
// PVQ_NOTE_F16: a dense weight beyond +-65504 is refused with the layer named; else PVQ_OK
pvq_status note_model_check_range(const NoteModelDims& d, const pvq_note_model_weights& w, pvq_note_precision prec, std::string& err);

// W [n][k] row-major -> the packed operand of nmh_dense, 16-bit twin of note_model_pack_b:
//   packed[column tile ct][chunk kc][strip s][lane l][j] = bits16(round(W[col][kmap(32 kc + 8 (l >> 4) + j)])), j = 0 .. 7,
//   col = 64 ct + 16 ((l & 15) >> 2) + 4 s + (l & 3)
// The kernel gives W as the instruction's A operand (lane l: matrix row l & 15, k = 8 (l >> 4) .. + 7) and the activations as B,
// so lane l's accumulator register r of strip s is activation row l & 15, matrix row 4 (l >> 4) + r: with the column numbering
// above, column 64 ct + 16 (l >> 4) + 4 s + r, and a lane holds 16 consecutive columns of one row.  k' past k (a half chunk when
// k is an odd multiple of 16), chunks past the last up to whole stages of NM_PC, and columns past n are zero.
// conv_order: k' = 16 p + c stands for feature c * o_pool + p (fc1); else k' = k.
std::vector<uint16_t> note_model_pack_b16(const float* W, uint32_t n, uint32_t k, bool conv_order, uint32_t o_pool, pvq_note_precision prec);
inline uint32_t note_model_stages16(uint32_t k) { return (note_model_pad32(k) / NM_KC16 + NM_PC - 1) / NM_PC; }

// ---- windows that continue across calls (note_carry.hip): the plan of one call ----
// A stream has been given seen[s] frames before the call and gets n now.  Frame f of the call is a model row when seen + f >=
// t_frames - 1; the model rows of all streams are numbered stream by stream, frame by frame, and 128 consecutive numbers are a
// tile, whatever streams they come from.  One descriptor per stream goes to the device, where note_carry_row expands it.
#if defined(__HIPCC__)
#define PVQ_NC_HD __host__ __device__ inline
#else
#define PVQ_NC_HD inline
#endif
struct alignas(16) NcStream {
    uint32_t first_row;   // table row of the stream's first model row
    uint32_t f_first;     // the call's frame that row stands for: max(0, t_frames - 1 - seen), at most n
    uint32_t rows;        // model rows: n - f_first
    uint32_t head;        // how many of them are head rows, f < t_frames - 1: their window begins before the call
    uint32_t n;           // frames given in this call
    uint32_t pad[3];
};
struct NcPlan {
    std::vector<NcStream> streams;
    uint64_t total_rows = 0, tiles = 0;   // tiles = ceil(total_rows / 128)
    uint32_t max_rows = 0, max_n = 0;     // the largest of a stream
};
// n_frames null: every stream gets stride_frames.  The caller has checked n_frames[s] <= stride_frames <= 2^31 - 1.
// PVQ_ERR_INVALID_ARG (text in err) when the call has 2^31 model rows or more.  `out` is reused: no allocation once it has n_streams entries.
pvq_status note_carry_plan(const NoteModelDims& d, const uint64_t* seen, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                           NcPlan& out, std::string& err);
// The stitched buffer of a stream holds 2 (t_frames - 1) frames: the tail (the last frames before the call, right-aligned) in the
// first half, then the call's first min(n, t_frames - 1) frames.  Model row i of stream s stands for frame f = f_first + i:
//   in_stitch  f < t_frames - 1: the window is floats [at, at + L) of the stream's stitched buffer (at = f * n_bins);
//              else floats [at, at + L) of d_db, at = (s * stride_frames + f - (t_frames - 1)) * n_bins
//   out_row    s * stride_frames + f
struct NcRow {
    bool in_stitch;
    uint64_t at, out_row;
};
PVQ_NC_HD NcRow note_carry_row(const NcStream& st, uint32_t s, uint32_t i, uint32_t t_frames, uint32_t n_bins, uint64_t stride_frames) {
    const uint64_t f = static_cast<uint64_t>(st.f_first) + i;
    NcRow r;
    r.in_stitch = f < t_frames - 1u;
    r.at = (r.in_stitch ? f : s * stride_frames + f - (t_frames - 1u)) * n_bins;
    r.out_row = s * stride_frames + f;
    return r;
}
// after the call: the frames a stream's tail holds, min(t_frames - 1, seen + n)
inline uint64_t note_carry_tail_frames(const NoteModelDims& d, uint64_t seen_after) { return std::min<uint64_t>(d.t_frames - 1u, seen_after); }

// ---- the workspace of a call, every precision ----
// The tile table (rounded up to 256 bytes), then per chunk of tiles two hidden buffers: PVQ_NOTE_F32 [rows][mlp] floats; 16-bit
// [rows][pad32(mlp)] of 2 bytes a value, behind the rounded features [rows][pad32(n_features)].  chunk_tiles: the whole tiles that
// fit `limit`, at least one, at most n_tiles and what a launch's grid takes.  feat_at, kf_pad and mlp_pad are the 16-bit path's and
// stay zero for PVQ_NOTE_F32.
struct NmWorkspace {
    size_t tab_bytes = 0, tile_bytes = 0, chunk_tiles = 0;
    size_t feat_at = 0, h_at[2] = {0, 0}, total = 0;   // byte offsets
    uint32_t kf_pad = 0, mlp_pad = 0;
};
NmWorkspace note_model_workspace(const NoteModelDims& d, pvq_note_precision precision, size_t n_tiles, uint64_t limit);
// the 16-bit cut under the name it had before the f32 cut joined it (bf16 and f16 share it): a program written against that name keeps building
using NmHalfWorkspace = NmWorkspace;
inline NmHalfWorkspace note_model_half_workspace(const NoteModelDims& d, size_t n_tiles, uint64_t limit) {
    return note_model_workspace(d, PVQ_NOTE_BF16, n_tiles, limit);
}

}  // namespace pvq
