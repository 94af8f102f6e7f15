// note_trainer_plan.hpp — host side of the note trainer (note_trainer.hip): the layout of the parameter arena, the argument checks,
// the per-step Adam constants, the split-K rule of the GEMMs, the dropout mask function, the plan and the metrics of the test
// pass, the plan of an epoch and the checks of a restored checkpoint.  Plain data in, plain data out: no HIP, no device pointer, no
// environment (the note_model_plan.cpp pattern).
//
// The step is pitchvis_train/train.py:108-162: forward in training mode (train.py:87-99), BCELoss, backward, optim.Adam with weight
// decay (train.py:141-144).  The test pass is train.py:164-198, the epoch loop train.py:147-162.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pvq.h"
#include "note_model_plan.hpp"

#ifdef __HIPCC__
#define PVQ_NT_HD __host__ __device__
#else
#define PVQ_NT_HD
#endif

namespace pvq {

constexpr uint32_t NT_MAX_BATCH = 4096;
constexpr int NT_BM = 64;   // rows of a GEMM workgroup tile: 4 waves x one MFMA row tile of 16
constexpr int NT_BN = 64;   // columns: 4 MFMA column strips of 16, all held by every wave
constexpr int NT_BK = 32;   // K of a stage: two chunks of four 16x16x4 steps
constexpr size_t NT_PART_FLOATS = size_t(4) << 20;   // split-K partial sums: splits * M * N never exceeds this (nt_splits)

// One tensor of the flat parameter arena.  The arena is the state_dict in its own order: conv1.weight [16][5], conv1.bias [16],
// fc1.weight [mlp][n_features], fc1.bias [mlp], layers.i.weight [mlp][mlp], layers.i.bias [mlp] for i = 0 .., output.weight
// [128][mlp], output.bias [128].  Every offset is a multiple of 4 floats (every size is), so float4 access is aligned.
struct NtTensor {
    size_t at = 0, n = 0;
};
struct NoteTrainerLayout {
    NoteModelDims d;
    NtTensor conv_w, conv_b, fc1_w, fc1_b, out_w, out_b;
    std::vector<NtTensor> layer_w, layer_b;
    size_t n_params = 0;
};
NoteTrainerLayout note_trainer_layout(const NoteModelDims& d);
// the arena filled from host weights
std::vector<float> note_trainer_arena(const NoteTrainerLayout& lay, const pvq_note_model_weights& w);

// the hyper-parameter and max_batch ranges of include/pvq.h; err receives the text
pvq_status note_trainer_check_hyper(const pvq_note_trainer_hyper* h, uint32_t max_batch, std::string& err);
// the checks of a step that need no device: mode, pointers, n_rows, batch, every index.  err receives the text
pvq_status note_trainer_check_step(const NoteModelDims& d, uint32_t max_batch, int mode, const void* d_db, const void* d_targets, size_t n_rows,
                                   const uint32_t* idx, uint32_t batch, std::string& err);

// The dropout mask (include/pvq.h states it in full).  nt_mix is the splitmix64 finaliser; the layer key folds seed, step and layer
// on the host, the kernel does one nt_mix per element.
PVQ_NT_HD inline uint64_t nt_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
inline uint64_t nt_layer_key(uint64_t seed, uint64_t step, uint32_t layer) {
    return nt_mix(nt_mix(seed + 0x9E3779B97F4A7C15ull * (step + 1)) ^ static_cast<uint64_t>(layer));
}
inline uint32_t nt_keep_threshold(double dropout) { return static_cast<uint32_t>(dropout * 16777216.0); }   // floor(p 2^24)
PVQ_NT_HD inline bool nt_keep(uint64_t layer_key, uint32_t row, uint32_t col, uint32_t threshold) {
    return static_cast<uint32_t>(nt_mix(layer_key ^ ((static_cast<uint64_t>(row) << 32) | col)) >> 40) >= threshold;
}

// Adam's per-step scalars (torch.optim.Adam, train.py:141-144), in double: step_size = lr / (1 - beta1^t), inv_bc2_sqrt = 1 / sqrt(1 - beta2^t)
struct NtAdamStep {
    double beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt;
};
NtAdamStep note_trainer_adam_step(const pvq_note_trainer_hyper& h, uint64_t t);

// K splits of a GEMM of m x n over k: enough workgroups to fill the chip (a fixed 512, not the device's count: the split decides
// the summation order, and equal calls must give equal bits on every device), at least 8 K stages per split, at most 8 splits, and
// splits * m * n within NT_PART_FLOATS.  1: no split, the GEMM writes its result itself.
uint32_t nt_splits(uint32_t m, uint32_t n, uint32_t k);

// The bf16 step (note_trainer_half.hpp; the rule: include/pvq.h, pvq_note_trainer_create_precision).  f32 and bf16 are admitted;
// f16 is refused with the reason, any other value as unknown.  err receives the text
pvq_status note_trainer_check_precision(int precision, std::string& err);
constexpr int NTH_BM = 64;   // nth_gemm's workgroup tile: 2 x 2 waves of 32 x 32
constexpr int NTH_BN = 64;
constexpr int NTH_BK = 64;   // K of a stage: two chunks of 32, one v_mfma_f32_16x16x32_bf16 each
inline uint32_t nth_pad32(uint32_t n) { return (n + 31u) & ~31u; }
// nt_splits for nth_gemm (k: the padded K): the same fixed 512 workgroups, at least 4 stages (256 k) per split, at most 8 splits,
// splits * m * n within NT_PART_FLOATS
uint32_t nth_splits(uint32_t m, uint32_t n, uint32_t k);
// One dense weight W [n][k] of the arena (at float offset src_at) and its two 16-bit copies in the shadow buffer: w_at [n][pad32(k)]
// and wt_at [k][pad32(n)], the padding zeros.  Offsets in 16-bit elements, multiples of 64.
struct NthShadow {
    size_t src_at = 0, w_at = 0, wt_at = 0;
    uint32_t n = 0, k = 0;
};
// The shadow weights (fc1, layers 0 .., output: in that order) and the 16-bit workspace of a handle, sized once from max_batch.  Every
// matrix is kept both ways round, [row][pad32(col)] and [col][pad32(row)], so that every product reads both operands along k; rows of a
// call are laid out densely with the strides of ITS batch (pad32(n_features), pad32(mlp), pad32(batch)), so values do not depend on
// max_batch.  Offsets in 16-bit elements, multiples of 64; h_at and ht_at hold layers + 1 matrices of h_stride and ht_stride each,
// da_at and dat_at two.
struct NoteTrainerHalfPlan {
    std::vector<NthShadow> shadow;
    size_t shadow_total = 0;
    uint32_t f_pad = 0, mlp_pad = 0, b_pad = 0;   // pad32 of n_features, mlp, max_batch
    size_t feat_at = 0, featt_at = 0, h_at = 0, ht_at = 0, dz_at = 0, dzt_at = 0, da_at = 0, dat_at = 0;
    size_t h_stride = 0, ht_stride = 0;
    size_t ws_total = 0;
};
NoteTrainerHalfPlan note_trainer_half_plan(const NoteTrainerLayout& lay, uint32_t max_batch);

// The test pass (train.py:164-198).  Dropout is off, so a row's forward depends on no other row: the forward runs in chunks of at
// most max_batch consecutive entries of idx, a function of n_idx and max_batch alone; `batch` shapes only the counting.
constexpr size_t NT_TEST_MAX_IDX = size_t(1) << 25;   // rows of a pass: 128 * rows, the most a count can reach, stays below 2^32
constexpr size_t NT_TEST_ROW_BYTES = 24 + 32;         // per row: tp, fp, fn, correct and the loss in double; two 128-bit masks
constexpr size_t NT_TEST_PITCH_BYTES = NM_OUT * 3 * sizeof(uint32_t);
struct NtTestChunk {
    size_t begin = 0;     // position in idx
    uint32_t rows = 0;    // 1 .. max_batch
};
struct NoteTrainerTestPlan {
    std::vector<NtTestChunk> chunks;   // in order, back to back, covering 0 .. n_idx
    size_t n_batches = 0;              // ceil(n_idx / batch): the last batch may be short
    size_t rows_bytes = 0;             // device: the per-row records and masks, n_idx * NT_TEST_ROW_BYTES
    size_t out_bytes = 0;              // the one read-back: n_batches records of 32 bytes, then the [128][3] pitch counts
};
NoteTrainerTestPlan note_trainer_test_plan(size_t n_idx, uint32_t max_batch, uint32_t batch);
// the checks of a test pass that need no device; err receives the text
pvq_status note_trainer_check_test(const NoteModelDims& d, const void* d_db, const void* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx,
                                   uint32_t batch, const void* out_batches, std::string& err);
// what train.py:185-198 prints, from the records: the plain mean of the batch F1 scores (2 tp / (2 tp + fp + fn), 0 when that
// denominator is 0), sum of correct / (128 * sum of rows), the plain mean of the batch losses.  An output may be null.
pvq_status note_test_metrics(const pvq_note_test_batch* b, size_t n_batches, double* mean_f1, double* accuracy, double* mean_loss, std::string& err);

// One epoch (train.py:147-162): the DataLoader's shuffle is the order of note_epoch_math.hpp, batch k its entries k * batch ..; the
// last batch may be short and still counts (train.py:64).  The handle keeps one grow-only device buffer and one pinned host buffer
// for it, both laid out in 4-byte words: the split as given, its gathered order, one loss per batch.
constexpr size_t NT_EPOCH_MAX_IDX = size_t(1) << 25;   // as a test pass
struct NoteTrainerEpochPlan {
    size_t n_batches = 0;      // ceil(n_idx / batch)
    uint32_t last_rows = 0;    // rows of the last batch, 1 .. batch
    size_t idx_at = 0, order_at = 0, loss_at = 0;   // device: word offsets of d_idx [n_idx], d_order [n_idx], d_losses [n_batches]
    size_t device_bytes = 0;
    size_t h_idx_at = 0, h_loss_at = 0;             // pinned host: the staged idx [n_idx], the losses read back [n_batches]
    size_t host_bytes = 0;
};
NoteTrainerEpochPlan note_trainer_epoch_plan(size_t n_idx, uint32_t batch);
// the checks of an epoch that need no device: pointers, batch, n_idx, n_rows, every index.  err receives the text
pvq_status note_trainer_check_epoch(const NoteModelDims& d, uint32_t max_batch, const void* d_db, const void* d_targets, size_t n_rows,
                                    const uint32_t* idx, size_t n_idx, uint32_t batch, std::string& err);
// running_loss / len(train_loader) (train.py:162): the batch losses added in double in batch order, over their number
double note_epoch_mean_loss(const float* losses, size_t n_batches);
// out[j] = order(first + j) of note_epoch_math.hpp for j < count, on the host.  Refuses n outside 1 .. 2^32, first + count > n, a null out
pvq_status note_epoch_order(uint64_t seed, uint64_t epoch, uint64_t n, uint64_t first, uint64_t count, uint32_t* out, std::string& err);
// the checks of pvq_note_trainer_write and pvq_note_trainer_set_steps
pvq_status note_trainer_check_write(int what, const void* host, size_t count, size_t n_params, std::string& err);
constexpr uint64_t NT_MAX_STEPS = uint64_t(1) << 53;   // Adam's t = steps + 1 goes through a double (note_trainer_adam_step)
pvq_status note_trainer_check_steps(uint64_t steps, std::string& err);

}  // namespace pvq
