// note_trainer_plan.cpp — see note_trainer_plan.hpp
#include "note_trainer_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "note_epoch_math.hpp"

namespace pvq {

NoteTrainerLayout note_trainer_layout(const NoteModelDims& d) {
    NoteTrainerLayout lay;
    lay.d = d;
    size_t at = 0;
    auto take = [&at](size_t n) {
        NtTensor t;
        t.at = at;
        t.n = n;
        at += n;
        return t;
    };
    lay.conv_w = take(NM_CH * NM_KW);
    lay.conv_b = take(NM_CH);
    lay.fc1_w = take(static_cast<size_t>(d.mlp) * d.n_features);
    lay.fc1_b = take(d.mlp);
    for (uint32_t i = 0; i < d.layers; ++i) {
        lay.layer_w.push_back(take(static_cast<size_t>(d.mlp) * d.mlp));
        lay.layer_b.push_back(take(d.mlp));
    }
    lay.out_w = take(static_cast<size_t>(NM_OUT) * d.mlp);
    lay.out_b = take(NM_OUT);
    lay.n_params = at;
    return lay;
}

std::vector<float> note_trainer_arena(const NoteTrainerLayout& lay, const pvq_note_model_weights& w) {
    std::vector<float> a(lay.n_params);
    auto put = [&a](const NtTensor& t, const float* src) { std::memcpy(a.data() + t.at, src, t.n * sizeof(float)); };
    put(lay.conv_w, w.conv_weight);
    put(lay.conv_b, w.conv_bias);
    put(lay.fc1_w, w.fc1_weight);
    put(lay.fc1_b, w.fc1_bias);
    for (uint32_t i = 0; i < lay.d.layers; ++i) {
        put(lay.layer_w[i], w.layer_weight[i]);
        put(lay.layer_b[i], w.layer_bias[i]);
    }
    put(lay.out_w, w.output_weight);
    put(lay.out_b, w.output_bias);
    return a;
}

pvq_status note_trainer_check_hyper(const pvq_note_trainer_hyper* h, uint32_t max_batch, std::string& err) {
    if (!h) {
        err = "note trainer: null hyper-parameters";
        return PVQ_ERR_INVALID_ARG;
    }
    // (written so that a NaN fails every test)
    if (!(h->lr > 0.0) || !std::isfinite(h->lr)) {
        err = "note trainer: lr must be a finite positive number";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0)) {
        err = "note trainer: beta1 and beta2 must lie in [0, 1)";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!(h->eps > 0.0) || !std::isfinite(h->eps)) {
        err = "note trainer: eps must be a finite positive number";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!(h->weight_decay >= 0.0) || !std::isfinite(h->weight_decay)) {
        err = "note trainer: weight_decay must be a finite number >= 0";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!(h->dropout >= 0.0 && h->dropout < 1.0)) {
        err = "note trainer: dropout must lie in [0, 1)";
        return PVQ_ERR_INVALID_ARG;
    }
    if (max_batch < 1 || max_batch > NT_MAX_BATCH) {
        err = "note trainer: max_batch must lie in 1 .. 4096";
        return PVQ_ERR_INVALID_ARG;
    }
    return PVQ_OK;
}

namespace {
// the row count of a dataset and every index of a batch, a test pass or an epoch
pvq_status check_rows(const NoteModelDims& d, size_t n_rows, const uint32_t* idx, size_t n, std::string& err) {
    if (n_rows > 0xffffffffull) {
        err = "note trainer: a dataset holds at most 2^32 - 1 rows";
        return PVQ_ERR_INVALID_ARG;
    }
    for (size_t i = 0; i < n; ++i)
        if (idx[i] < d.t_frames - 1 || idx[i] >= n_rows) {
            err = "note trainer: idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [t_frames - 1, n_rows)";
            return PVQ_ERR_INVALID_ARG;
        }
    return PVQ_OK;
}
}  // namespace

pvq_status note_trainer_check_step(const NoteModelDims& d, uint32_t max_batch, int mode, const void* d_db, const void* d_targets, size_t n_rows,
                                   const uint32_t* idx, uint32_t batch, std::string& err) {
    if (mode != PVQ_TRAIN_STEP && mode != PVQ_TRAIN_GRAD && mode != PVQ_TRAIN_EVAL) {
        err = "note trainer: unknown mode";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!d_db || !d_targets || !idx) {
        err = "note trainer: d_db, d_targets or idx is null";
        return PVQ_ERR_INVALID_ARG;
    }
    if (batch < 1 || batch > max_batch) {
        err = "note trainer: batch must lie in 1 .. max_batch (" + std::to_string(max_batch) + ")";
        return PVQ_ERR_INVALID_ARG;
    }
    return check_rows(d, n_rows, idx, batch, err);
}

NtAdamStep note_trainer_adam_step(const pvq_note_trainer_hyper& h, uint64_t t) {
    NtAdamStep s;
    s.beta1 = h.beta1;
    s.beta2 = h.beta2;
    s.eps = h.eps;
    s.weight_decay = h.weight_decay;
    const double td = static_cast<double>(t);
    s.step_size = h.lr / (1.0 - std::pow(h.beta1, td));
    s.inv_bc2_sqrt = 1.0 / std::sqrt(1.0 - std::pow(h.beta2, td));
    return s;
}

uint32_t nt_splits(uint32_t m, uint32_t n, uint32_t k) {
    const uint64_t blocks = static_cast<uint64_t>((m + NT_BM - 1) / NT_BM) * ((n + NT_BN - 1) / NT_BN);
    const uint32_t stages = (k + NT_BK - 1) / NT_BK;
    uint64_t s = std::min<uint64_t>({512 / blocks, stages / 8, 8});
    while (s > 1 && s * m * n > NT_PART_FLOATS) --s;
    return static_cast<uint32_t>(std::max<uint64_t>(s, 1));
}

pvq_status note_trainer_check_precision(int precision, std::string& err) {
    if (precision == PVQ_NOTE_F32 || precision == PVQ_NOTE_BF16) return PVQ_OK;
    if (precision == PVQ_NOTE_F16)
        err = "note trainer: precision f16 is not offered: dZ = (sigmoid(z) - y) / (128 * batch) is about 1e-5 and underflows f16 without loss "
              "scaling; train in bf16 or f32";
    else
        err = "note trainer: precision is none of pvq_note_precision";
    return PVQ_ERR_INVALID_ARG;
}

uint32_t nth_splits(uint32_t m, uint32_t n, uint32_t k) {
    const uint64_t blocks = static_cast<uint64_t>((m + NTH_BM - 1) / NTH_BM) * ((n + NTH_BN - 1) / NTH_BN);
    const uint32_t stages = (k + NTH_BK - 1) / NTH_BK;
    uint64_t s = std::min<uint64_t>({512 / blocks, stages / 4, 8});
    while (s > 1 && s * m * n > NT_PART_FLOATS) --s;
    return static_cast<uint32_t>(std::max<uint64_t>(s, 1));
}

NoteTrainerHalfPlan note_trainer_half_plan(const NoteTrainerLayout& lay, uint32_t max_batch) {
    const NoteModelDims& d = lay.d;
    NoteTrainerHalfPlan p;
    auto round64 = [](size_t n) { return (n + 63) & ~static_cast<size_t>(63); };
    size_t at = 0;
    auto take = [&at, &round64](size_t n) {
        const size_t here = at;
        at += round64(n);
        return here;
    };
    auto dense = [&](const NtTensor& t, uint32_t n, uint32_t k) {
        NthShadow s;
        s.src_at = t.at;
        s.n = n;
        s.k = k;
        s.w_at = take(static_cast<size_t>(n) * nth_pad32(k));
        s.wt_at = take(static_cast<size_t>(k) * nth_pad32(n));
        p.shadow.push_back(s);
    };
    dense(lay.fc1_w, d.mlp, d.n_features);
    for (uint32_t i = 0; i < d.layers; ++i) dense(lay.layer_w[i], d.mlp, d.mlp);
    dense(lay.out_w, NM_OUT, d.mlp);
    p.shadow_total = at;

    at = 0;
    const size_t B = max_batch;
    p.f_pad = nth_pad32(d.n_features);
    p.mlp_pad = nth_pad32(d.mlp);
    p.b_pad = nth_pad32(max_batch);
    p.h_stride = round64(B * p.mlp_pad);
    p.ht_stride = round64(static_cast<size_t>(d.mlp) * p.b_pad);
    p.feat_at = take(B * p.f_pad);
    p.featt_at = take(static_cast<size_t>(d.n_features) * p.b_pad);
    p.h_at = take((d.layers + 1) * p.h_stride);
    p.ht_at = take((d.layers + 1) * p.ht_stride);
    p.dz_at = take(B * NM_OUT);
    p.dzt_at = take(static_cast<size_t>(NM_OUT) * p.b_pad);
    p.da_at = take(2 * p.h_stride);
    p.dat_at = take(2 * p.ht_stride);
    p.ws_total = at;
    return p;
}

NoteTrainerTestPlan note_trainer_test_plan(size_t n_idx, uint32_t max_batch, uint32_t batch) {
    NoteTrainerTestPlan p;
    if (n_idx == 0 || max_batch == 0 || batch == 0) return p;
    for (size_t at = 0; at < n_idx; at += max_batch) {
        NtTestChunk c;
        c.begin = at;
        c.rows = static_cast<uint32_t>(std::min<size_t>(max_batch, n_idx - at));
        p.chunks.push_back(c);
    }
    p.n_batches = (n_idx + batch - 1) / batch;
    p.rows_bytes = n_idx * NT_TEST_ROW_BYTES;
    p.out_bytes = p.n_batches * sizeof(pvq_note_test_batch) + NT_TEST_PITCH_BYTES;
    return p;
}

pvq_status note_trainer_check_test(const NoteModelDims& d, const void* d_db, const void* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx,
                                   uint32_t batch, const void* out_batches, std::string& err) {
    if (!d_db || !d_targets || !idx) {
        err = "note trainer: d_db, d_targets or idx is null";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!out_batches) {
        err = "note trainer: out_batches is null";
        return PVQ_ERR_INVALID_ARG;
    }
    if (batch < 1) {
        err = "note trainer: the test batch must be at least 1";
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_idx < 1 || n_idx > NT_TEST_MAX_IDX) {
        err = "note trainer: n_idx must lie in 1 .. 2^25";
        return PVQ_ERR_INVALID_ARG;
    }
    return check_rows(d, n_rows, idx, n_idx, err);
}

pvq_status note_test_metrics(const pvq_note_test_batch* b, size_t n_batches, double* mean_f1, double* accuracy, double* mean_loss, std::string& err) {
    if (!b || n_batches < 1) {
        err = "note test metrics: the records are null or there is none";
        return PVQ_ERR_INVALID_ARG;
    }
    double f1 = 0.0, loss = 0.0;
    uint64_t correct = 0, rows = 0;
    for (size_t k = 0; k < n_batches; ++k) {
        const uint64_t den = 2 * static_cast<uint64_t>(b[k].tp) + b[k].fp + b[k].fn;
        if (den > 0) f1 += 2.0 * static_cast<double>(b[k].tp) / static_cast<double>(den);   // (else 0: sklearn's zero-division value)
        loss += b[k].loss;
        correct += b[k].correct;
        rows += b[k].rows;
    }
    if (rows == 0) {
        err = "note test metrics: the records hold no rows";
        return PVQ_ERR_INVALID_ARG;
    }
    if (mean_f1) *mean_f1 = f1 / static_cast<double>(n_batches);
    if (accuracy) *accuracy = static_cast<double>(correct) / (static_cast<double>(NM_OUT) * static_cast<double>(rows));
    if (mean_loss) *mean_loss = loss / static_cast<double>(n_batches);
    return PVQ_OK;
}

NoteTrainerEpochPlan note_trainer_epoch_plan(size_t n_idx, uint32_t batch) {
    NoteTrainerEpochPlan p;
    if (n_idx == 0 || batch == 0) return p;
    p.n_batches = (n_idx + batch - 1) / batch;
    p.last_rows = static_cast<uint32_t>(n_idx - (p.n_batches - 1) * batch);
    p.idx_at = 0;
    p.order_at = n_idx;
    p.loss_at = 2 * n_idx;
    p.device_bytes = (2 * n_idx + p.n_batches) * 4;
    p.h_idx_at = 0;
    p.h_loss_at = n_idx;
    p.host_bytes = (n_idx + p.n_batches) * 4;
    return p;
}

pvq_status note_trainer_check_epoch(const NoteModelDims& d, uint32_t max_batch, const void* d_db, const void* d_targets, size_t n_rows,
                                    const uint32_t* idx, size_t n_idx, uint32_t batch, std::string& err) {
    if (!d_db || !d_targets || !idx) {
        err = "note trainer: d_db, d_targets or idx is null";
        return PVQ_ERR_INVALID_ARG;
    }
    if (batch < 1 || batch > max_batch) {
        err = "note trainer: batch must lie in 1 .. max_batch (" + std::to_string(max_batch) + ")";
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_idx < 1 || n_idx > NT_EPOCH_MAX_IDX) {
        err = "note trainer: n_idx must lie in 1 .. 2^25";
        return PVQ_ERR_INVALID_ARG;
    }
    return check_rows(d, n_rows, idx, n_idx, err);
}

double note_epoch_mean_loss(const float* losses, size_t n_batches) {
    double s = 0.0;
    for (size_t k = 0; k < n_batches; ++k) s += static_cast<double>(losses[k]);
    return s / static_cast<double>(n_batches);
}

pvq_status note_epoch_order(uint64_t seed, uint64_t epoch, uint64_t n, uint64_t first, uint64_t count, uint32_t* out, std::string& err) {
    if (n < 1 || n > NE_MAX_N) {
        err = "note epoch order: n must lie in 1 .. 2^32";
        return PVQ_ERR_INVALID_ARG;
    }
    if (first > n || count > n - first) {
        err = "note epoch order: first + count exceeds n";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!out) {
        err = "note epoch order: out is null";
        return PVQ_ERR_INVALID_ARG;
    }
    const NoteEpochKeys k = ne_keys(seed, epoch, n);
    for (uint64_t j = 0; j < count; ++j) out[j] = static_cast<uint32_t>(ne_order(k, first + j));
    return PVQ_OK;
}

pvq_status note_trainer_check_write(int what, const void* host, size_t count, size_t n_params, std::string& err) {
    if (what < PVQ_TRAIN_WEIGHTS || what > PVQ_TRAIN_ADAM_V) {
        err = "note trainer: unknown array";
        return PVQ_ERR_INVALID_ARG;
    }
    if (!host) {
        err = "note trainer: the array to write is null";
        return PVQ_ERR_INVALID_ARG;
    }
    if (count != n_params) {
        err = "note trainer: count is " + std::to_string(count) + ", the handle holds " + std::to_string(n_params) + " parameters";
        return PVQ_ERR_INVALID_ARG;
    }
    return PVQ_OK;
}

pvq_status note_trainer_check_steps(uint64_t steps, std::string& err) {
    if (steps >= NT_MAX_STEPS) {
        err = "note trainer: steps must lie below 2^53";
        return PVQ_ERR_INVALID_ARG;
    }
    return PVQ_OK;
}

}  // namespace pvq
