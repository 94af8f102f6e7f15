// note_trainer_plan.cpp — see note_trainer_plan.hpp
#include "note_trainer_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

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
    if (n_rows > 0xffffffffull) {
        err = "note trainer: a dataset holds at most 2^32 - 1 rows";
        return PVQ_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < batch; ++i)
        if (idx[i] < d.t_frames - 1 || idx[i] >= n_rows) {
            err = "note trainer: idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [t_frames - 1, n_rows)";
            return PVQ_ERR_INVALID_ARG;
        }
    return PVQ_OK;
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

}  // namespace pvq
