// capi_notes.cpp — extern "C" surface of libpvq (include/pvq.h): note model, note trainer, test metrics.
#include <string>

#include "capi_support.hpp"
#include "note_carry.hpp"
#include "note_model.hpp"
#include "note_trainer.hpp"

extern "C" {

// pitchvis_train/train.py:67-99 as pitchvis_viewer/src/ml_system.rs:24-69 runs it: one row on the host, many rows on the device (note_model.hpp)
pvq_status pvq_note_model_create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights, pvq_note_model** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::NoteModel::create(device_id, params, weights, impl);
        });
    });
}
// the same model at any precision: its dense layers in f32 as above, or in bf16 or f16 (note_model_half.hpp)
pvq_status pvq_note_model_create_precision(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                                           pvq_note_precision precision, pvq_note_model** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            if (!pvq::note_precision_known(static_cast<int>(precision))) return invalid_arg("note model: precision is none of pvq_note_precision");
            return pvq::NoteModel::create(device_id, params, weights, precision, impl);
        });
    });
}
pvq_status pvq_note_model_precision(const pvq_note_model* m, pvq_note_precision* out) {
    return guarded([&] {
        if (!m || !out) return null_handle();
        *out = m->impl->precision();
        return PVQ_OK;
    });
}
pvq_status pvq_note_round(pvq_note_precision precision, const float* in, size_t n, float* out) {
    return guarded([&] {
        if (!pvq::note_precision_known(static_cast<int>(precision))) return invalid_arg("note round: precision is none of pvq_note_precision");
        if (n && (!in || !out)) return invalid_arg("note round: null input or output");
        for (size_t i = 0; i < n; ++i) out[i] = pvq::note_round(precision, in[i]);
        return PVQ_OK;
    });
}
void pvq_note_model_destroy(pvq_note_model* m) { destroy(m); }
pvq_status pvq_note_model_sizes(const pvq_note_model* m, uint32_t out4[4]) {
    return guarded([&] {
        if (!m || !out4) return null_handle();
        const pvq::NoteModelDims& d = m->impl->dims();
        out4[0] = d.L; out4[1] = d.o_conv; out4[2] = d.o_pool; out4[3] = d.n_features;
        return PVQ_OK;
    });
}
pvq_status pvq_note_model_infer(const pvq_note_model* m, const float* window_host, float out_prob[128]) {
    return guarded([&] {
        if (!m) return null_handle();
        if (!window_host || !out_prob) return invalid_arg("note model: null window or output");
        m->impl->infer(window_host, out_prob);   // ml_system.rs:24-69
        return PVQ_OK;
    });
}
pvq_status pvq_note_model_rows_device(pvq_note_model* m, const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                                      const pvq_note_model_outputs* outs, void* stream) {
    return guarded([&] {
        if (!m) return null_handle();
        const pvq_note_model_outputs none{};
        return m->impl->rows_device(d_db, n_frames, n_streams, stride_frames, outs ? *outs : none, static_cast<hipStream_t>(stream));
    });
}
// windows that continue across calls, rows of many streams in one tile (note_carry.hpp); ml_system.rs:50-69 feeds a frame per call
pvq_status pvq_note_carry_create(const pvq_note_model* m, uint32_t n_streams, pvq_note_carry** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            if (!m) return null_handle();
            return pvq::NoteCarry::create(m->impl->dims(), m->impl->device(), n_streams, impl);
        });
    });
}
void pvq_note_carry_destroy(pvq_note_carry* c) { destroy(c); }
pvq_status pvq_note_carry_reset(pvq_note_carry* c, int64_t stream_index, void* stream) {
    return guarded([&] {
        if (!c) return null_handle();
        return c->impl->reset(stream_index, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_note_carry_frames_seen(const pvq_note_carry* c, uint32_t stream_index, uint64_t* out) {
    return guarded([&] {
        if (!c) return null_handle();
        return c->impl->frames_seen(stream_index, out);
    });
}
pvq_status pvq_note_model_rows_carry_device(pvq_note_model* m, pvq_note_carry* c, const float* d_db, const size_t* n_frames, uint32_t n_streams,
                                            size_t stride_frames, const pvq_note_model_outputs* outs, void* stream) {
    return guarded([&] {
        if (!m || !c) return null_handle();
        const pvq_note_model_outputs none{};
        return m->impl->rows_carry_device(*c->impl, d_db, n_frames, n_streams, stride_frames, outs ? *outs : none, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_note_model_set_workspace_limit(pvq_note_model* m, uint64_t bytes) {
    return guarded([&] {
        if (!m) return null_handle();
        m->impl->set_workspace_limit(bytes);
        return PVQ_OK;
    });
}

// pitchvis_train/train.py:108-162, the optimisation step, on the device (note_trainer.hpp)
void pvq_note_trainer_hyper_default(pvq_note_trainer_hyper* h) {
    guarded([&] {
        if (!h) return;
        h->lr = 1e-5;                  // train.py:111
        h->beta1 = 0.9;                // torch.optim.Adam's defaults
        h->beta2 = 0.999;
        h->eps = 1.1920928955078125e-7;   // train.py:143 torch.finfo(torch.float32).eps
        h->weight_decay = 5e-4;        // train.py:144
        h->dropout = 0.1;              // train.py:131-138
        h->seed = 0;
    });
}
pvq_status pvq_note_trainer_create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                                   const pvq_note_trainer_hyper* hyper, uint32_t max_batch, pvq_note_trainer** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::NoteTrainer::create(device_id, params, weights, hyper, max_batch, impl);
        });
    });
}
// the same with the dense products in bf16 under the rule of include/pvq.h (note_trainer_half.hpp); PVQ_NOTE_F32 is the entry above
pvq_status pvq_note_trainer_create_precision(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                                             const pvq_note_trainer_hyper* hyper, uint32_t max_batch, pvq_note_precision precision,
                                             pvq_note_trainer** out) {
    if (precision == PVQ_NOTE_F32) return pvq_note_trainer_create(device_id, params, weights, hyper, max_batch, out);
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::NoteTrainer::create(device_id, params, weights, hyper, max_batch, precision, impl);
        });
    });
}
int pvq_note_trainer_precision(const pvq_note_trainer* t) {
    return guarded(0, [&] { return t ? static_cast<int>(t->impl->precision()) : 0; });
}
void pvq_note_trainer_destroy(pvq_note_trainer* t) { destroy(t); }
pvq_status pvq_note_trainer_step(pvq_note_trainer* t, int mode, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx,
                                 uint32_t batch, float* d_loss, float* d_logits, void* stream) {
    return guarded([&] {
        if (!t) return null_handle();
        return t->impl->step(mode, d_db, d_targets, n_rows, idx, batch, d_loss, d_logits, static_cast<hipStream_t>(stream));
    });
}
uint64_t pvq_note_trainer_steps(const pvq_note_trainer* t) { return guarded(0, [&] { return t ? t->impl->steps() : 0; }); }
uint64_t pvq_note_trainer_param_count(const pvq_note_trainer* t) { return guarded(0, [&] { return t ? t->impl->n_params() : 0; }); }
pvq_status pvq_note_trainer_read(pvq_note_trainer* t, int what, float* out_host, size_t capacity) {
    return guarded([&] {
        if (!t) return null_handle();
        return t->impl->read(what, out_host, capacity);
    });
}
// the inverse of pvq_note_trainer_read, and the counter: a checkpoint restored
pvq_status pvq_note_trainer_write(pvq_note_trainer* t, int what, const float* host, size_t count) {
    return guarded([&] {
        if (!t) return null_handle();
        return t->impl->write(what, host, count);
    });
}
pvq_status pvq_note_trainer_set_steps(pvq_note_trainer* t, uint64_t steps) {
    return guarded([&] {
        if (!t) return null_handle();
        return t->impl->set_steps(steps);
    });
}
// train.py:147-162, one epoch; its order on the host
pvq_status pvq_note_trainer_epoch(pvq_note_trainer* t, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx,
                                  uint32_t batch, uint64_t shuffle_seed, uint64_t epoch, float* out_losses, double* out_mean_loss, void* stream) {
    return guarded([&] {
        if (!t) return null_handle();
        return t->impl->epoch(d_db, d_targets, n_rows, idx, n_idx, batch, shuffle_seed, epoch, out_losses, out_mean_loss, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_note_epoch_order(uint64_t seed, uint64_t epoch, uint64_t n, uint64_t first, uint64_t count, uint32_t* out) {
    return guarded([&] {
        std::string err;
        const pvq_status st = pvq::note_epoch_order(seed, epoch, n, first, count, out, err);
        if (st != PVQ_OK) pvq::set_last_error(err);
        return st;
    });
}
// train.py:164-198, the test pass
pvq_status pvq_note_trainer_test(pvq_note_trainer* t, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx,
                                 uint32_t batch, pvq_note_test_batch* out_batches, uint32_t* out_pitch, float* d_logits, void* stream) {
    return guarded([&] {
        if (!t) return null_handle();
        return t->impl->test(d_db, d_targets, n_rows, idx, n_idx, batch, out_batches, out_pitch, d_logits, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_note_test_metrics(const pvq_note_test_batch* b, size_t n_batches, double* mean_f1, double* accuracy, double* mean_loss) {
    return guarded([&] {
        std::string err;
        const pvq_status st = pvq::note_test_metrics(b, n_batches, mean_f1, accuracy, mean_loss, err);
        if (st != PVQ_OK) pvq::set_last_error(err);
        return st;
    });
}
pvq_status pvq_note_trainer_dropout_keep(uint64_t seed, uint64_t step, uint32_t layer, uint32_t row, uint32_t col0, uint32_t n, double dropout,
                                         uint8_t* out_keep) {
    return guarded([&] {
        if (!out_keep || !(dropout >= 0.0 && dropout < 1.0)) return invalid_arg("note trainer: out_keep is null or dropout lies outside [0, 1)");
        const uint64_t key = pvq::nt_layer_key(seed, step, layer);
        const uint32_t threshold = pvq::nt_keep_threshold(dropout);
        for (uint32_t j = 0; j < n; ++j) out_keep[j] = pvq::nt_keep(key, row, col0 + j, threshold) ? 1 : 0;
        return PVQ_OK;
    });
}

}  // extern "C"
