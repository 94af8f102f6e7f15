// capi_analysis.cpp — extern "C" surface of libpvq (include/pvq.h): the analysis state of one stream on the host and of many on the device.
#include <cstring>
#include <vector>

#include "analysis_batch.hpp"
#include "analysis_host.hpp"
#include "capi_support.hpp"
#include "vqt_engine.hpp"

extern "C" {

void pvq_analysis_full_default_params(pvq_analysis_full_params* p) {
    guarded([&] {
        if (!p) return;
        const pvq::FullAnalysisParameters d;
        p->spectrogram_length = d.spectrogram_length;
        p->peak_min_prominence = d.peak_config.min_prominence;
        p->peak_min_height = d.peak_config.min_height;
        p->bass_min_prominence = d.bassline_peak_config.min_prominence;
        p->bass_min_height = d.bassline_peak_config.min_height;
        p->highest_bassnote = d.highest_bassnote;
        p->vqt_smoothing_duration_base_ns = d.vqt_smoothing_duration_base.ns;
        p->vqt_smoothing_calmness_min = d.vqt_smoothing_calmness_min;
        p->vqt_smoothing_calmness_max = d.vqt_smoothing_calmness_max;
        p->note_calmness_smoothing_duration_ns = d.note_calmness_smoothing_duration.ns;
        p->scene_calmness_smoothing_duration_ns = d.scene_calmness_smoothing_duration.ns;
        p->tuning_inaccuracy_smoothing_duration_ns = d.tuning_inaccuracy_smoothing_duration.ns;
        p->harmonic_threshold = d.harmonic_threshold;
    });
}

static pvq::FullAnalysisParameters full_to_cpp(const pvq_analysis_full_params* params) {
    pvq::FullAnalysisParameters q;
    if (params) {
        q.spectrogram_length = params->spectrogram_length;
        q.peak_config = {params->peak_min_prominence, params->peak_min_height};
        q.bassline_peak_config = {params->bass_min_prominence, params->bass_min_height};
        q.highest_bassnote = params->highest_bassnote;
        q.vqt_smoothing_duration_base = pvq::Duration{params->vqt_smoothing_duration_base_ns};
        q.vqt_smoothing_calmness_min = params->vqt_smoothing_calmness_min;
        q.vqt_smoothing_calmness_max = params->vqt_smoothing_calmness_max;
        q.note_calmness_smoothing_duration = pvq::Duration{params->note_calmness_smoothing_duration_ns};
        q.scene_calmness_smoothing_duration = pvq::Duration{params->scene_calmness_smoothing_duration_ns};
        q.tuning_inaccuracy_smoothing_duration = pvq::Duration{params->tuning_inaccuracy_smoothing_duration_ns};
        q.harmonic_threshold = params->harmonic_threshold;
    }
    return q;
}

static pvq::AnalysisBatchOutputs outputs_to_cpp(const pvq_analysis_batch_outputs* outs) {
    pvq::AnalysisBatchOutputs o;
    if (outs) {
        o.x_vqt_smoothed = outs->x_vqt_smoothed; o.x_vqt_peakfiltered = outs->x_vqt_peakfiltered; o.x_vqt_afterglow = outs->x_vqt_afterglow;
        o.calmness = outs->calmness; o.pitch_accuracy = outs->pitch_accuracy; o.pitch_deviation = outs->pitch_deviation;
        o.peak_mask = outs->peak_mask; o.peak_count = outs->peak_count; o.center = outs->center; o.size = outs->size;
        o.max_peaks = outs->max_peaks; o.scene_calmness = outs->scene_calmness; o.tuning_grid_inaccuracy = outs->tuning_grid_inaccuracy;
    }
    return o;
}

pvq_status pvq_analysis_state_create(float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                     const pvq_analysis_full_params* params, pvq_analysis_state** out) {
    return guarded([&] {
        if (!out) return null_handle();
        *out = nullptr;
        if (!(min_freq > 0.0f) || octaves == 0 || buckets_per_octave == 0) return invalid_arg("invalid VqtRange");
        const pvq::FullAnalysisParameters q = full_to_cpp(params);
        pvq::VqtRange r;
        r.min_freq = min_freq;
        r.octaves = octaves;
        r.buckets_per_octave = buckets_per_octave;
        *out = new pvq_analysis_state{std::unique_ptr<pvq::AnalysisState>(new pvq::AnalysisState(r, q))};
        return PVQ_OK;
    });
}

void pvq_analysis_state_destroy(pvq_analysis_state* s) { destroy(s); }

pvq_status pvq_analysis_state_update_vqt_smoothing_duration(pvq_analysis_state* s, int has_duration, uint64_t duration_ns) {
    return guarded([&] {
        if (!s) return null_handle();
        s->impl->update_vqt_smoothing_duration(has_duration != 0, pvq::Duration{duration_ns});
        return PVQ_OK;
    });
}

pvq_status pvq_analysis_state_preprocess(pvq_analysis_state* s, const float* x_vqt, size_t len, uint64_t frame_time_ns) {
    return guarded([&] {
        if (!s || !x_vqt) return null_handle();
        if (!s->impl->preprocess(x_vqt, len, pvq::Duration{frame_time_ns})) {
            pvq::set_last_error("x_vqt.len() == range.n_buckets()");
            return PVQ_ERR_BAD_LENGTH;
        }
        return PVQ_OK;
    });
}

float pvq_analysis_state_bin_to_frequency(const pvq_analysis_state* s, uint32_t bin) {
    return guarded(0.0f, [&] {
        return s ? s->impl->bin_to_frequency(bin) : 0.0f;
    });
}
uint32_t pvq_analysis_state_n_buckets(const pvq_analysis_state* s) {
    return guarded(0, [&] {
        return s ? s->impl->range.n_buckets() : 0;
    });
}

pvq_status pvq_analysis_state_get_field(const pvq_analysis_state* s, pvq_analysis_field f, float* out) {
    return guarded([&] {
        if (!s || !out) return null_handle();
        const pvq::AnalysisState& a = *s->impl;
        const uint32_t n = a.range.n_buckets();
        switch (f) {
            case PVQ_FIELD_X_VQT_SMOOTHED:
                for (uint32_t i = 0; i < n; ++i) out[i] = a.x_vqt_smoothed[i].get();
                return PVQ_OK;
            case PVQ_FIELD_X_VQT_PEAKFILTERED: std::memcpy(out, a.x_vqt_peakfiltered.data(), n * sizeof(float)); return PVQ_OK;
            case PVQ_FIELD_X_VQT_AFTERGLOW: std::memcpy(out, a.x_vqt_afterglow.data(), n * sizeof(float)); return PVQ_OK;
            case PVQ_FIELD_CALMNESS:
                for (uint32_t i = 0; i < n; ++i) out[i] = a.calmness[i].get();
                return PVQ_OK;
            case PVQ_FIELD_PITCH_ACCURACY: std::memcpy(out, a.pitch_accuracy.data(), n * sizeof(float)); return PVQ_OK;
            case PVQ_FIELD_PITCH_DEVIATION: std::memcpy(out, a.pitch_deviation.data(), n * sizeof(float)); return PVQ_OK;
        }
        pvq::set_last_error("unknown field");
        return PVQ_ERR_INVALID_ARG;
    });
}

uint32_t pvq_analysis_state_get_peaks(const pvq_analysis_state* s, uint32_t* out, uint32_t capacity) {
    return guarded(0, [&]() -> uint32_t {
        if (!s) return 0;
        const auto& p = s->impl->peaks;
        for (uint32_t i = 0; i < p.size() && i < capacity && out; ++i) out[i] = p[i];
        return static_cast<uint32_t>(p.size());
    });
}
uint32_t pvq_analysis_state_get_peaks_continuous(const pvq_analysis_state* s, float* center, float* size, uint32_t capacity) {
    return guarded(0, [&]() -> uint32_t {
        if (!s) return 0;
        const auto& p = s->impl->peaks_continuous;
        for (uint32_t i = 0; i < p.size() && i < capacity; ++i) {
            if (center) center[i] = p[i].center;
            if (size) size[i] = p[i].size;
        }
        return static_cast<uint32_t>(p.size());
    });
}
float pvq_analysis_state_scene_calmness(const pvq_analysis_state* s) {
    return guarded(0.0f, [&] {
        return s ? s->impl->smoothed_scene_calmness.get() : 0.0f;
    });
}
float pvq_analysis_state_tuning_grid_inaccuracy(const pvq_analysis_state* s) {
    return guarded(0.0f, [&] {
        return s ? s->impl->smoothed_tuning_grid_inaccuracy.get() : 0.0f;
    });
}

pvq_status pvq_analysis_batch_create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                     const pvq_analysis_full_params* params, uint32_t n_streams, pvq_analysis_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            pvq::VqtRange r;
            r.min_freq = min_freq;
            r.octaves = octaves;
            r.buckets_per_octave = buckets_per_octave;
            return pvq::AnalysisBatch::create(device_id, r, full_to_cpp(params), n_streams, impl);
        });
    });
}
void pvq_analysis_batch_destroy(pvq_analysis_batch* b) { destroy(b); }
pvq_status pvq_analysis_batch_update_vqt_smoothing_duration(pvq_analysis_batch* b, int has_duration, uint64_t duration_ns) {
    return guarded([&] {
        if (!b) return null_handle();
        b->impl->update_vqt_smoothing_duration(has_duration != 0, pvq::Duration{duration_ns});
        return PVQ_OK;
    });
}
pvq_status pvq_analysis_batch_preprocess_device(pvq_analysis_batch* b, const float* d_db, size_t n_frames, uint64_t frame_time_ns,
                                                const uint64_t* frame_times_ns, const pvq_analysis_batch_outputs* outs, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->preprocess_device(d_db, n_frames, pvq::Duration{frame_time_ns}, frame_times_ns, outputs_to_cpp(outs),
                                          static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_analysis_batch_preprocess_pcm(pvq_analysis_batch* b, pvq_vqt* v, const float* const* d_pcm, const size_t* n_lead, size_t n_frames,
                                             size_t hop, uint64_t frame_time_ns, float* d_db, const pvq_analysis_batch_outputs* outs, void* stream) {
    return guarded([&] {
        if (!b || !v) return null_handle();
        const pvq::VqtRange& r = v->impl->params().range;
        if (b->impl->device() != v->impl->device() || b->impl->n_bins() != v->impl->n_bins() || b->impl->range().min_freq != r.min_freq ||
            b->impl->range().buckets_per_octave != r.buckets_per_octave) {
            return invalid_arg("the transform handle and the analysis batch must sit on the same device and share the VqtRange");
        }
        if (n_frames == 0) return PVQ_OK;
        const uint32_t ns = b->impl->n_streams();
        float* db = d_db;
        if (!db) {
            pvq_status st = b->impl->frames_buffer((size_t)ns * n_frames * b->impl->n_bins() * sizeof(float), &db);
            if (st != PVQ_OK) return st;
        }
        std::vector<size_t> nf(ns, n_frames);
        pvq_status st = v->impl->batch_streams_device(d_pcm, n_lead, nf.data(), ns, hop, db, n_frames, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                                      static_cast<hipStream_t>(stream));
        if (st != PVQ_OK) return st;
        return b->impl->preprocess_device(db, n_frames, pvq::Duration{frame_time_ns}, nullptr, outputs_to_cpp(outs),
                                          static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_analysis_batch_get_field(pvq_analysis_batch* b, uint32_t stream_index, pvq_analysis_field f, float* out) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_field(stream_index, (int)f, out);
    });
}
pvq_status pvq_analysis_batch_get_scalars(pvq_analysis_batch* b, uint32_t stream_index, float* scene_calmness, float* tuning_grid_inaccuracy) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_scalars(stream_index, scene_calmness, tuning_grid_inaccuracy);
    });
}

}  // extern "C"
