// capi.cpp — extern "C" surface of libpvq (include/pvq.h) over pvq::Vqt.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/pvq.h"
#include <cmath>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "analysis_batch.hpp"
#include "analysis_host.hpp"
#include "backdrop_batch.hpp"
#include "backdrop_host.hpp"
#include "condition_batch.hpp"
#include "consumers_host.hpp"
#include "multi_host.hpp"
#include "note_model.hpp"
#include "note_trainer.hpp"
#include "overlay_batch.hpp"
#include "overlay_host.hpp"
#include "panels_batch.hpp"
#include "panels_host.hpp"
#include "present_batch.hpp"
#include "present_host.hpp"
#include "raster_batch.hpp"
#include "raster_host.hpp"
#include "render_batch.hpp"
#include "scene_batch.hpp"
#include "scene_host.hpp"
#include "stage_plan.hpp"
#include "synth_batch.hpp"
#include "synth_host.hpp"
#include "text_batch.hpp"
#include "text_host.hpp"
#include "vqt_engine.hpp"

struct pvq_vqt {
    std::unique_ptr<pvq::Vqt> impl;
};
struct pvq_analysis_state {
    std::unique_ptr<pvq::AnalysisState> impl;
};
struct pvq_analysis_batch {
    std::unique_ptr<pvq::AnalysisBatch> impl;
};
struct pvq_mono_agc {
    pvq::MonoAgc impl;
};
struct pvq_agc_batch {
    std::unique_ptr<pvq::AgcBatch> impl;
};
struct pvq_render_batch {
    std::unique_ptr<pvq::RenderBatch> impl;
};
struct pvq_scene_state {
    std::unique_ptr<pvq::SceneState> impl;
};
struct pvq_scene_batch {
    std::unique_ptr<pvq::SceneBatch> impl;
};
struct pvq_raster_batch {
    std::unique_ptr<pvq::RasterBatch> impl;
};
struct pvq_backdrop_batch {
    std::unique_ptr<pvq::BackdropBatch> impl;
};
struct pvq_overlay_state {
    pvq::OverlayState impl;
};
struct pvq_overlay_batch {
    std::unique_ptr<pvq::OverlayBatch> impl;
};
struct pvq_text_font {
    std::unique_ptr<pvq::TextFont> impl;
};
struct pvq_text_batch {
    std::unique_ptr<pvq::TextBatch> impl;
};
struct pvq_synth_bank {
    std::shared_ptr<const pvq::SynthBank> impl;
};
struct pvq_synth_state {
    std::unique_ptr<pvq::SynthState> impl;
};
struct pvq_synth_batch {
    std::unique_ptr<pvq::SynthBatch> impl;
};
struct pvq_present_batch {
    std::unique_ptr<pvq::PresentBatch> impl;
};
struct pvq_calmness_graph {
    pvq::CalmnessGraph impl;
};
struct pvq_panels_batch {
    std::unique_ptr<pvq::PanelsBatch> impl;
};
struct pvq_note_model {
    std::unique_ptr<pvq::NoteModel> impl;
};
struct pvq_note_trainer {
    std::unique_ptr<pvq::NoteTrainer> impl;
};
// device-resident ring: the newest buf_size samples are d_ring[w - buf_size, w); compacted when the linear
// buffer (4 x buf_size) runs out
struct pvq_stream {
    ~pvq_stream() {   // also runs when pvq_stream_create fails half way: no device buffer is leaked
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (d_ring) (void)hipFree(d_ring);
        if (d_db) (void)hipFree(d_db);
        if (h_in) (void)hipHostFree(h_in);
        if (h_out) (void)hipHostFree(h_out);
    }
    pvq_vqt* vqt = nullptr;
    size_t buf_size = 0, cap = 0, w = 0;
    float* d_ring = nullptr;
    float* d_db = nullptr;
    bool with_agc = false;
    pvq::MonoAgc agc{0.07f, 0.0001f};   // audio_desktop.rs:93
    float gain = 0.0f;                  // audio_desktop.rs:83
    float chunk_size_ms = 0.0f;
    // page-locked staging and a stream of the object's own: a push is one asynchronous DMA behind the conditioning on the host, a frame
    // the kernels + one asynchronous copy back + ONE wait (pageable buffers cost a staged, synchronous copy each way)
    hipStream_t stream = nullptr;
    float* h_in = nullptr;    // [buf_size]: the chunk being appended
    float* h_out = nullptr;   // [n_bins]
    bool in_flight = false;   // h_in is being read by a copy queued on `stream`
};

namespace {
pvq::VqtParameters to_cpp(const pvq_vqt_params& p) {
    pvq::VqtParameters q;
    q.sr = p.sr;
    q.n_fft = p.n_fft;
    q.range.min_freq = p.min_freq;
    q.range.octaves = p.octaves;
    q.range.buckets_per_octave = p.buckets_per_octave;
    q.sparsity_quantile = p.sparsity_quantile;
    q.quality = p.quality;
    q.gamma = p.gamma;
    return q;
}
pvq::AnalysisParameters to_cpp(const pvq_analysis_params* a) {
    pvq::AnalysisParameters q;
    if (a) {
        q.peak_min_prominence = a->peak_min_prominence;
        q.peak_min_height = a->peak_min_height;
        q.bass_min_prominence = a->bass_min_prominence;
        q.bass_min_height = a->bass_min_height;
        q.highest_bassnote = a->highest_bassnote;
        q.harmonic_threshold = a->harmonic_threshold;
    }
    return q;
}
pvq_status null_handle() {
    pvq::set_last_error("null handle");
    return PVQ_ERR_INVALID_ARG;
}
// include/pvq.h: "no exceptions cross the ABI".  Every extern "C" body below runs inside try { } catch (...) and lands here:
// a PanicError (the reference's assert! / expect texts, vqt.rs:785-792) becomes PVQ_ERR_INVALID_ARG, anything else
// (std::bad_alloc from a table or staging vector, std::length_error, ...) PVQ_ERR_INTERNAL; the text goes to pvq_last_error.
pvq_status translate_exception() noexcept {
    try {
        throw;
    } catch (const pvq::PanicError& e) {
        pvq::set_last_error_noexcept(e.what());
        return PVQ_ERR_INVALID_ARG;
    } catch (const std::bad_alloc&) {
        pvq::set_last_error_noexcept("out of host memory");
        return PVQ_ERR_INTERNAL;
    } catch (const std::exception& e) {
        pvq::set_last_error_noexcept(e.what());
        return PVQ_ERR_INTERNAL;
    } catch (...) {
        pvq::set_last_error_noexcept("unknown exception");
        return PVQ_ERR_INTERNAL;
    }
}
}  // namespace

extern "C" {

const char* pvq_status_string(pvq_status s) {
    try {
        switch (s) {
            case PVQ_OK: return "ok";
            case PVQ_ERR_ABOVE_NYQUIST: return "AboveNyquist";
            case PVQ_ERR_WINDOW_EXCEEDS_NFFT: return "WindowExceedsNFft";
            case PVQ_ERR_BAD_LENGTH: return "input must be exactly n_fft samples";
            case PVQ_ERR_INVALID_ARG: return "invalid argument";
            case PVQ_ERR_NO_DEVICE: return "handle has no GPU context (no CPU fallback)";
            case PVQ_ERR_DEVICE: return "HIP error";
            case PVQ_ERR_UNSUPPORTED: return "unsupported geometry";
            case PVQ_ERR_INTERNAL: return "internal error (out of memory or an unexpected exception)";
            case PVQ_ERR_NONFINITE_INPUT: return "non-finite sample in the input";
        }
        return "unknown";
    } catch (...) { (void)translate_exception(); return nullptr; }
}

const char* pvq_last_error(void) {
    try {
        return pvq::get_last_error();
    } catch (...) { (void)translate_exception(); return nullptr; }
}
uint32_t pvq_abi_version(void) {
    try {
        return PVQ_ABI_VERSION;
    } catch (...) { (void)translate_exception(); return 0; }
}

void pvq_vqt_default_params(pvq_vqt_params* p) {
    try {
        if (!p) return;
        const pvq::VqtParameters d;
        p->sr = d.sr;
        p->n_fft = d.n_fft;
        p->min_freq = d.range.min_freq;
        p->octaves = d.range.octaves;
        p->buckets_per_octave = d.range.buckets_per_octave;
        p->sparsity_quantile = d.sparsity_quantile;
        p->quality = d.quality;
        p->gamma = d.gamma;
    } catch (...) { (void)translate_exception(); }
}

pvq_status pvq_vqt_create(const pvq_vqt_params* params, int device_id, pvq_vqt** out, float err_detail[2]) {
    try {
        if (!params || !out) return null_handle();
        *out = nullptr;
        if (const char* t = pvq::dev_knob_str("PVQ_TEST_THROW")) {   // developer build only: test hook for the exception barrier (tests/test_capi_hardening.py)
            if (!std::strcmp(t, "bad_alloc")) throw std::bad_alloc();
            if (!std::strcmp(t, "length_error")) throw std::length_error("vector::_M_default_append");
            if (!std::strcmp(t, "int")) throw 42;
        }
        pvq::VqtError err;
        std::unique_ptr<pvq::Vqt> impl;
        const pvq_status st = pvq::Vqt::create(to_cpp(*params), device_id, impl, err);
        if (err_detail) {
            err_detail[0] = err.a;
            err_detail[1] = err.b;
        }
        if (st != PVQ_OK) return st;
        *out = new pvq_vqt{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

void pvq_vqt_destroy(pvq_vqt* v) {
    try {
        delete v;
    } catch (...) { (void)translate_exception(); }
}

void pvq_vqt_get_params(const pvq_vqt* v, pvq_vqt_params* out) {
    try {
        if (!v || !out) return;
        const pvq::VqtParameters& d = v->impl->params();
        out->sr = d.sr;
        out->n_fft = d.n_fft;
        out->min_freq = d.range.min_freq;
        out->octaves = d.range.octaves;
        out->buckets_per_octave = d.range.buckets_per_octave;
        out->sparsity_quantile = d.sparsity_quantile;
        out->quality = d.quality;
        out->gamma = d.gamma;
    } catch (...) { (void)translate_exception(); }
}

uint32_t pvq_vqt_n_bins(const pvq_vqt* v) {
    try {
        return v ? v->impl->n_bins() : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}
double pvq_vqt_delay_seconds(const pvq_vqt* v) {
    try {
        return v ? v->impl->delay_seconds() : 0.0;
    } catch (...) { (void)translate_exception(); return 0.0; }
}
uint32_t pvq_vqt_window_union(const pvq_vqt* v) {
    try {
        return v ? v->impl->plan().window_union : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}
pvq_status pvq_vqt_bandwidths_3db(const pvq_vqt* v, float* lo_hz, float* hi_hz) {
    try {
        if (!v || !lo_hz || !hi_hz) return null_handle();
        const pvq::HostPlan& pl = v->impl->plan();
        std::copy(pl.bandwidth_lo_hz.begin(), pl.bandwidth_lo_hz.end(), lo_hz);
        std::copy(pl.bandwidth_hi_hz.begin(), pl.bandwidth_hi_hz.end(), hi_hz);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
uint32_t pvq_vqt_warning_count(const pvq_vqt* v) {
    try {
        return v ? (uint32_t)v->impl->plan().warnings.size() : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}
pvq_status pvq_vqt_warning(const pvq_vqt* v, uint32_t i, char* buf, size_t cap) {
    try {
        if (!v || !buf || cap == 0) return null_handle();
        const pvq::HostPlan& pl = v->impl->plan();
        if (i >= pl.warnings.size()) {
            pvq::set_last_error("warning index out of range");
            return PVQ_ERR_INVALID_ARG;
        }
        const std::string& w = pl.warnings[i];
        const size_t nb = std::min(cap - 1, w.size());
        std::memcpy(buf, w.data(), nb);
        buf[nb] = '\0';
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
uint32_t pvq_vqt_n_groups(const pvq_vqt* v) {
    try {
        return v ? static_cast<uint32_t>(v->impl->kernel().window_groups.size()) : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}

pvq_status pvq_vqt_group_info(const pvq_vqt* v, uint32_t g, uint32_t info[5]) {
    try {
        if (!v || !info) return null_handle();
        const auto& groups = v->impl->kernel().window_groups;
        if (g >= groups.size()) {
            pvq::set_last_error("group index out of range");
            return PVQ_ERR_INVALID_ARG;
        }
        info[0] = groups[g].window_begin;
        info[1] = groups[g].window_end;
        info[2] = groups[g].filter_bank.rows;
        info[3] = groups[g].filter_bank.nnz();
        info[4] = groups[g].negative_filter_bank.nnz();
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_group_csr(const pvq_vqt* v, uint32_t g, int negative, uint32_t* row_ptr, uint32_t* col_idx,
                             float* values) {
    try {
        if (!v || !row_ptr || !col_idx || !values) return null_handle();
        const auto& groups = v->impl->kernel().window_groups;
        if (g >= groups.size()) {
            pvq::set_last_error("group index out of range");
            return PVQ_ERR_INVALID_ARG;
        }
        const pvq::CsrMatrix& m = negative ? groups[g].negative_filter_bank : groups[g].filter_bank;
        std::memcpy(row_ptr, m.row_ptr.data(), sizeof(uint32_t) * m.row_ptr.size());
        std::memcpy(col_idx, m.col_idx.data(), sizeof(uint32_t) * m.col_idx.size());
        std::memcpy(values, m.values.data(), sizeof(pvq::cf32) * m.values.size());
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_filter_params(const pvq_vqt* v, float* freq, float* window_length, uint32_t* factor,
                                 uint32_t* minwin) {
    try {
        if (!v) return null_handle();
        const auto& f = v->impl->plan().filters;
        for (size_t k = 0; k < f.size(); ++k) {
            if (freq) freq[k] = f[k].freq;
            if (window_length) window_length[k] = f[k].window_length;
            if (factor) factor[k] = f[k].sr_downscaling_factor;
            if (minwin) minwin[k] = f[k].minimum_needed_window_size;
        }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_calculate_instant_db(pvq_vqt* v, const float* x, size_t len, float* out_db) {
    try {
        if (!v) return null_handle();
        if (!x || !out_db) {
            pvq::set_last_error("null pointer");
            return PVQ_ERR_INVALID_ARG;
        }
        return v->impl->calculate_vqt_instant_in_db(x, len, out_db);
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_calculate_batch_db(pvq_vqt* v, const float* pcm, size_t n_lead, size_t hop, size_t n_frames,
                                      float* out_db) {
    try {
        if (!v) return null_handle();
        return v->impl->calculate_batch_db(pcm, n_lead, hop, n_frames, out_db);
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_calculate_batch_db_device(pvq_vqt* v, const float* d_pcm, size_t n_lead, size_t hop,
                                             size_t n_frames, float* d_out_db, float* d_out_cplx, void* stream) {
    try {
        if (!v) return null_handle();
        return v->impl->calculate_batch_db_device(d_pcm, n_lead, hop, n_frames, d_out_db, d_out_cplx,
                                                  static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_set_algo(pvq_vqt* v, pvq_algo algo) {
    try {
        if (!v) return null_handle();
        if (algo != PVQ_ALGO_AUTO && algo != PVQ_ALGO_FFT && algo != PVQ_ALGO_BLOCKDFT) {
            pvq::set_last_error("unknown algorithm");
            return PVQ_ERR_INVALID_ARG;
        }
        v->impl->set_algo(algo);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_algo pvq_vqt_last_algo(const pvq_vqt* v) {
    try {
        return v ? v->impl->last_algo() : PVQ_ALGO_AUTO;
    } catch (...) { (void)translate_exception(); return PVQ_ALGO_AUTO; }
}
pvq_algo pvq_vqt_resolve_algo(pvq_vqt* v, size_t hop, size_t n_frames) {
    try {
        if (!v || hop == 0) return PVQ_ALGO_AUTO;
        return v->impl->resolve_algo(hop, n_frames);
    } catch (...) { (void)translate_exception(); return PVQ_ALGO_AUTO; }
}

pvq_status pvq_vqt_set_twiddle_fp16(pvq_vqt* v, int enable) {
    try {
        if (!v) return null_handle();
        return v->impl->set_twiddle_fp16(enable != 0);
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_set_workspace_limit(pvq_vqt* v, uint64_t bytes) {
    try {
        if (!v) return null_handle();
        v->impl->set_workspace_limit((size_t)bytes);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

uint32_t pvq_vqt_blockdft_columns(const pvq_vqt* v) {
    try {
        return v ? v->impl->blockdft_columns() : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}

pvq_status pvq_vqt_set_gemm_precision(pvq_vqt* v, pvq_gemm_precision p) {
    try {
        if (!v) return null_handle();
        if (p != PVQ_GEMM_F32 && p != PVQ_GEMM_BF16X3) {
            pvq::set_last_error("unknown GEMM precision");
            return PVQ_ERR_INVALID_ARG;
        }
        v->impl->set_gemm_split_bf16(p == PVQ_GEMM_BF16X3);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

void pvq_analysis_default_params(pvq_analysis_params* a) {
    try {
        if (!a) return;
        const pvq::AnalysisParameters d;
        a->peak_min_prominence = d.peak_min_prominence;
        a->peak_min_height = d.peak_min_height;
        a->bass_min_prominence = d.bass_min_prominence;
        a->bass_min_height = d.bass_min_height;
        a->highest_bassnote = d.highest_bassnote;
        a->harmonic_threshold = d.harmonic_threshold;
    } catch (...) { (void)translate_exception(); }
}

pvq_status pvq_analyze_batch_device(pvq_vqt* v, const float* d_db, size_t n_frames, const pvq_analysis_params* a,
                                    uint32_t* d_peak_mask, uint32_t* d_peak_count, float* d_center, float* d_size,
                                    uint32_t max_peaks, void* stream) {
    try {
        if (!v) return null_handle();
        return v->impl->analyze_batch_device(d_db, n_frames, to_cpp(a), d_peak_mask, d_peak_count, d_center, d_size,
                                             max_peaks, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_analyze_batch(pvq_vqt* v, const float* db, size_t n_frames, const pvq_analysis_params* a,
                             uint32_t* peak_mask, uint32_t* peak_count, float* center, float* size,
                             uint32_t max_peaks) {
    try {
        if (!v) return null_handle();
        return v->impl->analyze_batch(db, n_frames, to_cpp(a), peak_mask, peak_count, center, size, max_peaks);
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_analyze_batch_device(pvq_vqt* v, const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames,
                                        const pvq_analysis_params* a, float* d_out_db, uint32_t* d_peak_mask,
                                        uint32_t* d_peak_count, float* d_center, float* d_size, uint32_t max_peaks,
                                        void* stream) {
    try {
        if (!v) return null_handle();
        return v->impl->vqt_analyze_batch_device(d_pcm, n_lead, hop, n_frames, to_cpp(a), d_out_db, d_peak_mask,
                                                 d_peak_count, d_center, d_size, max_peaks,
                                                 static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_calculate_batch_db_streams(pvq_vqt* v, const float* const* d_pcm, const size_t* n_lead, const size_t* n_frames,
                                              uint32_t n_streams, size_t hop, float* d_out_db, size_t out_stride_frames, void* stream) {
    try {
        if (!v) return null_handle();
        return v->impl->batch_streams_device(d_pcm, n_lead, n_frames, n_streams, hop, d_out_db, out_stride_frames, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, 0, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_analyze_batch_streams(pvq_vqt* v, const float* const* d_pcm, const size_t* n_lead, const size_t* n_frames,
                                         uint32_t n_streams, size_t hop, const pvq_analysis_params* a, float* d_out_db,
                                         size_t out_stride_frames, uint32_t* d_peak_mask, uint32_t* d_peak_count, float* d_center,
                                         float* d_size, uint32_t max_peaks, void* stream) {
    try {
        if (!v) return null_handle();
        const pvq::AnalysisParameters ap = to_cpp(a);
        return v->impl->batch_streams_device(d_pcm, n_lead, n_frames, n_streams, hop, d_out_db, out_stride_frames, &ap, d_peak_mask,
                                             d_peak_count, d_center, d_size, max_peaks, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_plan_shard(uint64_t n_frames_total, uint64_t hop, uint64_t window_union, uint32_t rank, uint32_t world, pvq_shard* out) {
    try {
        pvq::ShardPlan sp;
        if (!out || !pvq::plan_shard(n_frames_total, hop, window_union, rank, world, &sp)) {
            pvq::set_last_error("pvq_plan_shard: null output or rank >= world");
            return PVQ_ERR_INVALID_ARG;
        }
        out->first_frame = sp.first_frame;
        out->n_frames = sp.n_frames;
        out->sample_begin = sp.sample_begin;
        out->sample_end = sp.sample_end;
        out->n_lead = sp.n_lead;
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_analyze_batch_multi(pvq_vqt* const* handles, uint32_t n_handles, const float* pcm, size_t n_lead, size_t hop,
                                       size_t n_frames, const pvq_analysis_params* a, float* out_db, uint32_t* peak_mask,
                                       uint32_t* peak_count, float* center, float* size, uint32_t max_peaks) {
    try {
        if (!handles || n_handles == 0) return null_handle();
        std::vector<pvq::Vqt*> hs(n_handles, nullptr);
        for (uint32_t i = 0; i < n_handles; ++i) {
            if (!handles[i]) return null_handle();
            hs[i] = handles[i]->impl.get();
        }
        return pvq::analyze_batch_multi(hs.data(), n_handles, pcm, n_lead, hop, n_frames, to_cpp(a), out_db, peak_mask, peak_count,
                                        center, size, max_peaks);
    } catch (...) { return translate_exception(); }
}

void pvq_analysis_full_default_params(pvq_analysis_full_params* p) {
    try {
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
    } catch (...) { (void)translate_exception(); }
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

pvq_status pvq_analysis_state_create(float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                     const pvq_analysis_full_params* params, pvq_analysis_state** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        if (!(min_freq > 0.0f) || octaves == 0 || buckets_per_octave == 0) {
            pvq::set_last_error("invalid VqtRange");
            return PVQ_ERR_INVALID_ARG;
        }
        const pvq::FullAnalysisParameters q = full_to_cpp(params);
        pvq::VqtRange r;
        r.min_freq = min_freq;
        r.octaves = octaves;
        r.buckets_per_octave = buckets_per_octave;
        *out = new pvq_analysis_state{std::unique_ptr<pvq::AnalysisState>(new pvq::AnalysisState(r, q))};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

void pvq_analysis_state_destroy(pvq_analysis_state* s) {
    try {
        delete s;
    } catch (...) { (void)translate_exception(); }
}

pvq_status pvq_analysis_state_update_vqt_smoothing_duration(pvq_analysis_state* s, int has_duration, uint64_t duration_ns) {
    try {
        if (!s) return null_handle();
        s->impl->update_vqt_smoothing_duration(has_duration != 0, pvq::Duration{duration_ns});
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_analysis_state_preprocess(pvq_analysis_state* s, const float* x_vqt, size_t len, uint64_t frame_time_ns) {
    try {
        if (!s || !x_vqt) return null_handle();
        if (!s->impl->preprocess(x_vqt, len, pvq::Duration{frame_time_ns})) {
            pvq::set_last_error("x_vqt.len() == range.n_buckets()");
            return PVQ_ERR_BAD_LENGTH;
        }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

float pvq_analysis_state_bin_to_frequency(const pvq_analysis_state* s, uint32_t bin) {
    try {
        return s ? s->impl->bin_to_frequency(bin) : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}
uint32_t pvq_analysis_state_n_buckets(const pvq_analysis_state* s) {
    try {
        return s ? s->impl->range.n_buckets() : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}

pvq_status pvq_analysis_state_get_field(const pvq_analysis_state* s, pvq_analysis_field f, float* out) {
    try {
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
    } catch (...) { return translate_exception(); }
}

uint32_t pvq_analysis_state_get_peaks(const pvq_analysis_state* s, uint32_t* out, uint32_t capacity) {
    try {
        if (!s) return 0;
        const auto& p = s->impl->peaks;
        for (uint32_t i = 0; i < p.size() && i < capacity && out; ++i) out[i] = p[i];
        return static_cast<uint32_t>(p.size());
    } catch (...) { (void)translate_exception(); return 0; }
}
uint32_t pvq_analysis_state_get_peaks_continuous(const pvq_analysis_state* s, float* center, float* size, uint32_t capacity) {
    try {
        if (!s) return 0;
        const auto& p = s->impl->peaks_continuous;
        for (uint32_t i = 0; i < p.size() && i < capacity; ++i) {
            if (center) center[i] = p[i].center;
            if (size) size[i] = p[i].size;
        }
        return static_cast<uint32_t>(p.size());
    } catch (...) { (void)translate_exception(); return 0; }
}
float pvq_analysis_state_scene_calmness(const pvq_analysis_state* s) {
    try {
        return s ? s->impl->smoothed_scene_calmness.get() : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}
float pvq_analysis_state_tuning_grid_inaccuracy(const pvq_analysis_state* s) {
    try {
        return s ? s->impl->smoothed_tuning_grid_inaccuracy.get() : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}

pvq_status pvq_analysis_batch_create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                     const pvq_analysis_full_params* params, uint32_t n_streams, pvq_analysis_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        pvq::VqtRange r;
        r.min_freq = min_freq;
        r.octaves = octaves;
        r.buckets_per_octave = buckets_per_octave;
        std::unique_ptr<pvq::AnalysisBatch> impl;
        const pvq_status st = pvq::AnalysisBatch::create(device_id, r, full_to_cpp(params), n_streams, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_analysis_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_analysis_batch_destroy(pvq_analysis_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_analysis_batch_update_vqt_smoothing_duration(pvq_analysis_batch* b, int has_duration, uint64_t duration_ns) {
    try {
        if (!b) return null_handle();
        b->impl->update_vqt_smoothing_duration(has_duration != 0, pvq::Duration{duration_ns});
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_analysis_batch_preprocess_device(pvq_analysis_batch* b, const float* d_db, size_t n_frames, uint64_t frame_time_ns,
                                                const uint64_t* frame_times_ns, const pvq_analysis_batch_outputs* outs, void* stream) {
    try {
        if (!b) return null_handle();
        pvq::AnalysisBatchOutputs o;
        if (outs) {
            o.x_vqt_smoothed = outs->x_vqt_smoothed; o.x_vqt_peakfiltered = outs->x_vqt_peakfiltered; o.x_vqt_afterglow = outs->x_vqt_afterglow;
            o.calmness = outs->calmness; o.pitch_accuracy = outs->pitch_accuracy; o.pitch_deviation = outs->pitch_deviation;
            o.peak_mask = outs->peak_mask; o.peak_count = outs->peak_count; o.center = outs->center; o.size = outs->size;
            o.max_peaks = outs->max_peaks; o.scene_calmness = outs->scene_calmness; o.tuning_grid_inaccuracy = outs->tuning_grid_inaccuracy;
        }
        return b->impl->preprocess_device(d_db, n_frames, pvq::Duration{frame_time_ns}, frame_times_ns, o, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_analysis_batch_preprocess_pcm(pvq_analysis_batch* b, pvq_vqt* v, const float* const* d_pcm, const size_t* n_lead, size_t n_frames,
                                             size_t hop, uint64_t frame_time_ns, float* d_db, const pvq_analysis_batch_outputs* outs, void* stream) {
    try {
        if (!b || !v) return null_handle();
        const pvq::VqtRange& r = v->impl->params().range;
        if (b->impl->device() != v->impl->device() || b->impl->n_bins() != v->impl->n_bins() || b->impl->range().min_freq != r.min_freq ||
            b->impl->range().buckets_per_octave != r.buckets_per_octave) {
            pvq::set_last_error("the transform handle and the analysis batch must sit on the same device and share the VqtRange");
            return PVQ_ERR_INVALID_ARG;
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
        pvq::AnalysisBatchOutputs o;
        if (outs) {
            o.x_vqt_smoothed = outs->x_vqt_smoothed; o.x_vqt_peakfiltered = outs->x_vqt_peakfiltered; o.x_vqt_afterglow = outs->x_vqt_afterglow;
            o.calmness = outs->calmness; o.pitch_accuracy = outs->pitch_accuracy; o.pitch_deviation = outs->pitch_deviation;
            o.peak_mask = outs->peak_mask; o.peak_count = outs->peak_count; o.center = outs->center; o.size = outs->size;
            o.max_peaks = outs->max_peaks; o.scene_calmness = outs->scene_calmness; o.tuning_grid_inaccuracy = outs->tuning_grid_inaccuracy;
        }
        return b->impl->preprocess_device(db, n_frames, pvq::Duration{frame_time_ns}, nullptr, o, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_analysis_batch_get_field(pvq_analysis_batch* b, uint32_t stream_index, pvq_analysis_field f, float* out) {
    try {
        if (!b) return null_handle();
        return b->impl->get_field(stream_index, (int)f, out);
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_analysis_batch_get_scalars(pvq_analysis_batch* b, uint32_t stream_index, float* scene_calmness, float* tuning_grid_inaccuracy) {
    try {
        if (!b) return null_handle();
        return b->impl->get_scalars(stream_index, scene_calmness, tuning_grid_inaccuracy);
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_vqt_set_profiling(pvq_vqt* v, int enable) {
    try {
        if (!v) return null_handle();
        v->impl->set_profiling(enable == 2 ? 2 : (enable != 0 ? 1 : 0));
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
uint32_t pvq_vqt_last_kernel_ms(pvq_vqt* v, float* out_ms, uint32_t capacity) {
    try {
        if (!v || !out_ms) return 0;
        return v->impl->last_kernel_ms(out_ms, capacity);
    } catch (...) { (void)translate_exception(); return 0; }
}
uint32_t pvq_vqt_last_kernel_launches(pvq_vqt* v, uint32_t* out_n, uint32_t capacity) {
    try {
        if (!v || !out_n) return 0;
        return v->impl->last_kernel_launches(out_n, capacity);
    } catch (...) { (void)translate_exception(); return 0; }
}
pvq_status pvq_vqt_input_status(pvq_vqt* v, void* stream) {
    try {
        if (!v) return null_handle();
        return v->impl->input_status(static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
double pvq_vqt_last_gemm_flop(const pvq_vqt* v) {
    try {
        return v ? v->impl->last_gemm_flop() : 0.0;
    } catch (...) { (void)translate_exception(); return 0.0; }
}
float pvq_vqt_last_sclk_mhz(pvq_vqt* v) {
    try {
        return v ? v->impl->last_sclk_mhz() : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}
uint32_t pvq_vqt_last_frames_per_launch(const pvq_vqt* v) {
    try {
        return v ? v->impl->last_frames_per_launch() : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}
const char* pvq_vqt_kernel_name(uint32_t slot) {
    try {
        return pvq::Vqt::slot_name(slot);
    } catch (...) { (void)translate_exception(); return nullptr; }
}

// ------------------------------------------------------------------------------------------------
// callers either side of the path
// ------------------------------------------------------------------------------------------------
pvq_status pvq_mono_agc_create(float desired_output_rms, float distortion_factor, pvq_mono_agc** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::string why;
        if (!pvq::MonoAgc::valid(desired_output_rms, distortion_factor, &why)) {
            pvq::set_last_error(why);
            return PVQ_ERR_INVALID_ARG;
        }
        *out = new pvq_mono_agc{pvq::MonoAgc(desired_output_rms, distortion_factor)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_mono_agc_destroy(pvq_mono_agc* a) {
    try {
        delete a;
    } catch (...) { (void)translate_exception(); }
}
void pvq_mono_agc_freeze_gain(pvq_mono_agc* a, int freeze) {
    try {
        if (a) a->impl.freeze_gain(freeze != 0);
    } catch (...) { (void)translate_exception(); }
}
int pvq_mono_agc_is_gain_frozen(const pvq_mono_agc* a) {
    try {
        return a && a->impl.is_gain_frozen() ? 1 : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}
float pvq_mono_agc_gain(const pvq_mono_agc* a) {
    try {
        return a ? a->impl.gain() : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}
void pvq_mono_agc_process(pvq_mono_agc* a, float* samples, size_t n) {
    try {
        if (a && samples) a->impl.process(samples, n);
    } catch (...) { (void)translate_exception(); }
}

size_t pvq_train_chunk_samples(const pvq_vqt* v) {
    try {
        return v ? pvq::train_chunk_samples(v->impl->delay_seconds(), v->impl->params().sr) : 0;
    } catch (...) { (void)translate_exception(); return 0; }
}
pvq_status pvq_train_condition_stream(pvq_mono_agc* a, const float* left, const float* right, size_t n_chunks, size_t chunk,
                                      float* mono_out, float* gain_out) {
    try {
        if (!a || !left || !mono_out) return null_handle();
        pvq::train_condition_stream(a->impl, left, right, n_chunks, chunk, mono_out, gain_out);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
// train.rs:146-163 + 286-301: the conditioning of many files side by side, on the device (condition_batch.hpp)
pvq_status pvq_agc_batch_create(int device_id, uint32_t n_streams, float desired_output_rms, float distortion_factor, pvq_agc_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::AgcBatch> impl;
        const pvq_status st = pvq::AgcBatch::create(device_id, n_streams, desired_output_rms, distortion_factor, impl);   // lib.rs:35-53
        if (st != PVQ_OK) return st;
        *out = new pvq_agc_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_agc_batch_destroy(pvq_agc_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_agc_batch_condition_device(pvq_agc_batch* b, const float* const* d_left, const float* const* d_right, const size_t* n_chunks,
                                          size_t chunk, float* const* d_mono_out, float* d_gain_out, size_t gain_stride, void* stream) {
    try {
        if (!b) return null_handle();
        return b->impl->condition_device(d_left, d_right, n_chunks, chunk, d_mono_out, d_gain_out, gain_stride,
                                         static_cast<hipStream_t>(stream));   // train.rs:286-301
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_agc_batch_get_gains(pvq_agc_batch* b, float* gains) {
    try {
        if (!b) return null_handle();
        return b->impl->get_gains(gains);   // lib.rs:72
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_train_frames_db(pvq_vqt* v, const float* mono, size_t n_chunks, size_t chunk, size_t step, float* out_db) {
    try {
        if (!v || !mono || !out_db) return null_handle();
        if (chunk == 0 || step == 0) {
            pvq::set_last_error("chunk and step must be positive");
            return PVQ_ERR_INVALID_ARG;
        }
        const size_t n_frames = n_chunks / step;
        if (n_frames == 0) return PVQ_OK;
        return v->impl->calculate_batch_db(mono, 0, chunk * step, n_frames, out_db);
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_train_rows(const float* db, size_t n_frames, uint32_t n_bins, const uint32_t* voice_ptr, const int32_t* voice_key,
                          const float* voice_gain_left, const float* voice_gain_right, const float* agc_gain, float* out_rows) {
    try {
        if (!db || !voice_ptr || !agc_gain || !out_rows) return null_handle();
        std::string why;
        if (!pvq::train_rows(db, n_frames, n_bins, voice_ptr, voice_key, voice_gain_left, voice_gain_right, agc_gain, out_rows, &why)) {
            pvq::set_last_error(why);
            return PVQ_ERR_INVALID_ARG;
        }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_npy_write_f32(const char* path, const float* data, uint64_t n) {
    try {
        if (!path || (!data && n)) return null_handle();
        std::string why;
        if (!pvq::npy_write_f32(path, data, n, &why)) {
            pvq::set_last_error(why);
            return PVQ_ERR_INVALID_ARG;
        }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

pvq_status pvq_stream_create(pvq_vqt* v, size_t buf_size, int with_agc, pvq_stream** out) {
    try {
        if (!v || !out) return null_handle();
        *out = nullptr;
        const size_t n_fft = v->impl->params().n_fft;
        if (buf_size < n_fft) {
            pvq::set_last_error("ring buffer shorter than n_fft");
            return PVQ_ERR_BAD_LENGTH;
        }
        if (!v->impl->has_device()) {
            pvq::set_last_error("the streaming front end needs a GPU handle");
            return PVQ_ERR_NO_DEVICE;
        }
        auto s = std::make_unique<pvq_stream>();
        s->vqt = v;
        s->buf_size = buf_size;
        s->cap = 4 * buf_size;
        s->with_agc = with_agc != 0;
        PVQ_HIP(hipSetDevice(v->impl->device()));
        PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_ring), s->cap * sizeof(float)));
        PVQ_HIP(hipMemset(s->d_ring, 0, s->cap * sizeof(float)));
        PVQ_HIP(hipStreamSynchronize(nullptr));   // (the object's own stream does not wait for the null stream)
        PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_db), v->impl->n_bins() * sizeof(float)));
        PVQ_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_in), buf_size * sizeof(float), hipHostMallocDefault));
        PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_out), v->impl->n_bins() * sizeof(float), hipHostMallocDefault));
        s->w = buf_size;
        *out = s.release();
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_stream_destroy(pvq_stream* s) {
    try {
        delete s;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_stream_push(pvq_stream* s, const float* data, size_t n) {
    try {
        if (!s || (!data && n)) return null_handle();
        if (n == 0) return PVQ_OK;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(data[i])) return PVQ_OK;   // audio_desktop.rs:97-100: the chunk is dropped
        if (n > s->buf_size) {                            // Vec::drain(..n) would panic
            pvq::set_last_error("chunk longer than the ring buffer");
            return PVQ_ERR_BAD_LENGTH;
        }
        PVQ_HIP(hipSetDevice(s->vqt->impl->device()));
        if (s->in_flight) {   // a second push before the previous one's copy was waited for (no frame in between)
            PVQ_HIP(hipStreamSynchronize(s->stream));
            s->in_flight = false;
        }
        std::copy(data, data + n, s->h_in);
        if (s->with_agc) {
            float sq = 0.0f;
            for (size_t i = 0; i < n; ++i) sq += data[i] * data[i];     // audio_desktop.rs:101
            s->agc.freeze_gain(sq < 1e-6f);                             // :102
            s->agc.process(s->h_in, n);                                 // :111 (over the newest samples of the ring)
            s->gain = s->agc.gain();                                    // :112
        }
        if (s->w + n > s->cap) {   // compact: newest buf_size samples to the front (ranges do not overlap: cap = 4 buf_size)
            PVQ_HIP(hipMemcpyAsync(s->d_ring, s->d_ring + s->w - s->buf_size, s->buf_size * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
            s->w = s->buf_size;
        }
        PVQ_HIP(hipMemcpyAsync(s->d_ring + s->w, s->h_in, n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        s->in_flight = true;
        s->w += n;
        s->chunk_size_ms = static_cast<float>(n) / s->vqt->impl->params().sr * 1000.0f;   // :118
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
float pvq_stream_gain(const pvq_stream* s) {
    try {
        return s ? s->gain : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}
float pvq_stream_chunk_size_ms(const pvq_stream* s) {
    try {
        return s ? s->chunk_size_ms : 0.0f;
    } catch (...) { (void)translate_exception(); return 0.0f; }
}
pvq_status pvq_stream_frame_db(pvq_stream* s, float* out_db) {
    try {
        if (!s || !out_db) return null_handle();
        const size_t n_fft = s->vqt->impl->params().n_fft;
        // one frame over the newest n_fft samples: n_lead = n_fft - 1 samples of history + a hop of 1
        pvq_status st = s->vqt->impl->calculate_batch_db_device(s->d_ring + s->w - n_fft, n_fft - 1, 1, 1, s->d_db, nullptr, s->stream);
        if (st != PVQ_OK) return st;
        const size_t nb = s->vqt->impl->n_bins();
        PVQ_HIP(hipMemcpyAsync(s->h_out, s->d_db, nb * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        PVQ_HIP(hipStreamSynchronize(s->stream));
        s->in_flight = false;
        std::copy(s->h_out, s->h_out + nb, out_db);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_stream_read(pvq_stream* s, float* out, size_t n_last) {
    try {
        if (!s || !out) return null_handle();
        if (n_last > s->buf_size) {
            pvq::set_last_error("n_last exceeds the ring buffer");
            return PVQ_ERR_BAD_LENGTH;
        }
        PVQ_HIP(hipSetDevice(s->vqt->impl->device()));
        PVQ_HIP(hipStreamSynchronize(s->stream));   // the appends queued on the object's stream
        s->in_flight = false;
        PVQ_HIP(hipMemcpy(out, s->d_ring + s->w - n_last, n_last * sizeof(float), hipMemcpyDeviceToHost));
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

void* pvq_host_alloc(size_t bytes) {
    try {
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
        if (e != hipSuccess) {
            pvq::set_last_error(std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
            return nullptr;
        }
        return p;
    } catch (...) { (void)translate_exception(); return nullptr; }
}
void pvq_host_free(void* p) {
    try {
        if (p) (void)hipHostFree(p);
    } catch (...) { (void)translate_exception(); }
}

void pvq_calculate_color(uint16_t buckets_per_octave, float bucket, const float* colors, float gray_level, float easing_pow,
                         float out_rgb[3]) {
    try {
        pvq::calculate_color(buckets_per_octave, bucket, reinterpret_cast<const float(*)[3]>(colors), gray_level, easing_pow, out_rgb);
    } catch (...) { (void)translate_exception(); }
}
size_t pvq_led_frame(uint32_t n_buckets, uint16_t buckets_per_octave, const float* center, const float* size, uint32_t n_peaks,
                     const float* colors, float gray_level, float easing_pow, uint8_t* out) {
    try {
        return pvq::led_frame(n_buckets, buckets_per_octave, center, size, n_peaks, reinterpret_cast<const float(*)[3]>(colors),
                              gray_level, easing_pow, out);
    } catch (...) { (void)translate_exception(); return 0; }
}

// pitchvis_viewer/src/display_system/update.rs:961-1065: the spectrogram row of one AnalysisState
pvq_status pvq_spectrogram_row(int mode, uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, const float* center,
                               const float* size, uint32_t n_peaks, const float* colors, float gray_level, float easing_pow, uint8_t* out_rgba) {
    try {
        if (mode != PVQ_SPECTROGRAM_VQT && mode != PVQ_SPECTROGRAM_PEAKS) {
            pvq::set_last_error("unknown spectrogram mode");
            return PVQ_ERR_INVALID_ARG;
        }
        if (buckets_per_octave == 0 || !colors || (!out_rgba && n_buckets) || (mode == PVQ_SPECTROGRAM_VQT && !x_vqt_smoothed && n_buckets) ||
            (mode == PVQ_SPECTROGRAM_PEAKS && n_peaks && (!center || !size))) {
            pvq::set_last_error("spectrogram row: buckets_per_octave == 0 or a missing array");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::spectrogram_row(mode, n_buckets, buckets_per_octave, x_vqt_smoothed, center, size, n_peaks,
                             reinterpret_cast<const float(*)[3]>(colors), gray_level, easing_pow, out_rgba);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
// update.rs:1102-1131: the chroma strengths of one AnalysisState
pvq_status pvq_chroma_row(float min_freq, uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, float out12[12]) {
    try {
        if (buckets_per_octave == 0 || !out12 || (!x_vqt_smoothed && n_buckets)) {
            pvq::set_last_error("chroma row: buckets_per_octave == 0 or a missing array");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::chroma_row(min_freq, n_buckets, buckets_per_octave, x_vqt_smoothed, out12);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
// update.rs:961-1065 + 1102-1131 and pitchvis_serial/src/main.rs:122-175 for many rows, on the device (render_batch.hpp)
pvq_status pvq_render_batch_create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave, const float* colors,
                                   float gray_level, float easing_pow, pvq_render_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::RenderBatch> impl;
        const pvq_status st = pvq::RenderBatch::create(device_id, min_freq, octaves, buckets_per_octave, colors, gray_level, easing_pow, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_render_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_render_batch_destroy(pvq_render_batch* r) {
    try {
        delete r;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_render_batch_rows_device(pvq_render_batch* r, size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center,
                                        const float* d_size, const uint32_t* d_peak_count, uint32_t max_peaks, const pvq_render_outputs* outs,
                                        void* stream) {
    try {
        if (!r) return null_handle();
        const pvq_render_outputs none{};
        return r->impl->rows_device(n_rows, d_x_vqt_smoothed, d_center, d_size, d_peak_count, max_peaks, outs ? *outs : none,
                                    static_cast<hipStream_t>(stream));   // update.rs:961-1065, 1102-1131; main.rs:122-175
    } catch (...) { return translate_exception(); }
}

// pitchvis_viewer/src/display_system/update.rs:38-426: the pitch-ball scene, one stream on the host (scene_host.hpp) and many on the
// device (scene_batch.hpp)
void pvq_scene_default_settings(pvq_scene_settings* s) {
    if (!s) return;
    s->visuals_mode = PVQ_VISUALS_FULL;
    s->enable_bloom = 1;
    s->colors = nullptr;
    s->gray_level = 60.0f;   // pitchvis_colors/src/lib.rs:56-57
    s->easing_pow = 1.3f;
}
pvq_status pvq_scene_state_create(uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings* settings, pvq_scene_state** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        if (octaves == 0 || buckets_per_octave == 0 || static_cast<uint64_t>(octaves) * buckets_per_octave > 0x7FFFFFFFull) {
            pvq::set_last_error("scene: octaves and buckets_per_octave must be positive");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq_scene_settings cfg;
        pvq_scene_default_settings(&cfg);
        if (settings) cfg = *settings;
        pvq::scene::Settings s;
        if (!pvq::scene_settings(octaves, buckets_per_octave, cfg.visuals_mode, cfg.enable_bloom, cfg.colors, cfg.gray_level, cfg.easing_pow, s)) {
            pvq::set_last_error("scene: unknown visuals mode");
            return PVQ_ERR_INVALID_ARG;
        }
        *out = new pvq_scene_state{std::unique_ptr<pvq::SceneState>(new pvq::SceneState(s))};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_scene_state_destroy(pvq_scene_state* s) {
    try {
        delete s;
    } catch (...) { (void)translate_exception(); }
}
uint32_t pvq_scene_state_n_bins(const pvq_scene_state* s) { return s ? s->impl->settings().n_bins : 0; }
uint32_t pvq_scene_state_n_segments(const pvq_scene_state* s) { return s ? s->impl->settings().n_segments : 0; }
pvq_status pvq_scene_state_update(pvq_scene_state* s, const float* center, const float* size, uint32_t n_peaks, const float* calmness,
                                  const float* pitch_accuracy, const float* pitch_deviation, float scene_calmness, uint64_t frame_time_ns) {
    try {
        if (!s) return null_handle();
        if (n_peaks && (!center || !size || !calmness || !pitch_accuracy || !pitch_deviation)) {
            pvq::set_last_error("scene: a frame with peaks needs center, size, calmness, pitch_accuracy and pitch_deviation");
            return PVQ_ERR_INVALID_ARG;
        }
        s->impl->update(center, size, n_peaks, calmness, pitch_accuracy, pitch_deviation, scene_calmness, frame_time_ns);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_scene_state_get(const pvq_scene_state* s, float* ball_xyzs, float* ball_rgba, float* ball_params, uint32_t* ball_visible,
                               uint32_t* bass_lit, float* bass_rgba, float* bloom) {
    try {
        if (!s) return null_handle();
        const pvq::SceneBalls& b = s->impl->balls();
        const uint32_t n = s->impl->settings().n_bins;
        if (ball_visible)
            for (uint32_t w = 0; w < (n + 31) / 32; ++w) ball_visible[w] = 0u;
        for (uint32_t i = 0; i < n; ++i) {
            if (ball_xyzs) { ball_xyzs[4 * i] = b.x[i]; ball_xyzs[4 * i + 1] = b.y[i]; ball_xyzs[4 * i + 2] = b.z[i]; ball_xyzs[4 * i + 3] = b.scale[i]; }
            if (ball_rgba) { ball_rgba[4 * i] = b.r[i]; ball_rgba[4 * i + 1] = b.g[i]; ball_rgba[4 * i + 2] = b.b[i]; ball_rgba[4 * i + 3] = b.a[i]; }
            if (ball_params) { ball_params[3 * i] = b.calmness[i]; ball_params[3 * i + 1] = b.accuracy[i]; ball_params[3 * i + 2] = b.deviation[i]; }
            if (ball_visible && b.visible[i]) ball_visible[i / 32] |= 1u << (i % 32);
        }
        if (bass_lit) *bass_lit = s->impl->bass_lit();
        if (bass_rgba)
            for (int i = 0; i < 4; ++i) bass_rgba[i] = s->impl->bass_rgba()[i];
        if (bloom) *bloom = s->impl->bloom();
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_scene_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings* settings,
                                  uint32_t n_streams, pvq_scene_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::SceneBatch> impl;
        const pvq_status st = pvq::SceneBatch::create(device_id, octaves, buckets_per_octave, settings, n_streams, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_scene_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_scene_batch_destroy(pvq_scene_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
uint32_t pvq_scene_batch_n_segments(const pvq_scene_batch* b) { return b ? b->impl->n_segments() : 0; }
pvq_status pvq_scene_batch_frames_device(pvq_scene_batch* b, size_t n_frames, const pvq_scene_inputs* in, uint64_t frame_time_ns,
                                         const uint64_t* frame_times_ns, const pvq_scene_outputs* outs, void* stream) {
    try {
        if (!b) return null_handle();
        const pvq_scene_inputs no_in{};
        const pvq_scene_outputs none{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, frame_time_ns, frame_times_ns, outs ? *outs : none,
                                      static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_scene_batch_get_state(pvq_scene_batch* b, uint32_t stream_index, float* ball_xyzs, float* ball_rgba, float* ball_params,
                                     uint32_t* ball_visible, uint32_t* bass_lit, float* bass_rgba, float* bloom) {
    try {
        if (!b) return null_handle();
        return b->impl->get_state(stream_index, ball_xyzs, ball_rgba, ball_params, ball_visible, bass_lit, bass_rgba, bloom);
    } catch (...) { return translate_exception(); }
}

// noisy_color_rings_2d.wgsl:395-428 with setup.rs:110-112, :359-365: the pitch balls as pixels, one frame on the host
// (raster_host.hpp) and many streams on the device (raster_batch.hpp)
pvq_status pvq_raster_shade(const float* rgba, const float* params, float u, float v, float* out4) {
    try {
        if (!rgba || !params || !out4) {
            pvq::set_last_error("raster shade: rgba, params and out4 are needed");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::raster_shade(rgba, params, u, v, out4);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_raster_touch(uint32_t n_bins, const float* center, uint32_t n_peaks, float elapsed, float* time_inout) {
    try {
        if (!time_inout || (n_peaks && !center)) {
            pvq::set_last_error("raster touch: time_inout is needed, and center with n_peaks > 0");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::raster_touch(n_bins, center, n_peaks, elapsed, time_inout);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_raster_frame(uint32_t n_bins, uint32_t width, uint32_t height, float viewport_height, int visuals_mode, const float* ball_xyzs,
                            const float* ball_rgba, const float* ball_params, const uint32_t* ball_visible, const float* ball_time,
                            const float* background, float* image_out) {
    try {
        if (!ball_xyzs || !ball_rgba || !ball_params || !ball_visible || !ball_time || !image_out) {
            pvq::set_last_error("raster frame: the five ball arrays and image_out are needed");
            return PVQ_ERR_INVALID_ARG;
        }
        std::string err;
        if (!pvq::stage_image_ok("raster frame", width, height, viewport_height, err) || !pvq::stage_mode_ok("raster frame", visuals_mode, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::raster_frame(n_bins, width, height, viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height, visuals_mode,
                          ball_xyzs, ball_rgba, ball_params, ball_visible, ball_time, background, image_out);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_raster_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                   uint32_t n_streams, uint32_t width, uint32_t height, pvq_raster_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::RasterBatch> impl;
        const pvq_status st = pvq::RasterBatch::create(device_id, octaves, buckets_per_octave, visuals_mode, viewport_height, n_streams,
                                                       width, height, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_raster_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_raster_batch_destroy(pvq_raster_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_raster_batch_frames_device(pvq_raster_batch* b, size_t n_frames, const pvq_raster_inputs* in, const float* elapsed_s,
                                          float* d_image, float* d_ball_time, void* stream) {
    try {
        if (!b) return null_handle();
        const pvq_raster_inputs no_in{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, elapsed_s, d_image, d_ball_time, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_raster_batch_get_times(pvq_raster_batch* b, uint32_t stream_index, float* out) {
    try {
        if (!b) return null_handle();
        return b->impl->get_times(stream_index, out);
    } catch (...) { return translate_exception(); }
}

// pitchvis_viewer/src/display_system/update.rs:474-869: the debug panels, one stream on the host (panels_host.hpp) and many on the
// device (panels_batch.hpp)
pvq_status pvq_spectrum_mesh(uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, const float* center, const float* size,
                             uint32_t n_peaks, const float* colors, float gray_level, float* line_pos, float* line_rgba, float* disc_pos,
                             float* disc_rgba) {
    try {
        if (n_buckets < 2 || buckets_per_octave == 0 || !colors) {
            pvq::set_last_error("spectrum mesh: n_buckets < 2, buckets_per_octave == 0 or no colors");
            return PVQ_ERR_INVALID_ARG;
        }
        if (((line_pos || line_rgba) && !x_vqt_smoothed) || ((disc_pos || disc_rgba) && n_peaks && (!center || !size))) {
            pvq::set_last_error("spectrum mesh: the line reads x_vqt_smoothed, the discs read center and size");
            return PVQ_ERR_INVALID_ARG;
        }
        std::vector<float> rgb(3 * static_cast<size_t>(buckets_per_octave));
        float cs[24];
        pvq::panel_color_table(buckets_per_octave, colors, gray_level, rgb.data());
        pvq::panel_disc_table(cs);
        pvq::spectrum_mesh(n_buckets, buckets_per_octave, x_vqt_smoothed, center, size, n_peaks, rgb.data(), cs, line_pos, line_rgba, disc_pos,
                           disc_rgba);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_calmness_histogram_mesh(uint32_t n_buckets, const float* calmness, float* pos, float* rgba) {
    try {
        if (n_buckets < 2 || !calmness) {
            pvq::set_last_error("calmness histogram: n_buckets < 2 or no calmness");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::calmness_histogram_mesh(n_buckets, calmness, pos, rgba);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_calmness_graph_create(uint32_t capacity, pvq_calmness_graph** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        const uint32_t cap = capacity ? capacity : pvq::panels::DEFAULT_GRAPH_CAPACITY;
        if (cap < 2 || cap > 1024) {
            pvq::set_last_error("calmness graph: capacity must be 2 .. 1024 (0: 300)");
            return PVQ_ERR_INVALID_ARG;
        }
        *out = new pvq_calmness_graph{pvq::CalmnessGraph(cap)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_calmness_graph_destroy(pvq_calmness_graph* g) {
    try {
        delete g;
    } catch (...) { (void)translate_exception(); }
}
uint32_t pvq_calmness_graph_capacity(const pvq_calmness_graph* g) { return g ? g->impl.capacity() : 0; }
pvq_status pvq_calmness_graph_push(pvq_calmness_graph* g, float value) {
    try {
        if (!g) return null_handle();
        g->impl.push(value);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_calmness_graph_mesh(const pvq_calmness_graph* g, float* pos, float* rgba, float* history) {
    try {
        if (!g) return null_handle();
        g->impl.mesh(pos, rgba);
        if (history) g->impl.history(history);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_panel_topology(uint32_t n_quads, uint32_t n_circles, uint32_t* indices, float* uvs) {
    try {
        if (4ull * n_quads + 13ull * n_circles > 0xFFFFFFFFull) {
            pvq::set_last_error("panel topology: the vertex count does not fit a u32 index");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::panel_topology(n_quads, n_circles, indices, uvs);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_panels_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const float* colors, float gray_level,
                                   uint32_t n_streams, uint32_t graph_capacity, pvq_panels_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::PanelsBatch> impl;
        const pvq_status st = pvq::PanelsBatch::create(device_id, octaves, buckets_per_octave, colors, gray_level, n_streams, graph_capacity, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_panels_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_panels_batch_destroy(pvq_panels_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
uint32_t pvq_panels_batch_graph_capacity(const pvq_panels_batch* b) { return b ? b->impl->graph_capacity() : 0; }
pvq_status pvq_panels_batch_rows_device(pvq_panels_batch* b, size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center,
                                        const float* d_size, const uint32_t* d_peak_count, uint32_t max_peaks, const float* d_calmness,
                                        const pvq_panels_outputs* outs, void* stream) {
    try {
        if (!b) return null_handle();
        const pvq_panels_outputs none{};
        return b->impl->rows_device(n_rows, d_x_vqt_smoothed, d_center, d_size, d_peak_count, max_peaks, d_calmness, outs ? *outs : none,
                                    static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_panels_batch_graph_device(pvq_panels_batch* b, size_t n_frames, const float* d_scene_calmness, size_t first_emitted,
                                         float* graph_pos, float* graph_rgba, void* stream) {
    try {
        if (!b) return null_handle();
        return b->impl->graph_device(n_frames, d_scene_calmness, first_emitted, graph_pos, graph_rgba, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_panels_batch_get_history(pvq_panels_batch* b, uint32_t stream_index, float* out) {
    try {
        if (!b) return null_handle();
        return b->impl->get_history(stream_index, out);
    } catch (...) { return translate_exception(); }
}

// The picture behind the balls — spider net, debug panels, lit bass spiral (setup.rs:127-222, update.rs:369-425, :474-869 as pixels):
// one frame on the host (backdrop_host.hpp) and many streams on the device (backdrop_batch.hpp)
pvq_status pvq_backdrop_geometry(uint32_t octaves, int what, float* quads_out, uint32_t* n_out) {
    try {
        if (octaves == 0 || octaves > 1024 || what < pvq::backdrop::NET_SPIRAL || what > pvq::backdrop::BASS) {
            pvq::set_last_error("backdrop geometry: octaves 1 .. 1024, what one of net spiral, rays, bass");
            return PVQ_ERR_INVALID_ARG;
        }
        if (n_out) *n_out = pvq::backdrop::geometry_count(octaves, what);
        if (quads_out) {
            const std::vector<float> q = pvq::backdrop_geometry(octaves, what);
            std::copy(q.begin(), q.end(), quads_out);
        }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_backdrop_panel_transforms(uint32_t n_bins, uint32_t width, uint32_t height, float viewport_height, float* out) {
    try {
        if (!out) {
            pvq::set_last_error("backdrop panel transforms: out is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        std::string err;
        if (!pvq::stage_image_ok("backdrop panel transforms", width, height, viewport_height, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::backdrop::panel_transforms(n_bins, width, height, viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height, out);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_backdrop_draw_mesh(uint32_t width, uint32_t height, float viewport_height, size_t n_triangles, const float* pos, const float* rgba,
                                  const float* transform, float* image_inout) {
    try {
        if (!image_inout || (n_triangles && (!pos || !rgba))) {
            pvq::set_last_error("backdrop draw mesh: image_inout is needed, and pos and rgba with n_triangles > 0");
            return PVQ_ERR_INVALID_ARG;
        }
        std::string err;
        if (!pvq::stage_image_ok("backdrop draw mesh", width, height, viewport_height, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::backdrop_draw_mesh(width, height, viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height, n_triangles, pos, rgba,
                                transform, image_inout);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_backdrop_frame(uint32_t octaves, uint32_t buckets_per_octave, uint32_t width, uint32_t height, float viewport_height,
                              int visuals_mode, uint32_t bass_lit, const float* bass_rgba, const pvq_backdrop_panels* panels,
                              const float* background, float* image_out) {
    try {
        if (!image_out || (bass_lit && !bass_rgba)) {
            pvq::set_last_error("backdrop frame: image_out is needed, and bass_rgba with bass_lit > 0");
            return PVQ_ERR_INVALID_ARG;
        }
        const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
        if (octaves == 0 || buckets_per_octave == 0 || octaves > 1024 || n < 2 || n > 0x7FFFFFFFull) {
            pvq::set_last_error("backdrop frame: octaves 1 .. 1024, buckets_per_octave positive, at least two bins");
            return PVQ_ERR_INVALID_ARG;
        }
        std::string err;
        if (!pvq::stage_image_ok("backdrop frame", width, height, viewport_height, err) || !pvq::stage_mode_ok("backdrop frame", visuals_mode, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        if (panels && (!panels->line_pos != !panels->line_rgba || !panels->disc_pos != !panels->disc_rgba ||
                       !panels->hist_pos != !panels->hist_rgba || !panels->graph_pos != !panels->graph_rgba ||
                       (panels->graph_pos && panels->graph_capacity < 2))) {
            pvq::set_last_error("backdrop frame: a mesh needs its positions and its colours, the graph its graph_capacity >= 2");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::backdrop_frame(octaves, buckets_per_octave, width, height, viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height,
                            visuals_mode, bass_lit, bass_rgba, panels, background, image_out);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_backdrop_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                     uint32_t n_streams, uint32_t width, uint32_t height, pvq_backdrop_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::BackdropBatch> impl;
        const pvq_status st = pvq::BackdropBatch::create(device_id, octaves, buckets_per_octave, visuals_mode, viewport_height, n_streams,
                                                         width, height, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_backdrop_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_backdrop_batch_destroy(pvq_backdrop_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_backdrop_batch_frames_device(pvq_backdrop_batch* b, size_t n_frames, const pvq_backdrop_inputs* in, float* d_image, void* stream) {
    try {
        if (!b) return null_handle();
        const pvq_backdrop_inputs no_in{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, d_image, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_backdrop_balls_over_device(pvq_raster_batch* b, size_t n_frames, const pvq_raster_inputs* in, const float* elapsed_s,
                                          float* d_image_inout, float* d_ball_time, void* stream) {
    try {
        if (!b) return null_handle();
        const pvq_raster_inputs no_in{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, elapsed_s, d_image_inout, d_ball_time, static_cast<hipStream_t>(stream), true);
    } catch (...) { return translate_exception(); }
}

// The spectrogram quad and the chroma boxes in front of the balls (setup.rs:418-541, update.rs:929-1172, spectrogram_scroll.wgsl):
// one stream on the host (overlay_host.hpp) and many streams on the device (overlay_batch.hpp)
namespace {
bool overlay_bins_ok(const char* who, uint32_t n_bins) {
    if (n_bins >= pvq::overlay::MIN_BINS && n_bins <= pvq::overlay::MAX_BINS) return true;
    pvq::set_last_error(std::string(who) + ": n_bins is 3 .. 1024");
    return false;
}
}  // namespace
pvq_status pvq_overlay_quad(uint32_t n_bins, uint32_t history_rows, float* out4) {
    try {
        std::string err;
        if (!out4) {
            pvq::set_last_error("overlay quad: out4 is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        if (!overlay_bins_ok("overlay quad", n_bins)) return PVQ_ERR_INVALID_ARG;
        if (!pvq::overlay_args_ok("overlay quad", history_rows, 0.0f, nullptr, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::overlay::reference_quad(n_bins, history_rows == 0 ? pvq::overlay::HISTORY_ROWS : history_rows, out4);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_overlay_state_create(uint32_t n_bins, uint32_t history_rows, pvq_overlay_state** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::string err;
        if (!overlay_bins_ok("overlay state", n_bins)) return PVQ_ERR_INVALID_ARG;
        if (!pvq::overlay_args_ok("overlay state", history_rows, 0.0f, nullptr, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        *out = new pvq_overlay_state{pvq::OverlayState(n_bins, history_rows == 0 ? pvq::overlay::HISTORY_ROWS : history_rows)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_overlay_state_destroy(pvq_overlay_state* s) {
    try {
        delete s;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_overlay_state_push(pvq_overlay_state* s, const uint8_t* row_rgba) {
    try {
        if (!s) return null_handle();
        if (!row_rgba) {
            pvq::set_last_error("overlay state: row_rgba is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        s->impl.push(row_rgba);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_overlay_state_texture(const pvq_overlay_state* s, uint8_t* out, uint32_t* write_index) {
    try {
        if (!s) return null_handle();
        if (out) std::memcpy(out, s->impl.texture(), static_cast<size_t>(s->impl.history_rows()) * s->impl.n_bins() * 4);
        if (write_index) *write_index = s->impl.write_index();
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_overlay_frame(const pvq_overlay_state* state, uint32_t width, uint32_t height, float viewport_height, float ui_scale,
                             const float* quad, const float* chroma12, const float* colors, float* image_inout) {
    try {
        if (!image_inout || (!state && !chroma12)) {
            pvq::set_last_error("overlay frame: image_inout is needed, and a state or chroma12");
            return PVQ_ERR_INVALID_ARG;
        }
        std::string err;
        if (!pvq::stage_image_ok("overlay frame", width, height, viewport_height, err) ||
            !pvq::overlay_args_ok("overlay frame", 0, ui_scale, quad, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::overlay::Tables tables;
        pvq::overlay_tables(colors, tables);
        pvq::overlay_frame(state ? &state->impl : nullptr, width, height, viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height,
                           ui_scale == 0.0f ? 1.0f : ui_scale, quad, chroma12, tables, image_inout);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_overlay_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, uint32_t history_rows, float viewport_height,
                                    float ui_scale, const float* quad, const float* colors, uint32_t n_streams, uint32_t width, uint32_t height,
                                    pvq_overlay_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::OverlayBatch> impl;
        const pvq_status st = pvq::OverlayBatch::create(device_id, octaves, buckets_per_octave, history_rows, viewport_height, ui_scale, quad, colors,
                                                        n_streams, width, height, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_overlay_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_overlay_batch_destroy(pvq_overlay_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_overlay_batch_frames_device(pvq_overlay_batch* b, size_t n_frames, const uint8_t* d_rows, const float* d_chroma,
                                           float* d_image_inout, void* stream) {
    try {
        if (!b) return null_handle();
        return b->impl->frames_device(n_frames, d_rows, d_chroma, d_image_inout, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_overlay_batch_get_texture(pvq_overlay_batch* b, uint32_t stream_index, uint8_t* out, uint32_t* write_index) {
    try {
        if (!b) return null_handle();
        return b->impl->get_texture(stream_index, out, write_index);
    } catch (...) { return translate_exception(); }
}

// The pitch-name labels over the balls and under the overlay (setup.rs:386-416): a font the caller brings, one picture on the host
// (text_host.hpp) and many rows on the device (text_batch.hpp)
pvq_status pvq_text_font_from_ttf(const uint8_t* bytes, size_t n_bytes, pvq_text_font** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::TextFont> impl;
        std::string err;
        const pvq_status st = pvq::TextFont::from_ttf(bytes, n_bytes, impl, err);
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        *out = new pvq_text_font{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_text_font_from_outlines(uint32_t n_glyphs, const uint32_t* codepoints, const float* advances, const uint32_t* n_contours,
                                       const uint32_t* contour_ends, const uint32_t* n_points, const float* points, const uint8_t* on_curve,
                                       uint32_t units_per_em, float ascent, float descent, pvq_text_font** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::TextFont> impl;
        std::string err;
        const pvq_status st = pvq::TextFont::from_outlines(n_glyphs, codepoints, advances, n_contours, contour_ends, n_points, points, on_curve,
                                                           units_per_em, ascent, descent, impl, err);
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        *out = new pvq_text_font{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_text_font_destroy(pvq_text_font* f) {
    try {
        delete f;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_text_font_metrics(const pvq_text_font* f, uint32_t* units_per_em, float* ascent, float* descent) {
    try {
        if (!f) return null_handle();
        if (units_per_em) *units_per_em = f->impl->units_per_em();
        if (ascent) *ascent = f->impl->ascent();
        if (descent) *descent = f->impl->descent();
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_text_font_glyph(pvq_text_font* f, uint32_t codepoint, float* advance, uint32_t* n_contours, uint32_t* n_points,
                               uint32_t cap_contours, uint32_t cap_points, uint32_t* contour_ends, float* points, uint8_t* on_curve) {
    try {
        if (!f) return null_handle();
        const pvq::TextGlyph* g = nullptr;
        std::string err;
        const pvq_status st = f->impl->glyph(codepoint, g, err);
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        if (advance) *advance = g->advance;
        if (n_contours) *n_contours = static_cast<uint32_t>(g->contour_ends.size());
        if (n_points) *n_points = static_cast<uint32_t>(g->on_curve.size());
        if ((contour_ends && cap_contours < g->contour_ends.size()) || ((points || on_curve) && cap_points < g->on_curve.size())) {
            pvq::set_last_error("text font glyph: an array is smaller than the glyph; ask for the counts first");
            return PVQ_ERR_INVALID_ARG;
        }
        if (contour_ends) std::copy(g->contour_ends.begin(), g->contour_ends.end(), contour_ends);
        if (points) std::copy(g->points.begin(), g->points.end(), points);
        if (on_curve) std::copy(g->on_curve.begin(), g->on_curve.end(), on_curve);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_text_pitch_labels(uint32_t octaves, const float* colors, pvq_text_label* out12) {
    try {
        if (!out12 || octaves == 0 || octaves > 255) {
            pvq::set_last_error("text pitch labels: octaves is 1 .. 255 and out12 is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::text_pitch_labels(octaves, colors, out12);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
namespace {
pvq_status text_plans(const char* who, pvq_text_font* font, const pvq_text_label* labels, uint32_t n, uint32_t width, uint32_t height,
                      float viewport_height, std::vector<pvq::TextLabelPlan>& plans) {
    std::string err;
    if (!pvq::stage_image_ok(who, width, height, viewport_height, err)) {
        pvq::set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    const pvq_status st = pvq::text_plan(who, *font->impl, labels, n, width, height,
                                         viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height, plans, err);
    if (st != PVQ_OK) pvq::set_last_error(err);
    return st;
}
}  // namespace
pvq_status pvq_text_layout_query(pvq_text_font* font, const pvq_text_label* labels, uint32_t n, uint32_t width, uint32_t height,
                                 float viewport_height, pvq_text_layout* out_n) {
    try {
        if (!font) return null_handle();
        if (!out_n) {
            pvq::set_last_error("text layout: out_n is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        std::vector<pvq::TextLabelPlan> plans;
        if (pvq_status st = text_plans("text layout", font, labels, n, width, height, viewport_height, plans)) return st;
        for (uint32_t l = 0; l < n; ++l) {
            const pvq::TextLabelPlan& p = plans[l];
            out_n[l] = pvq_text_layout{p.on_image ? 1u : 0u, p.x0, p.y0, p.x1, p.y1, p.on_image ? static_cast<uint32_t>(p.segments.size()) : 0u,
                                       p.n_tiles(), p.origin_x, p.baseline_y};
        }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_text_frame(pvq_text_font* font, const pvq_text_label* labels, uint32_t n, uint32_t width, uint32_t height, float viewport_height,
                          float* image_inout, float* coverage_out) {
    try {
        if (!font) return null_handle();
        if (!image_inout && !coverage_out) {
            pvq::set_last_error("text frame: image_inout or coverage_out is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        std::vector<pvq::TextLabelPlan> plans;
        if (pvq_status st = text_plans("text frame", font, labels, n, width, height, viewport_height, plans)) return st;
        pvq::text_frame(plans, width, height, image_inout, coverage_out);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_text_batch_create(int device_id, pvq_text_font* font, const pvq_text_label* labels, uint32_t n, float viewport_height,
                                 uint32_t width, uint32_t height, pvq_text_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        if (!font) return null_handle();
        std::unique_ptr<pvq::TextBatch> impl;
        const pvq_status st = pvq::TextBatch::create(device_id, *font->impl, labels, n, viewport_height, width, height, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_text_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_text_batch_destroy(pvq_text_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_text_batch_rows_device(pvq_text_batch* b, size_t n_rows, float* d_image_inout, void* stream) {
    try {
        if (!b) return null_handle();
        return b->impl->rows_device(n_rows, d_image_inout, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_text_batch_get_coverage(pvq_text_batch* b, int label, float* out) {
    try {
        if (!b) return null_handle();
        return b->impl->get_coverage(label, out);
    } catch (...) { return translate_exception(); }
}

// Bloom, display transform and sRGB bytes (setup.rs:347-383, update.rs:346-347): one picture on the host (present_host.hpp) and many
// on the device (present_batch.hpp)
namespace {
pvq::present::Settings present_settings(const pvq_present_settings* s) {
    if (!s) return pvq::present::default_settings();
    return pvq::present::Settings{s->low_frequency_boost, s->low_frequency_boost_curvature, s->high_pass_frequency, s->threshold,
                                  s->threshold_softness,  s->composite_mode,                s->max_mip_dimension,   s->tonemapping};
}
}  // namespace
void pvq_present_default_settings(pvq_present_settings* s) {
    if (!s) return;
    const pvq::present::Settings d = pvq::present::default_settings();
    *s = pvq_present_settings{d.low_frequency_boost, d.low_frequency_boost_curvature, d.high_pass_frequency, d.threshold,
                              d.threshold_softness,  d.composite_mode,                d.max_mip_dimension,   d.tonemapping};
}
pvq_status pvq_present_mips(uint32_t width, uint32_t height, uint32_t max_mip_dimension, uint32_t* out_count, uint32_t* out_sizes) {
    try {
        std::string err;
        pvq::present::Settings s = pvq::present::default_settings();
        s.max_mip_dimension = max_mip_dimension;
        if (!pvq::stage_image_ok("present mips", width, height, 0.0f, err) || !pvq::present_settings_ok("present mips", s, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::PresentPlan plan;
        if (!pvq::present_plan("present mips", width, height, pvq::present_resolved(s).max_mip_dimension, plan, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_UNSUPPORTED;
        }
        if (out_count) *out_count = plan.mips.n;
        if (out_sizes)
            for (uint32_t k = 0; k < plan.mips.n; ++k) {
                out_sizes[2 * k] = plan.mips.w[k];
                out_sizes[2 * k + 1] = plan.mips.h[k];
            }
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_present_blend_factors(const pvq_present_settings* settings, float intensity, uint32_t n_mips, float* out) {
    try {
        std::string err;
        const pvq::present::Settings s = present_settings(settings);
        if (!out || n_mips == 0 || n_mips > pvq::present::MAX_MIPS) {
            pvq::set_last_error("present blend factors: out is needed, and n_mips 1 .. 11");
            return PVQ_ERR_INVALID_ARG;
        }
        if (!pvq::present_settings_ok("present blend factors", s, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        pvq::present_blend_factors(s, intensity, n_mips, out);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_present_frame(const pvq_present_settings* settings, uint32_t width, uint32_t height, const float* image, float intensity,
                             uint8_t* out_rgba8, float* out_hdr) {
    try {
        if (!image || !out_rgba8) {
            pvq::set_last_error("present frame: image and out_rgba8 are needed");
            return PVQ_ERR_INVALID_ARG;
        }
        std::string err;
        const pvq::present::Settings raw = present_settings(settings);
        if (!pvq::stage_image_ok("present frame", width, height, 0.0f, err) || !pvq::present_settings_ok("present frame", raw, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_INVALID_ARG;
        }
        const pvq::present::Settings s = pvq::present_resolved(raw);
        pvq::PresentPlan plan;
        if (!pvq::present_plan("present frame", width, height, s.max_mip_dimension, plan, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_UNSUPPORTED;
        }
        pvq::present_frame(s, plan, width, height, image, intensity, out_rgba8, out_hdr);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_present_batch_create(int device_id, const pvq_present_settings* settings, uint32_t width, uint32_t height, pvq_present_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::PresentBatch> impl;
        const pvq_status st = pvq::PresentBatch::create(device_id, present_settings(settings), width, height, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_present_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_present_batch_destroy(pvq_present_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_present_batch_set_workspace_limit(pvq_present_batch* b, uint64_t bytes) {
    try {
        if (!b) return null_handle();
        return b->impl->set_workspace_limit(bytes);
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_present_batch_rows_device(pvq_present_batch* b, size_t n_rows, const float* d_image, const float* d_intensity, uint8_t* d_rgba8,
                                         float* d_hdr, void* stream) {
    try {
        if (!b) return null_handle();
        return b->impl->rows_device(n_rows, d_image, d_intensity, d_rgba8, d_hdr, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}

// pitchvis_train/train.py:67-99 as pitchvis_viewer/src/ml_system.rs:24-69 runs it: one row on the host, many rows on the device (note_model.hpp)
pvq_status pvq_note_model_create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights, pvq_note_model** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::NoteModel> impl;
        const pvq_status st = pvq::NoteModel::create(device_id, params, weights, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_note_model{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_note_model_destroy(pvq_note_model* m) {
    try {
        delete m;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_note_model_sizes(const pvq_note_model* m, uint32_t out4[4]) {
    try {
        if (!m || !out4) return null_handle();
        const pvq::NoteModelDims& d = m->impl->dims();
        out4[0] = d.L; out4[1] = d.o_conv; out4[2] = d.o_pool; out4[3] = d.n_features;
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_note_model_infer(const pvq_note_model* m, const float* window_host, float out_prob[128]) {
    try {
        if (!m) return null_handle();
        if (!window_host || !out_prob) {
            pvq::set_last_error("note model: null window or output");
            return PVQ_ERR_INVALID_ARG;
        }
        m->impl->infer(window_host, out_prob);   // ml_system.rs:24-69
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_note_model_rows_device(pvq_note_model* m, const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                                      const pvq_note_model_outputs* outs, void* stream) {
    try {
        if (!m) return null_handle();
        const pvq_note_model_outputs none{};
        return m->impl->rows_device(d_db, n_frames, n_streams, stride_frames, outs ? *outs : none, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_note_model_set_workspace_limit(pvq_note_model* m, uint64_t bytes) {
    try {
        if (!m) return null_handle();
        m->impl->set_workspace_limit(bytes);
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

// pitchvis_train/train.py:108-162, the optimisation step, on the device (note_trainer.hpp)
void pvq_note_trainer_hyper_default(pvq_note_trainer_hyper* h) {
    if (!h) return;
    h->lr = 1e-5;                  // train.py:111
    h->beta1 = 0.9;                // torch.optim.Adam's defaults
    h->beta2 = 0.999;
    h->eps = 1.1920928955078125e-7;   // train.py:143 torch.finfo(torch.float32).eps
    h->weight_decay = 5e-4;        // train.py:144
    h->dropout = 0.1;              // train.py:131-138
    h->seed = 0;
}
pvq_status pvq_note_trainer_create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                                   const pvq_note_trainer_hyper* hyper, uint32_t max_batch, pvq_note_trainer** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::unique_ptr<pvq::NoteTrainer> impl;
        const pvq_status st = pvq::NoteTrainer::create(device_id, params, weights, hyper, max_batch, impl);
        if (st != PVQ_OK) return st;
        *out = new pvq_note_trainer{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_note_trainer_destroy(pvq_note_trainer* t) {
    try {
        delete t;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_note_trainer_step(pvq_note_trainer* t, int mode, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx,
                                 uint32_t batch, float* d_loss, float* d_logits, void* stream) {
    try {
        if (!t) return null_handle();
        return t->impl->step(mode, d_db, d_targets, n_rows, idx, batch, d_loss, d_logits, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
uint64_t pvq_note_trainer_steps(const pvq_note_trainer* t) { return t ? t->impl->steps() : 0; }
uint64_t pvq_note_trainer_param_count(const pvq_note_trainer* t) { return t ? t->impl->n_params() : 0; }
pvq_status pvq_note_trainer_read(pvq_note_trainer* t, int what, float* out_host, size_t capacity) {
    try {
        if (!t) return null_handle();
        return t->impl->read(what, out_host, capacity);
    } catch (...) { return translate_exception(); }
}
// train.py:164-198, the test pass
pvq_status pvq_note_trainer_test(pvq_note_trainer* t, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx,
                                 uint32_t batch, pvq_note_test_batch* out_batches, uint32_t* out_pitch, float* d_logits, void* stream) {
    try {
        if (!t) return null_handle();
        return t->impl->test(d_db, d_targets, n_rows, idx, n_idx, batch, out_batches, out_pitch, d_logits, static_cast<hipStream_t>(stream));
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_note_test_metrics(const pvq_note_test_batch* b, size_t n_batches, double* mean_f1, double* accuracy, double* mean_loss) {
    try {
        std::string err;
        const pvq_status st = pvq::note_test_metrics(b, n_batches, mean_f1, accuracy, mean_loss, err);
        if (st != PVQ_OK) pvq::set_last_error(err);
        return st;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_note_trainer_dropout_keep(uint64_t seed, uint64_t step, uint32_t layer, uint32_t row, uint32_t col0, uint32_t n, double dropout,
                                         uint8_t* out_keep) {
    try {
        if (!out_keep || !(dropout >= 0.0 && dropout < 1.0)) {
            pvq::set_last_error("note trainer: out_keep is null or dropout lies outside [0, 1)");
            return PVQ_ERR_INVALID_ARG;
        }
        const uint64_t key = pvq::nt_layer_key(seed, step, layer);
        const uint32_t threshold = pvq::nt_keep_threshold(dropout);
        for (uint32_t j = 0; j < n; ++j) out_keep[j] = pvq::nt_keep(key, row, col0 + j, threshold) ? 1 : 0;
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}

// The synthesizer (rustysynth_fork, dry path): the bank, one stream on the host (synth_host.hpp) and many on the device
// (synth_batch.hpp)
namespace {
static_assert(sizeof(pvq_synth_record) == sizeof(pvq::synth::Record), "one layout");
pvq_status synth_snapshots_out(const pvq::SynthPlan& p, uint32_t* out_counts, uint32_t* voice_ptr, size_t ptr_capacity, int32_t* key, float* gain_left,
                               float* gain_right, size_t capacity) {
    const size_t n_snap = p.snapshot_ptr.empty() ? 0 : p.snapshot_ptr.size() - 1, n_voices = p.snapshots.size();
    if (out_counts) {
        out_counts[0] = static_cast<uint32_t>(n_snap);
        out_counts[1] = static_cast<uint32_t>(n_voices);
    }
    if (!voice_ptr && !key && !gain_left && !gain_right) return PVQ_OK;
    if (!voice_ptr || !key || !gain_left || !gain_right || ptr_capacity < n_snap + 1 || capacity < n_voices) {
        pvq::set_last_error("synth snapshots: all four arrays are needed, voice_ptr of snapshots + 1 and the others of as many entries as there are voices");
        return PVQ_ERR_INVALID_ARG;
    }
    for (size_t k = 0; k <= n_snap; ++k) voice_ptr[k] = p.snapshot_ptr.empty() ? 0u : p.snapshot_ptr[k];
    for (size_t k = 0; k < n_voices; ++k) {
        key[k] = p.snapshots[k].key;
        gain_left[k] = p.snapshots[k].current_mix_gain_left;
        gain_right[k] = p.snapshots[k].current_mix_gain_right;
    }
    return PVQ_OK;
}
}  // namespace
pvq_status pvq_synth_bank_create(const int16_t* wave_data, size_t n_wave, const int32_t* samples, uint32_t n_samples, const int16_t* instrument_gs,
                                 const uint32_t* instrument_sample, uint32_t n_instrument_regions, const uint32_t* instruments, uint32_t n_instruments,
                                 const int16_t* preset_gs, const uint32_t* preset_instrument, uint32_t n_preset_regions, const int32_t* presets,
                                 uint32_t n_presets, pvq_synth_bank** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        std::shared_ptr<const pvq::SynthBank> impl;
        std::string err;
        const pvq_status st = pvq::SynthBank::create(wave_data, n_wave, samples, n_samples, instrument_gs, instrument_sample, n_instrument_regions,
                                                     instruments, n_instruments, preset_gs, preset_instrument, n_preset_regions, presets, n_presets, impl,
                                                     err);   // soundfont.rs, instrument_region.rs:33-87, preset_region.rs:26-53
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        *out = new pvq_synth_bank{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_synth_bank_destroy(pvq_synth_bank* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_synth_bank_counts(const pvq_synth_bank* b, uint64_t* out4) {
    try {
        if (!b || !out4) return null_handle();
        out4[0] = b->impl->wave.size();
        out4[1] = b->impl->iregions.size();
        out4[2] = b->impl->pregions.size();
        out4[3] = b->impl->presets.size();
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_synth_state_create(const pvq_synth_bank* bank, int32_t sample_rate, uint32_t maximum_polyphony, pvq_synth_state** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        if (!bank) return null_handle();
        std::unique_ptr<pvq::SynthState> impl;
        std::string err;
        const pvq_status st = pvq::SynthState::create(bank->impl, sample_rate, maximum_polyphony, impl, err);   // synthesizer.rs:58-174
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        *out = new pvq_synth_state{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_synth_state_destroy(pvq_synth_state* s) {
    try {
        delete s;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_synth_state_render(pvq_synth_state* s, const double* time_s, const int32_t* channel, const int32_t* command, const int32_t* data1,
                                  const int32_t* data2, size_t n_events, size_t n_blocks, const uint32_t* snapshot_blocks, size_t n_snapshots, float* left,
                                  float* right) {
    try {
        if (!s) return null_handle();
        std::string err;
        const pvq::SynthEvents ev{time_s, channel, command, data1, data2, n_events};
        const pvq_status st = s->impl->render(ev, n_blocks, snapshot_blocks, n_snapshots, left, right, err);   // midifile_sequencer.rs:52-104
        if (st != PVQ_OK) pvq::set_last_error(err);
        return st;
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_synth_state_get_snapshots(const pvq_synth_state* s, uint32_t* out_counts, uint32_t* voice_ptr, size_t ptr_capacity, int32_t* key,
                                         float* gain_left, float* gain_right, size_t capacity) {
    try {
        if (!s) return null_handle();
        return synth_snapshots_out(s->impl->last_plan(), out_counts, voice_ptr, ptr_capacity, key, gain_left, gain_right, capacity);   // synthesizer.rs:525
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_synth_state_get_plan(const pvq_synth_state* s, uint32_t* out_counts, uint32_t* block_ptr, size_t ptr_capacity, pvq_synth_record* records,
                                    size_t capacity) {
    try {
        if (!s) return null_handle();
        const pvq::SynthPlan& p = s->impl->last_plan();
        const size_t n_blocks = p.block_ptr.empty() ? 0 : p.block_ptr.size() - 1, n_records = p.records.size();
        if (out_counts) {
            out_counts[0] = static_cast<uint32_t>(n_blocks);
            out_counts[1] = static_cast<uint32_t>(n_records);
        }
        if (!block_ptr && !records) return PVQ_OK;
        if (!block_ptr || !records || ptr_capacity < n_blocks + 1 || capacity < n_records) {
            pvq::set_last_error("synth plan: block_ptr of blocks + 1 entries and records of as many as the plan holds are needed");
            return PVQ_ERR_INVALID_ARG;
        }
        for (size_t k = 0; k <= n_blocks; ++k) block_ptr[k] = p.block_ptr.empty() ? 0u : p.block_ptr[k];
        if (n_records) std::memcpy(records, p.records.data(), n_records * sizeof(pvq_synth_record));
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
uint32_t pvq_synth_state_active_voices(const pvq_synth_state* s) {
    try {
        return s ? s->impl->active_voice_count() : 0;   // voice_collection.rs:11
    } catch (...) { (void)translate_exception(); return 0; }
}
pvq_status pvq_synth_batch_create(int device_id, const pvq_synth_bank* bank, uint32_t n_streams, int32_t sample_rate, uint32_t maximum_polyphony,
                                  pvq_synth_batch** out) {
    try {
        if (!out) return null_handle();
        *out = nullptr;
        if (!bank) return null_handle();
        std::unique_ptr<pvq::SynthBatch> impl;
        const pvq_status st = pvq::SynthBatch::create(device_id, bank->impl, n_streams, sample_rate, maximum_polyphony, impl);   // synthesizer.rs:58-174
        if (st != PVQ_OK) return st;
        *out = new pvq_synth_batch{std::move(impl)};
        return PVQ_OK;
    } catch (...) { return translate_exception(); }
}
void pvq_synth_batch_destroy(pvq_synth_batch* b) {
    try {
        delete b;
    } catch (...) { (void)translate_exception(); }
}
pvq_status pvq_synth_batch_render_device(pvq_synth_batch* b, const uint64_t* event_ptr, const double* time_s, const int32_t* channel,
                                         const int32_t* command, const int32_t* data1, const int32_t* data2, const size_t* n_blocks, float* const* d_left,
                                         float* const* d_right, const uint32_t* snapshot_blocks, size_t n_snapshots, void* stream) {
    try {
        if (!b) return null_handle();
        if (!event_ptr) {
            pvq::set_last_error("synth batch: event_ptr is needed");
            return PVQ_ERR_INVALID_ARG;
        }
        const uint32_t n = b->impl->n_streams();
        std::vector<pvq::SynthEvents> ev(n);
        for (uint32_t s = 0; s < n; ++s) {
            const uint64_t e0 = event_ptr[s], e1 = event_ptr[s + 1];
            if (e1 < e0 || (e1 > e0 && !(time_s && channel && command && data1 && data2))) {
                pvq::set_last_error("synth batch: event_ptr must ascend, and the event arrays are needed where it names events");
                return PVQ_ERR_INVALID_ARG;
            }
            if (e1 > e0) ev[s] = pvq::SynthEvents{time_s + e0, channel + e0, command + e0, data1 + e0, data2 + e0, static_cast<size_t>(e1 - e0)};
        }
        return b->impl->render_device(ev.data(), n_blocks, d_left, d_right, snapshot_blocks, n_snapshots,
                                      static_cast<hipStream_t>(stream));   // midifile_sequencer.rs:52-104 for every stream
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_synth_batch_last_times(pvq_synth_batch* b, float* out_ms4, uint64_t* out_records) {
    try {
        if (!b) return null_handle();
        return b->impl->last_times(out_ms4, out_records);
    } catch (...) { return translate_exception(); }
}
pvq_status pvq_synth_batch_get_snapshots(const pvq_synth_batch* b, uint32_t stream_index, uint32_t* out_counts, uint32_t* voice_ptr, size_t ptr_capacity,
                                         int32_t* key, float* gain_left, float* gain_right, size_t capacity) {
    try {
        if (!b) return null_handle();
        const pvq::SynthPlan* p = b->impl->plan_of(stream_index);
        if (!p) {
            pvq::set_last_error("synth batch: stream_index is 0 .. n_streams - 1");
            return PVQ_ERR_INVALID_ARG;
        }
        return synth_snapshots_out(*p, out_counts, voice_ptr, ptr_capacity, key, gain_left, gain_right, capacity);   // synthesizer.rs:525
    } catch (...) { return translate_exception(); }
}

}  // extern "C"
