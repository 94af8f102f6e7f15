// capi_vqt.cpp — extern "C" surface of libpvq (include/pvq.h): status / last error / ABI version, the transform handle and its
// getters, algo / precision / workspace, batch, streams, multi-device, pvq_plan_shard, profiling.
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_support.hpp"
#include "multi_host.hpp"
#include "vqt_engine.hpp"

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
pvq_vqt_params to_c(const pvq::VqtParameters& d) {
    pvq_vqt_params p;
    p.sr = d.sr;
    p.n_fft = d.n_fft;
    p.min_freq = d.range.min_freq;
    p.octaves = d.range.octaves;
    p.buckets_per_octave = d.range.buckets_per_octave;
    p.sparsity_quantile = d.sparsity_quantile;
    p.quality = d.quality;
    p.gamma = d.gamma;
    return p;
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
}  // namespace

extern "C" {

const char* pvq_status_string(pvq_status s) {
    return guarded(nullptr, [&]() -> const char* {
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
    });
}

const char* pvq_last_error(void) {
    return guarded(nullptr, [&] {
        return pvq::get_last_error();
    });
}
uint32_t pvq_abi_version(void) {
    return guarded(0, [&] {
        return PVQ_ABI_VERSION;
    });
}

void pvq_vqt_default_params(pvq_vqt_params* p) {
    guarded([&] {
        if (!p) return;
        *p = to_c(pvq::VqtParameters{});
    });
}

pvq_status pvq_vqt_create(const pvq_vqt_params* params, int device_id, pvq_vqt** out, float err_detail[2]) {
    return guarded([&] {
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
    });
}

void pvq_vqt_destroy(pvq_vqt* v) { destroy(v); }

void pvq_vqt_get_params(const pvq_vqt* v, pvq_vqt_params* out) {
    guarded([&] {
        if (!v || !out) return;
        *out = to_c(v->impl->params());
    });
}

uint32_t pvq_vqt_n_bins(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? v->impl->n_bins() : 0;
    });
}
double pvq_vqt_delay_seconds(const pvq_vqt* v) {
    return guarded(0.0, [&] {
        return v ? v->impl->delay_seconds() : 0.0;
    });
}
uint32_t pvq_vqt_window_union(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? v->impl->plan().window_union : 0;
    });
}
pvq_status pvq_vqt_bandwidths_3db(const pvq_vqt* v, float* lo_hz, float* hi_hz) {
    return guarded([&] {
        if (!v || !lo_hz || !hi_hz) return null_handle();
        const pvq::HostPlan& pl = v->impl->plan();
        std::copy(pl.bandwidth_lo_hz.begin(), pl.bandwidth_lo_hz.end(), lo_hz);
        std::copy(pl.bandwidth_hi_hz.begin(), pl.bandwidth_hi_hz.end(), hi_hz);
        return PVQ_OK;
    });
}
uint32_t pvq_vqt_warning_count(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? (uint32_t)v->impl->plan().warnings.size() : 0;
    });
}
pvq_status pvq_vqt_warning(const pvq_vqt* v, uint32_t i, char* buf, size_t cap) {
    return guarded([&] {
        if (!v || !buf || cap == 0) return null_handle();
        const pvq::HostPlan& pl = v->impl->plan();
        if (i >= pl.warnings.size()) return invalid_arg("warning index out of range");
        const std::string& w = pl.warnings[i];
        const size_t nb = std::min(cap - 1, w.size());
        std::memcpy(buf, w.data(), nb);
        buf[nb] = '\0';
        return PVQ_OK;
    });
}
uint32_t pvq_vqt_n_groups(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? static_cast<uint32_t>(v->impl->kernel().window_groups.size()) : 0;
    });
}

pvq_status pvq_vqt_group_info(const pvq_vqt* v, uint32_t g, uint32_t info[5]) {
    return guarded([&] {
        if (!v || !info) return null_handle();
        const auto& groups = v->impl->kernel().window_groups;
        if (g >= groups.size()) return invalid_arg("group index out of range");
        info[0] = groups[g].window_begin;
        info[1] = groups[g].window_end;
        info[2] = groups[g].filter_bank.rows;
        info[3] = groups[g].filter_bank.nnz();
        info[4] = groups[g].negative_filter_bank.nnz();
        return PVQ_OK;
    });
}

pvq_status pvq_vqt_group_csr(const pvq_vqt* v, uint32_t g, int negative, uint32_t* row_ptr, uint32_t* col_idx,
                             float* values) {
    return guarded([&] {
        if (!v || !row_ptr || !col_idx || !values) return null_handle();
        const auto& groups = v->impl->kernel().window_groups;
        if (g >= groups.size()) return invalid_arg("group index out of range");
        const pvq::CsrMatrix& m = negative ? groups[g].negative_filter_bank : groups[g].filter_bank;
        std::memcpy(row_ptr, m.row_ptr.data(), sizeof(uint32_t) * m.row_ptr.size());
        std::memcpy(col_idx, m.col_idx.data(), sizeof(uint32_t) * m.col_idx.size());
        std::memcpy(values, m.values.data(), sizeof(pvq::cf32) * m.values.size());
        return PVQ_OK;
    });
}

pvq_status pvq_vqt_filter_params(const pvq_vqt* v, float* freq, float* window_length, uint32_t* factor,
                                 uint32_t* minwin) {
    return guarded([&] {
        if (!v) return null_handle();
        const auto& f = v->impl->plan().filters;
        for (size_t k = 0; k < f.size(); ++k) {
            if (freq) freq[k] = f[k].freq;
            if (window_length) window_length[k] = f[k].window_length;
            if (factor) factor[k] = f[k].sr_downscaling_factor;
            if (minwin) minwin[k] = f[k].minimum_needed_window_size;
        }
        return PVQ_OK;
    });
}

pvq_status pvq_vqt_calculate_instant_db(pvq_vqt* v, const float* x, size_t len, float* out_db) {
    return guarded([&] {
        if (!v) return null_handle();
        if (!x || !out_db) return invalid_arg("null pointer");
        return v->impl->calculate_vqt_instant_in_db(x, len, out_db);
    });
}

pvq_status pvq_vqt_calculate_batch_db(pvq_vqt* v, const float* pcm, size_t n_lead, size_t hop, size_t n_frames,
                                      float* out_db) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->calculate_batch_db(pcm, n_lead, hop, n_frames, out_db);
    });
}

pvq_status pvq_vqt_calculate_batch_db_device(pvq_vqt* v, const float* d_pcm, size_t n_lead, size_t hop,
                                             size_t n_frames, float* d_out_db, float* d_out_cplx, void* stream) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->calculate_batch_db_device(d_pcm, n_lead, hop, n_frames, d_out_db, d_out_cplx,
                                                  static_cast<hipStream_t>(stream));
    });
}

pvq_status pvq_vqt_set_algo(pvq_vqt* v, pvq_algo algo) {
    return guarded([&] {
        if (!v) return null_handle();
        if (algo != PVQ_ALGO_AUTO && algo != PVQ_ALGO_FFT && algo != PVQ_ALGO_BLOCKDFT) return invalid_arg("unknown algorithm");
        v->impl->set_algo(algo);
        return PVQ_OK;
    });
}
pvq_algo pvq_vqt_last_algo(const pvq_vqt* v) {
    return guarded(PVQ_ALGO_AUTO, [&] {
        return v ? v->impl->last_algo() : PVQ_ALGO_AUTO;
    });
}
pvq_algo pvq_vqt_resolve_algo(pvq_vqt* v, size_t hop, size_t n_frames) {
    return guarded(PVQ_ALGO_AUTO, [&]() -> pvq_algo {
        if (!v || hop == 0) return PVQ_ALGO_AUTO;
        return v->impl->resolve_algo(hop, n_frames);
    });
}

pvq_status pvq_vqt_set_twiddle_fp16(pvq_vqt* v, int enable) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->set_twiddle_fp16(enable != 0);
    });
}

pvq_status pvq_vqt_set_workspace_limit(pvq_vqt* v, uint64_t bytes) {
    return guarded([&] {
        if (!v) return null_handle();
        v->impl->set_workspace_limit((size_t)bytes);
        return PVQ_OK;
    });
}

uint32_t pvq_vqt_blockdft_columns(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? v->impl->blockdft_columns() : 0;
    });
}

pvq_status pvq_vqt_set_gemm_precision(pvq_vqt* v, pvq_gemm_precision p) {
    return guarded([&] {
        if (!v) return null_handle();
        if (p != PVQ_GEMM_F32 && p != PVQ_GEMM_BF16X3) return invalid_arg("unknown GEMM precision");
        v->impl->set_gemm_split_bf16(p == PVQ_GEMM_BF16X3);
        return PVQ_OK;
    });
}

void pvq_analysis_default_params(pvq_analysis_params* a) {
    guarded([&] {
        if (!a) return;
        const pvq::AnalysisParameters d;
        a->peak_min_prominence = d.peak_min_prominence;
        a->peak_min_height = d.peak_min_height;
        a->bass_min_prominence = d.bass_min_prominence;
        a->bass_min_height = d.bass_min_height;
        a->highest_bassnote = d.highest_bassnote;
        a->harmonic_threshold = d.harmonic_threshold;
    });
}

pvq_status pvq_analyze_batch_device(pvq_vqt* v, const float* d_db, size_t n_frames, const pvq_analysis_params* a,
                                    uint32_t* d_peak_mask, uint32_t* d_peak_count, float* d_center, float* d_size,
                                    uint32_t max_peaks, void* stream) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->analyze_batch_device(d_db, n_frames, to_cpp(a), d_peak_mask, d_peak_count, d_center, d_size,
                                             max_peaks, static_cast<hipStream_t>(stream));
    });
}

pvq_status pvq_analyze_batch(pvq_vqt* v, const float* db, size_t n_frames, const pvq_analysis_params* a,
                             uint32_t* peak_mask, uint32_t* peak_count, float* center, float* size,
                             uint32_t max_peaks) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->analyze_batch(db, n_frames, to_cpp(a), peak_mask, peak_count, center, size, max_peaks);
    });
}

pvq_status pvq_vqt_analyze_batch_device(pvq_vqt* v, const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames,
                                        const pvq_analysis_params* a, float* d_out_db, uint32_t* d_peak_mask,
                                        uint32_t* d_peak_count, float* d_center, float* d_size, uint32_t max_peaks,
                                        void* stream) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->vqt_analyze_batch_device(d_pcm, n_lead, hop, n_frames, to_cpp(a), d_out_db, d_peak_mask,
                                                 d_peak_count, d_center, d_size, max_peaks,
                                                 static_cast<hipStream_t>(stream));
    });
}

pvq_status pvq_vqt_calculate_batch_db_streams(pvq_vqt* v, const float* const* d_pcm, const size_t* n_lead, const size_t* n_frames,
                                              uint32_t n_streams, size_t hop, float* d_out_db, size_t out_stride_frames, void* stream) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->batch_streams_device(d_pcm, n_lead, n_frames, n_streams, hop, d_out_db, out_stride_frames, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, 0, static_cast<hipStream_t>(stream));
    });
}

pvq_status pvq_vqt_analyze_batch_streams(pvq_vqt* v, const float* const* d_pcm, const size_t* n_lead, const size_t* n_frames,
                                         uint32_t n_streams, size_t hop, const pvq_analysis_params* a, float* d_out_db,
                                         size_t out_stride_frames, uint32_t* d_peak_mask, uint32_t* d_peak_count, float* d_center,
                                         float* d_size, uint32_t max_peaks, void* stream) {
    return guarded([&] {
        if (!v) return null_handle();
        const pvq::AnalysisParameters ap = to_cpp(a);
        return v->impl->batch_streams_device(d_pcm, n_lead, n_frames, n_streams, hop, d_out_db, out_stride_frames, &ap, d_peak_mask,
                                             d_peak_count, d_center, d_size, max_peaks, static_cast<hipStream_t>(stream));
    });
}

pvq_status pvq_plan_shard(uint64_t n_frames_total, uint64_t hop, uint64_t window_union, uint32_t rank, uint32_t world, pvq_shard* out) {
    return guarded([&] {
        pvq::ShardPlan sp;
        if (!out || !pvq::plan_shard(n_frames_total, hop, window_union, rank, world, &sp))
            return invalid_arg("pvq_plan_shard: null output or rank >= world");
        out->first_frame = sp.first_frame;
        out->n_frames = sp.n_frames;
        out->sample_begin = sp.sample_begin;
        out->sample_end = sp.sample_end;
        out->n_lead = sp.n_lead;
        return PVQ_OK;
    });
}

pvq_status pvq_vqt_analyze_batch_multi(pvq_vqt* const* handles, uint32_t n_handles, const float* pcm, size_t n_lead, size_t hop,
                                       size_t n_frames, const pvq_analysis_params* a, float* out_db, uint32_t* peak_mask,
                                       uint32_t* peak_count, float* center, float* size, uint32_t max_peaks) {
    return guarded([&] {
        if (!handles || n_handles == 0) return null_handle();
        std::vector<pvq::Vqt*> hs(n_handles, nullptr);
        for (uint32_t i = 0; i < n_handles; ++i) {
            if (!handles[i]) return null_handle();
            hs[i] = handles[i]->impl.get();
        }
        return pvq::analyze_batch_multi(hs.data(), n_handles, pcm, n_lead, hop, n_frames, to_cpp(a), out_db, peak_mask, peak_count,
                                        center, size, max_peaks);
    });
}

pvq_status pvq_vqt_set_profiling(pvq_vqt* v, int enable) {
    return guarded([&] {
        if (!v) return null_handle();
        v->impl->set_profiling(enable == 2 ? 2 : (enable != 0 ? 1 : 0));
        return PVQ_OK;
    });
}
uint32_t pvq_vqt_last_kernel_ms(pvq_vqt* v, float* out_ms, uint32_t capacity) {
    return guarded(0, [&]() -> uint32_t {
        if (!v || !out_ms) return 0;
        return v->impl->last_kernel_ms(out_ms, capacity);
    });
}
uint32_t pvq_vqt_last_kernel_launches(pvq_vqt* v, uint32_t* out_n, uint32_t capacity) {
    return guarded(0, [&]() -> uint32_t {
        if (!v || !out_n) return 0;
        return v->impl->last_kernel_launches(out_n, capacity);
    });
}
pvq_status pvq_vqt_input_status(pvq_vqt* v, void* stream) {
    return guarded([&] {
        if (!v) return null_handle();
        return v->impl->input_status(static_cast<hipStream_t>(stream));
    });
}
double pvq_vqt_last_gemm_flop(const pvq_vqt* v) {
    return guarded(0.0, [&] {
        return v ? v->impl->last_gemm_flop() : 0.0;
    });
}
float pvq_vqt_last_sclk_mhz(pvq_vqt* v) {
    return guarded(0.0f, [&] {
        return v ? v->impl->last_sclk_mhz() : 0.0f;
    });
}
uint32_t pvq_vqt_last_frames_per_launch(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? v->impl->last_frames_per_launch() : 0;
    });
}
const char* pvq_vqt_kernel_name(uint32_t slot) {
    return guarded(nullptr, [&] {
        return pvq::Vqt::slot_name(slot);
    });
}

}  // extern "C"
