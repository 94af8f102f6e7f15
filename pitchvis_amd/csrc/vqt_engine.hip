// vqt_engine.hip — the pvq::Vqt handle: create and destroy, device tables, profiling slots, the ordering of a handle's calls, the
// route decision of a batch (FFT path or block-DFT path), many streams in one call with their staging, the host-buffer wrappers and
// the single-frame call.
//
// One kernel: stage_streams (the copy kernel of the stream staging).  The paths a call is routed to live in their own units:
//   fft_path.hip       the FFT path: vqt_fft_frames, vqt_fft_group, db_rows, db_rows_batch and their launchers (fft_path.hpp)
//   peaks_frames.hip   peaks_frames_lean, peaks_frames_generic, launch_peaks_frames, Vqt::peaks_stage, Vqt::make_peak_params
//   vqt_blockdft.hip   the block-DFT path (with blockdft_gemm.hip, blockdft_dots.hip)
//   multi_batch.hip    analyze_batch_multi, the multi-device driver
#include "vqt_engine.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "device_tables.hpp"
#include "fft_path.hpp"
#include "peaks_device.hpp"

// (kept from before the FFT path and the peak kernels left this unit: no host float expression here rounds differently than it did)
#pragma clang fp contract(off)

namespace pvq {

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
void set_last_error_noexcept(const char* s) noexcept {
    try {
        g_last_error = s ? s : "";
    } catch (...) {
        g_last_error.clear();
    }
}
const char* get_last_error() { return g_last_error.c_str(); }

const char* Vqt::slot_name(uint32_t s) {
    switch (s) {
        case SLOT_FFT_FRAMES: return "vqt_fft_frames";
        case SLOT_BLOCKDFT_GEMM: return "blockdft_gemm";
        case SLOT_BLOCKDFT_COMBINE: return "blockdft_combine";
        case SLOT_BLOCKDFT_DOTS: return "blockdft_dots_db";
        case SLOT_PEAKS: return "peaks_frames";
        default: return "";
    }
}

pvq_status Vqt::require_device() const {
    if (has_device()) return PVQ_OK;
    set_last_error("handle was created without a device; there is no CPU fallback");
    return PVQ_ERR_NO_DEVICE;
}

pvq_status Vqt::create(const VqtParameters& p, int device_id, std::unique_ptr<Vqt>& out, VqtError& err) {
    if (p.range.octaves == 0 || p.range.buckets_per_octave == 0 || p.n_fft < 4 || (p.n_fft & (p.n_fft - 1)) != 0 ||
        !(p.sr > 0.0f) || !(p.range.min_freq > 0.0f)) {
        set_last_error("invalid VqtParameters (n_fft must be a power of two, sr/min_freq/octaves/buckets > 0)");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<Vqt> v(new Vqt());
    err = build_plan(p, v->plan_);
    if (err.kind == VqtError::AboveNyquist) {
        set_last_error(err.to_string());
        return PVQ_ERR_ABOVE_NYQUIST;
    }
    if (err.kind == VqtError::WindowExceedsNFft) {
        set_last_error(err.to_string());
        return PVQ_ERR_WINDOW_EXCEEDS_NFFT;
    }
    v->device_id_ = device_id;
    if (device_id >= 0) {
        int n_dev = 0;
        hipError_t e = hipGetDeviceCount(&n_dev);
        if (e != hipSuccess || device_id >= n_dev) {
            set_last_error("no such HIP device (hipGetDeviceCount: " + std::string(hipGetErrorString(e)) + ")");
            return PVQ_ERR_DEVICE;
        }
        PVQ_HIP(hipSetDevice(device_id));
        pvq_status st = v->upload_tables();
        if (st != PVQ_OK) return st;
    }
    out = std::move(v);
    return PVQ_OK;
}

Vqt::~Vqt() {
    if (device_id_ >= 0) {
        (void)hipSetDevice(device_id_);
        if (dev_) {
            free_device_tables(dev_);
            dev_ = nullptr;
        }
        if (multi_stream_) (void)hipStreamDestroy(multi_stream_);
        if (host_streams_ready_)
            for (int i = 0; i < 3; ++i) (void)hipStreamDestroy(host_streams_[i]);
        for (hipEvent_t e : host_events_) (void)hipEventDestroy(e);
        if (inst_stream_) (void)hipStreamDestroy(inst_stream_);
        if (order_ev_) (void)hipEventDestroy(order_ev_);
        if (inst_pin_) (void)hipHostFree(inst_pin_);
        for (int s = 0; s < N_SLOTS; ++s)
            for (int k = 0; k < 2; ++k)
                for (hipEvent_t e : ev_[s][k]) (void)hipEventDestroy(e);
    }
    // (the workspaces and shard buffers go after this body, with their device set)
}

pvq_status Vqt::set_twiddle_fp16(bool on) {
    if (on == twiddle_fp16_) return PVQ_OK;
    twiddle_fp16_ = on;
    if (device_id_ < 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    if (dev_) {
        free_device_tables(dev_);   // frees the block-DFT tables too; they are rebuilt on the next batch call
        dev_ = nullptr;
    }
    return upload_tables();
}

pvq_status Vqt::upload_tables() {
    std::string msg;
    dev_ = build_device_tables(plan_, twiddle_fp16_, msg);
    if (!dev_) {
        set_last_error(msg);
        return msg.rfind("unsupported", 0) == 0 ? PVQ_ERR_UNSUPPORTED : PVQ_ERR_DEVICE;
    }
    return PVQ_OK;
}

void Vqt::set_profiling(int mode) {
    profiling_ = mode != 0;
    profiling_main_only_ = mode == 2;
    for (int s = 0; s < N_SLOTS; ++s) ev_count_[s] = 0;
}

void Vqt::slot_begin(int slot, hipStream_t s) {
    if (profiling_main_only_ && slot != SLOT_BLOCKDFT_GEMM && slot != SLOT_FFT_FRAMES) return;
    if (!profiling_ || ev_count_[slot] >= kMaxTimedLaunches) return;
    const int i = ev_count_[slot];
    if ((int)ev_[slot][0].size() <= i) {
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        ev_[slot][0].push_back(a);
        ev_[slot][1].push_back(b);
    }
    (void)hipEventRecord(ev_[slot][0][i], s);
}
void Vqt::slot_end(int slot, hipStream_t s) {
    if (profiling_main_only_ && slot != SLOT_BLOCKDFT_GEMM && slot != SLOT_FFT_FRAMES) return;
    if (!profiling_ || ev_count_[slot] >= kMaxTimedLaunches) return;
    (void)hipEventRecord(ev_[slot][1][ev_count_[slot]], s);
    ++ev_count_[slot];
}

uint32_t Vqt::last_kernel_ms(float* out, uint32_t cap) {
    uint32_t n = 0;
    for (int s = 0; s < N_SLOTS && (uint32_t)s < cap; ++s) {
        out[s] = -1.0f;
        double sum = 0.0;
        int ok = 0;
        for (int i = 0; i < ev_count_[s]; ++i) {
            if (hipEventSynchronize(ev_[s][1][i]) != hipSuccess) continue;
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev_[s][0][i], ev_[s][1][i]) == hipSuccess) {
                sum += ms;
                ++ok;
            }
        }
        if (ok) out[s] = (float)(sum / ok);
        n = s + 1;
    }
    return n;
}

uint32_t Vqt::last_kernel_launches(uint32_t* out, uint32_t cap) const {
    uint32_t n = 0;
    for (int s = 0; s < N_SLOTS && (uint32_t)s < cap; ++s) {
        out[s] = (uint32_t)ev_count_[s];
        n = s + 1;
    }
    return n;
}

pvq_status Vqt::calculate_batch_db_device(const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames,
                                          float* d_out_db, float* d_out_cplx, hipStream_t stream) {
    return run_batch(d_pcm, n_lead, hop, n_frames, d_out_db, d_out_cplx, nullptr, stream);
}

pvq_status Vqt::vqt_analyze_batch_device(const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames,
                                         const AnalysisParameters& ap, float* d_out_db, uint32_t* d_peak_mask,
                                         uint32_t* d_peak_count, float* d_center, float* d_size, uint32_t max_peaks,
                                         hipStream_t stream) {
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if ((d_center == nullptr) != (d_size == nullptr)) {
        set_last_error("analyze: only one of center/size given");
        return PVQ_ERR_INVALID_ARG;
    }
    PeakParamsDev pk;
    if (!make_peak_params(ap, d_peak_mask, d_peak_count, d_center, d_size, max_peaks, pk)) {
        set_last_error("unsupported: peak detection handles 3..1024 bins per frame");
        return PVQ_ERR_UNSUPPORTED;
    }
    return run_batch(d_pcm, n_lead, hop, n_frames, d_out_db, nullptr, &pk, stream);
}

pvq_status Vqt::order_on(hipStream_t s) {
    if (order_valid_ && order_stream_ != s) {
        if (!order_ev_) PVQ_HIP(hipEventCreateWithFlags(&order_ev_, hipEventDisableTiming));
        // a marker behind everything the previous call queued; should its stream be gone (destroyed by the caller: an invalid
        // handle), a stream that no longer exists has nothing in flight that a device-wide wait would not cover
        if (hipEventRecord(order_ev_, order_stream_) == hipSuccess) {
            PVQ_HIP(hipStreamWaitEvent(s, order_ev_, 0));
        } else {
            (void)hipGetLastError();
            PVQ_HIP(hipDeviceSynchronize());
        }
    }
    order_stream_ = s;
    order_valid_ = true;
    return PVQ_OK;
}

static const char kNoBlockHop[] =
    "block-DFT path: no multiple r * hop (r = 1, 2, 4, 8, 16) is a multiple of 64 samples that the windows hold at most 16 times "
    "(or a power of two dividing every window)";
static const char kNonFiniteInput[] =
    "non-finite sample (NaN / Inf) in the input: the affected frames are unspecified (the reference's audio "
    "callback drops such chunks, audio_desktop.rs:102-105; peak_detection.rs:145 would panic)";

pvq_status Vqt::run_batch(const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames, float* d_out_db,
                          float* d_out_cplx, const PeakParamsDev* pk, hipStream_t stream) {
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if (n_frames == 0) return PVQ_OK;
    if (!d_pcm || !d_out_db || hop == 0 || n_frames > (size_t)0x7fffffff) {
        set_last_error("calculate_batch: null pointer, zero hop or too many frames");
        return PVQ_ERR_INVALID_ARG;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    {
        pvq_status os = order_on(stream);
        if (os != PVQ_OK) return os;
    }
    // The block-DFT path takes the hop itself (r = 1), or — a hop it cannot take but whose r-fold it can, 800 -> 1 600 — r interleaved
    // block grids of hop r * hop: grid i holds the frames i, i + r, ... (each hop' block is then transformed once per grid)
    size_t r = 0;
    switch (route(hop, n_frames, &r)) {
        case BatchRoute::Fft: return launch_fft_path(d_pcm, n_lead, hop, n_frames, d_out_db, d_out_cplx, pk, stream);
        case BatchRoute::RefuseNoHop: set_last_error(kNoBlockHop); return PVQ_ERR_UNSUPPORTED;
        case BatchRoute::RefuseUnfusedHop:
            set_last_error("block-DFT path: this geometry runs the unfused stages, which take the hop only as it is");
            return PVQ_ERR_UNSUPPORTED;
        case BatchRoute::BlockStreams:
        case BatchRoute::BlockPerStream: break;
    }
    if (r == 1) return launch_blockdft_path(d_pcm, n_lead, hop, n_frames, d_out_db, d_out_cplx, pk, stream);
    std::vector<StreamRun> st;
    append_interleaved_runs(st, d_pcm, n_lead, n_frames, hop, r, 0);
    return launch_blockdft_streams(st.data(), st.size(), hop * r, d_out_db, d_out_cplx, n_frames, pk, stream);
}

// The one route decision (route_batch, batch_plan.hpp) under the handle's settings, for a call of n_frames frames in all.
BatchRoute Vqt::route(size_t hop, size_t n_frames, size_t* r_out) const {
    const size_t r = *r_out = blockdft_hop_factor(hop);
    return route_batch(algo_, r, r != 0 && blockdft_takes_streams(hop * r), n_frames,
                       algo_ == PVQ_ALGO_AUTO && r != 0 ? auto_block_min_frames(plan_, hop, r) : 0);
}

// which path run_batch takes for a batch of this shape (the multi-device driver decides once for the WHOLE stream, so that a shard of a
// few frames runs the path the unsharded stream runs: the two paths agree to the parity bars, not bit for bit)
pvq_algo Vqt::resolve_algo(size_t hop, size_t n_frames) const {
    size_t r = 0;
    return route(hop, n_frames, &r) == BatchRoute::Fft ? PVQ_ALGO_FFT : PVQ_ALGO_BLOCKDFT;   // (a refusal: forced, the run functions report the error)
}

size_t Vqt::blockdft_hop_factor(size_t hop) const {
    for (size_t r = 1; r <= 16; r *= 2)
        if (blockdft_applicable(hop * r)) return r;
    return 0;
}

pvq_status Vqt::batch_streams_device(const float* const* d_pcm, const size_t* n_lead, const size_t* n_frames, uint32_t n_streams, size_t hop,
                                     float* d_out_db, size_t stride, const AnalysisParameters* ap, uint32_t* d_peak_mask, uint32_t* d_peak_count,
                                     float* d_center, float* d_size, uint32_t max_peaks, hipStream_t stream) {
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if (n_streams == 0) return PVQ_OK;
    if (!d_pcm || !n_frames || !d_out_db || hop == 0) {
        set_last_error("batch_streams: null pointer or zero hop");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((d_center == nullptr) != (d_size == nullptr)) {
        set_last_error("batch_streams: only one of center/size given");
        return PVQ_ERR_INVALID_ARG;
    }
    bool ragged = false;
    size_t total = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        if (n_frames[s] > stride || n_frames[s] > (size_t)0x7fffffff) {
            set_last_error("batch_streams: a stream has more frames than out_stride_frames (or than 2^31 - 1)");
            return PVQ_ERR_INVALID_ARG;
        }
        if (n_frames[s] > 0 && !d_pcm[s]) {
            set_last_error("batch_streams: null stream pointer");
            return PVQ_ERR_INVALID_ARG;
        }
        ragged |= n_frames[s] != stride;
        total += n_frames[s];
    }
    const size_t rows_total = (size_t)n_streams * stride;
    if (rows_total > (size_t)0x7fffffff) {
        set_last_error("batch_streams: more than 2^31 - 1 output rows");
        return PVQ_ERR_INVALID_ARG;
    }
    PeakParamsDev pk;
    const bool want_peaks = ap && (d_peak_mask || d_peak_count || d_center);
    if (want_peaks && !make_peak_params(*ap, d_peak_mask, d_peak_count, d_center, d_size, max_peaks, pk)) {
        set_last_error("unsupported: peak detection handles 3..1024 bins per frame");
        return PVQ_ERR_UNSUPPORTED;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    {
        pvq_status os = order_on(stream);
        if (os != PVQ_OK) return os;
    }
    const size_t nb = n_bins();
    // rows a stream does not fill are zero frames: nothing reads uninitialised memory, their peak outputs say "no peaks"
    if (ragged) PVQ_HIP(hipMemsetAsync(d_out_db, 0, rows_total * nb * sizeof(float), stream));
    if (total == 0) return PVQ_OK;
    const PeakParamsDev* pkp = want_peaks ? &pk : nullptr;
    size_t r = 0;   // 1: the hop itself; > 1: r interleaved block grids of hop r * hop (Vqt::run_batch)
    switch (route(hop, total, &r)) {
        case BatchRoute::RefuseNoHop:
        case BatchRoute::RefuseUnfusedHop: set_last_error(kNoBlockHop); return PVQ_ERR_UNSUPPORTED;
        case BatchRoute::Fft: {   // (any hop): all streams in ONE launch, the peaks over all rows behind it
            std::vector<FftStream> tab;
            long long f0 = 0;
            for (uint32_t s = 0; s < n_streams; ++s) {
                if (n_frames[s] == 0) continue;
                const size_t lead = n_lead ? n_lead[s] : 0;
                tab.push_back(FftStream{d_pcm[s], (long long)lead, (long long)(lead + n_frames[s] * hop), (long long)((size_t)s * stride), f0});
                f0 += (long long)n_frames[s];
            }
            return launch_fft_streams(tab.data(), tab.size(), nullptr, 0, hop, (size_t)f0, rows_total, d_out_db, nullptr, pkp, stream);
        }
        case BatchRoute::BlockPerStream:   // one stream per call (the unfused block-DFT stages), the peaks once over all rows
            for (uint32_t s = 0; s < n_streams; ++s) {
                if (n_frames[s] == 0) continue;
                pvq_status st = launch_blockdft_path(d_pcm[s], n_lead ? n_lead[s] : 0, hop, n_frames[s], d_out_db + (size_t)s * stride * nb, nullptr, nullptr, stream);
                if (st != PVQ_OK) return st;
            }
            break;
        case BatchRoute::BlockStreams: {   // short streams staged into buffers (plan_stream_staging), then the long ones as they are
            static const int stage_max_env = dev_knob("PVQ_STAGE_MAX", 2048);   // streams of at most this many frames are staged (0: none; measured: 2 048 frames gain 2 %, 512 gain 42 %, 4 096 lose 9 %)
            const StreamStaging plan = plan_stream_staging(d_pcm, n_lead, n_frames, n_streams, stride, hop, r, plan_.window_union, (size_t)stage_max_env);
            for (const StagedBuffer& b : plan.buffers) {   // filled and analysed one after the other on `stream`
                pvq_status ls = stage_buffer(b, hop, stream);
                if (ls != PVQ_OK) return ls;
                std::vector<StreamRun> runs;
                append_staged_runs(runs, b, ws_stage_.as<float>(), hop, r);
                ls = launch_blockdft_streams(runs.data(), runs.size(), hop * r, d_out_db, nullptr, rows_total, nullptr, stream);
                if (ls != PVQ_OK) return ls;
            }
            if (!plan.longs.empty()) {
                pvq_status ls = launch_blockdft_streams(plan.longs.data(), plan.longs.size(), hop * r, d_out_db, nullptr, rows_total, nullptr, stream);
                if (ls != PVQ_OK) return ls;
            }
            break;
        }
    }
    if (want_peaks) {
        pvq_status ps = peaks_stage(d_out_db, rows_total, pk, stream);
        if (ps != PVQ_OK) return ps;
        PVQ_HIP(hipGetLastError());
    }
    return PVQ_OK;
}

// ------------------------------------------------------------------------------------------------
// Many SHORT streams, staged one behind the other (plan_stream_staging, batch_plan.hpp): piece p copies `count` samples from its stream to
// position dst_off of the staging buffer (zeroed before: the gaps between the streams are the zeros / the history each stream's
// first frames see).  grid: (chunks, pieces).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_streams(float* __restrict__ dst, const StagePiece* __restrict__ pieces) {
    const StagePiece p = pieces[blockIdx.y];
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    float* d = dst + p.dst_off;
    for (long long i = t0; i < p.count; i += step) d[i] = p.src[i];
    for (long long i = p.zero_from + t0; i < p.dst_off; i += step) dst[i] = 0.0f;
    for (long long i = p.dst_off + p.count + t0; i < p.zero_to; i += step) dst[i] = 0.0f;
}

// One staged buffer into ws_stage_: the piece table up, then the copy kernel (every sample of the buffer is written).
pvq_status Vqt::stage_buffer(const StagedBuffer& b, size_t hop, hipStream_t stream) {
    pvq_status es = ws_stage_.reserve(b.frames * hop * sizeof(float));
    if (es != PVQ_OK) return es;
    es = ws_stage_tab_.reserve(b.pieces.size() * sizeof(StagePiece));
    if (es != PVQ_OK) return es;
    PVQ_HIP(hipMemcpyAsync(ws_stage_tab_.as<void>(), b.pieces.data(), b.pieces.size() * sizeof(StagePiece), hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns)
    // (the piece table holds at most 65 535 pieces per launch of the copy kernel: grid.y)
    for (size_t p0 = 0; p0 < b.pieces.size(); p0 += 65535) {
        const unsigned np = (unsigned)std::min<size_t>(65535, b.pieces.size() - p0);
        const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((b.longest + 1023) / 1024, 64));
        hipLaunchKernelGGL(stage_streams, dim3(gx, np), dim3(256), 0, stream, ws_stage_.as<float>(), ws_stage_tab_.as<StagePiece>() + p0);
    }
    return PVQ_OK;
}

pvq_status Vqt::calculate_batch_db(const float* pcm, size_t n_lead, size_t hop, size_t n_frames, float* out_db) {
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if (n_frames == 0) return PVQ_OK;
    if (!pcm || !out_db || hop == 0) {
        set_last_error("calculate_batch: null pointer or zero hop");
        return PVQ_ERR_INVALID_ARG;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    // a synchronous call answers for its own input only: whatever an earlier asynchronous call left in the flag (and nobody
    // polled with input_status) is dropped here, not reported against this call's clean samples
    PVQ_HIP(hipDeviceSynchronize());
    PVQ_HIP(hipMemset(dev_->d_status, 0, sizeof(uint32_t)));
    const size_t n_samples = n_lead + n_frames * hop;
    pvq_status st = ws_pcm_.reserve(n_samples * sizeof(float));
    if (st != PVQ_OK) return st;
    st = ws_out_.reserve(n_frames * n_bins() * sizeof(float));
    if (st != PVQ_OK) return st;
    const size_t nb = n_bins();
    constexpr size_t PART = 16384;   // frames per pipeline part
    if (n_frames < 2 * PART) {
        PVQ_HIP(hipMemcpy(ws_pcm_.as<void>(), pcm, n_samples * sizeof(float), hipMemcpyHostToDevice));
        st = calculate_batch_db_device(ws_pcm_.as<float>(), n_lead, hop, n_frames,
                                       ws_out_.as<float>(), nullptr, nullptr);
        if (st != PVQ_OK) return st;
        PVQ_HIP(hipMemcpy(out_db, ws_out_.as<void>(), n_frames * nb * sizeof(float), hipMemcpyDeviceToHost));
        return input_status(nullptr);
    }
    // Large batches: upload, transform and download in parts on three streams, so that with page-locked host buffers
    // (pvq_host_alloc) the two PCIe directions and the kernels overlap.  Part p's frames see the parts before it as
    // history (n_lead grows), so the results are those of one call.  Pageable buffers make the copies synchronous:
    // same results, no overlap.
    if (!host_streams_ready_) {
        for (int i = 0; i < 3; ++i) PVQ_HIP(hipStreamCreateWithFlags(&host_streams_[i], hipStreamNonBlocking));
        host_streams_ready_ = true;
    }
    hipStream_t s_in = host_streams_[0], s_run = host_streams_[1], s_out = host_streams_[2];
    const size_t n_parts = (n_frames + PART - 1) / PART;
    while (host_events_.size() < 2 * n_parts) {
        hipEvent_t e;
        PVQ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        host_events_.push_back(e);
    }
    float* d_pcm = ws_pcm_.as<float>();
    float* d_out = ws_out_.as<float>();
    size_t sample_done = 0;
    // the path is decided ONCE for the whole call and pinned for its parts (as analyze_batch_multi does for its shards): left to itself
    // PVQ_ALGO_AUTO would send a tail part below its threshold to the FFT path, whose values agree with the block-DFT path's to the
    // parity bars, not bit for bit — one synchronous call would mix the two
    struct AlgoPin {
        Vqt* v; pvq_algo saved;
        AlgoPin(Vqt* vv, pvq_algo a) : v(vv), saved(vv->algo()) { v->set_algo(a); }
        ~AlgoPin() { v->set_algo(saved); }
    } pin(this, resolve_algo(hop, n_frames));
    for (size_t p = 0; p < n_parts; ++p) {
        const size_t fbeg = p * PART, nf = std::min(PART, n_frames - fbeg);
        const size_t sample_end = n_lead + (fbeg + nf) * hop;
        PVQ_HIP(hipMemcpyAsync(d_pcm + sample_done, pcm + sample_done, (sample_end - sample_done) * sizeof(float), hipMemcpyHostToDevice, s_in));
        sample_done = sample_end;
        PVQ_HIP(hipEventRecord(host_events_[2 * p], s_in));
        PVQ_HIP(hipStreamWaitEvent(s_run, host_events_[2 * p], 0));
        st = calculate_batch_db_device(d_pcm, n_lead + fbeg * hop, hop, nf, d_out + fbeg * nb, nullptr, s_run);
        if (st != PVQ_OK) return st;
        PVQ_HIP(hipEventRecord(host_events_[2 * p + 1], s_run));
        PVQ_HIP(hipStreamWaitEvent(s_out, host_events_[2 * p + 1], 0));
        PVQ_HIP(hipMemcpyAsync(out_db + fbeg * nb, d_out + fbeg * nb, nf * nb * sizeof(float), hipMemcpyDeviceToHost, s_out));
    }
    PVQ_HIP(hipStreamSynchronize(s_out));
    PVQ_HIP(hipStreamSynchronize(s_run));
    return input_status(s_run);
}

pvq_status Vqt::input_status(hipStream_t stream) {
    if (!has_device() || !dev_ || !dev_->d_status) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    // read and clear as ONE stream-ordered step behind everything the stream holds: a flag raised by work queued on this stream
    // before the call is seen, nothing of it can fall between the read and the clear
    uint32_t flag = 0;
    PVQ_HIP(hipMemcpyAsync(&flag, dev_->d_status, sizeof flag, hipMemcpyDeviceToHost, stream));
    PVQ_HIP(hipMemsetAsync(dev_->d_status, 0, sizeof flag, stream));
    PVQ_HIP(hipStreamSynchronize(stream));
    if (flag == 0) return PVQ_OK;
    set_last_error(kNonFiniteInput);
    return PVQ_ERR_NONFINITE_INPUT;
}

pvq_status Vqt::calculate_vqt_instant_in_db(const float* x, size_t len, float* out_db) {
    if (len != plan_.params.n_fft) {
        set_last_error("input must be exactly n_fft samples");
        return PVQ_ERR_BAD_LENGTH;
    }
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if (!x || !out_db) {
        set_last_error("calculate_vqt_instant_in_db: null pointer");
        return PVQ_ERR_INVALID_ARG;
    }
    // The reference's call shape — one frame, host slice in, host vector out (the viewer: once per rendered frame) — is latency, not
    // throughput: the general host-buffer route (three streams, events, pageable copies of all n_fft samples, a flag read) took
    // 77-92 us of which the GPU worked ~20.  Here: only the window union travels (the first n_fft - window_union samples are never
    // read, SURVEY Appendix B: half of the buffer at 48 kHz, three quarters at the defaults), through page-locked staging on one
    // stream with ONE wait; the non-finite check the kernels would flag is made on the host while the samples are staged; the
    // frame runs the FFT path group-split (launch_fft_streams).  Same kernel, same samples: same bits as a batch of one.
    PVQ_HIP(hipSetDevice(device_id_));
    const size_t wu = plan_.window_union, nb = n_bins(), n_fft = plan_.params.n_fft;
    if (!inst_stream_) PVQ_HIP(hipStreamCreateWithFlags(&inst_stream_, hipStreamNonBlocking));
    if (!inst_pin_) PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&inst_pin_), (wu + nb) * sizeof(float), hipHostMallocDefault));
    {   // (an asynchronous batch still queued on the caller's stream owns ws_pcm_ / ws_out_ / the group-split rows until it is done)
        pvq_status os = order_on(inst_stream_);
        if (os != PVQ_OK) return os;
    }
    pvq_status st = ws_pcm_.reserve(wu * sizeof(float));
    if (st != PVQ_OK) return st;
    st = ws_out_.reserve(nb * sizeof(float));
    if (st != PVQ_OK) return st;
    const float* src = x + (n_fft - wu);
    float bad = 0.0f;   // x - x is 0 for a finite x, NaN for NaN / Inf
    for (size_t i = 0; i < wu; ++i) {
        inst_pin_[i] = src[i];
        bad += src[i] - src[i];
    }
    if (!(bad == 0.0f)) {
        set_last_error(kNonFiniteInput);
        return PVQ_ERR_NONFINITE_INPUT;
    }
    PVQ_HIP(hipMemcpyAsync(ws_pcm_.as<void>(), inst_pin_, wu * sizeof(float), hipMemcpyHostToDevice, inst_stream_));
    // frame 0 of a stream of `wu` samples with wu - 1 of them as history and a hop of 1: its n_fft buffer ends at the last sample
    st = launch_fft_path(ws_pcm_.as<float>(), wu - 1, 1, 1, ws_out_.as<float>(), nullptr, nullptr, inst_stream_);
    if (st != PVQ_OK) return st;
    last_algo_ = PVQ_ALGO_FFT;
    PVQ_HIP(hipMemcpyAsync(inst_pin_ + wu, ws_out_.as<void>(), nb * sizeof(float), hipMemcpyDeviceToHost, inst_stream_));
    PVQ_HIP(hipStreamSynchronize(inst_stream_));
    std::copy(inst_pin_ + wu, inst_pin_ + wu + nb, out_db);
    return PVQ_OK;
}

pvq_status Vqt::analyze_batch_device(const float* d_db, size_t n_frames, const AnalysisParameters& ap,
                                     uint32_t* d_peak_mask, uint32_t* d_peak_count, float* d_center, float* d_size,
                                     uint32_t max_peaks, hipStream_t stream) {
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if (n_frames == 0) return PVQ_OK;
    if (!d_db || ((d_center == nullptr) != (d_size == nullptr))) {
        set_last_error("analyze_batch: null dB pointer, or only one of center/size given");
        return PVQ_ERR_INVALID_ARG;
    }
    PeakParamsDev a;
    if (!make_peak_params(ap, d_peak_mask, d_peak_count, d_center, d_size, max_peaks, a)) {
        set_last_error("unsupported: peak detection handles 3..1024 bins per frame");
        return PVQ_ERR_UNSUPPORTED;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    {
        pvq_status os = order_on(stream);
        if (os != PVQ_OK) return os;
    }
    pvq_status ps = peaks_stage(d_db, n_frames, a, stream);
    if (ps != PVQ_OK) return ps;
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status Vqt::analyze_batch(const float* db, size_t n_frames, const AnalysisParameters& ap, uint32_t* peak_mask,
                              uint32_t* peak_count, float* center, float* size, uint32_t max_peaks) {
    if (pvq_status ds = require_device(); ds != PVQ_OK) return ds;
    if (n_frames == 0) return PVQ_OK;
    if (!db) {
        set_last_error("analyze_batch: null dB pointer");
        return PVQ_ERR_INVALID_ARG;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    const size_t nb = n_bins(), words = (nb + 31) / 32;
    const size_t b_db = n_frames * nb * sizeof(float);
    const size_t b_mask = n_frames * words * sizeof(uint32_t);
    const size_t b_cnt = n_frames * sizeof(uint32_t);
    const size_t b_pk = n_frames * (size_t)max_peaks * sizeof(float);
    pvq_status st = ws_out_.reserve(b_db);
    if (st != PVQ_OK) return st;
    st = ws_misc_.reserve(b_mask + b_cnt + 2 * b_pk + 64);
    if (st != PVQ_OK) return st;
    char* base = ws_misc_.as<char>();
    uint32_t* d_mask = reinterpret_cast<uint32_t*>(base);
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + b_mask);
    float* d_ctr = reinterpret_cast<float*>(base + b_mask + b_cnt);
    float* d_sz = reinterpret_cast<float*>(base + b_mask + b_cnt + b_pk);
    PVQ_HIP(hipMemcpy(ws_out_.as<void>(), db, b_db, hipMemcpyHostToDevice));
    if (max_peaks) PVQ_HIP(hipMemset(d_ctr, 0, 2 * b_pk));
    st = analyze_batch_device(ws_out_.as<float>(), n_frames, ap, d_mask, d_cnt,
                              max_peaks ? d_ctr : nullptr, max_peaks ? d_sz : nullptr, max_peaks, nullptr);
    if (st != PVQ_OK) return st;
    PVQ_HIP(hipDeviceSynchronize());
    if (peak_mask) PVQ_HIP(hipMemcpy(peak_mask, d_mask, b_mask, hipMemcpyDeviceToHost));
    if (peak_count) PVQ_HIP(hipMemcpy(peak_count, d_cnt, b_cnt, hipMemcpyDeviceToHost));
    if (center && max_peaks) PVQ_HIP(hipMemcpy(center, d_ctr, b_pk, hipMemcpyDeviceToHost));
    if (size && max_peaks) PVQ_HIP(hipMemcpy(size, d_sz, b_pk, hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
