/*
 * pvq.h — C ABI of libpvq: MI355X-native batched VQT pitch-analysis engine.
 *
 * Drop-in boundary for the hot path of heinzelotto/pitchvis' `pitchvis_analysis` crate.  The
 * reference has no FFI of its own (consumers link the rlib); every entry point
 * below names the Rust item it replaces (paths relative to pitchvis_analysis/src/).  A Rust shim
 * that re-exposes `Vqt` / `VqtParameters` / `VqtError` over these symbols is shown in
 * INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, caller-allocated outputs, no exceptions cross the ABI
 * (every entry point catches: where the reference panics in kernel construction, vqt.rs:785-792,
 * the call returns PVQ_ERR_INVALID_ARG with the reference's panic text; std::bad_alloc and the like
 * become PVQ_ERR_INTERNAL), every fallible call returns a pvq_status.  A handle is NOT thread-safe (the reference takes
 * `&mut self`, vqt.rs:866); distinct handles are independent (one per worker thread / stream,
 * as pitchvis_train/src/train.rs:146-155 does).  All compute runs on the GPU: there is no CPU
 * fallback, and every compute entry point fails with PVQ_ERR_NO_DEVICE on a handle created
 * without a device.
 */
#ifndef PVQ_H
#define PVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVQ_ABI_VERSION 4   /* (pvq_agc_batch_* came later and left the number alone: new symbols only, nothing that existed changed.)  4: + pvq_vqt_calculate_batch_db_streams, pvq_vqt_analyze_batch_streams (many streams per call).  3: + pvq_vqt_set_workspace_limit, pvq_plan_shard, pvq_vqt_analyze_batch_multi, pvq_analysis_batch_*, profiling mode 2; per-call NaN flag semantics of the synchronous entry points */

/* replaces VqtParameters + VqtRange (vqt.rs:238-262, 278-331), flattened POD */
typedef struct pvq_vqt_params {
    float sr;                    /* VqtParameters::sr */
    uint32_t n_fft;              /* VqtParameters::n_fft */
    float min_freq;              /* VqtRange::min_freq */
    uint32_t octaves;            /* VqtRange::octaves (u8 in the reference) */
    uint32_t buckets_per_octave; /* VqtRange::buckets_per_octave (u16 in the reference) */
    float sparsity_quantile;     /* VqtParameters::sparsity_quantile */
    float quality;               /* VqtParameters::quality */
    float gamma;                 /* VqtParameters::gamma */
} pvq_vqt_params;

/* replaces VqtError (vqt.rs:350-366) plus the panics of vqt.rs:867-871 / analysis.rs:289 */
typedef enum pvq_status {
    PVQ_OK = 0,
    PVQ_ERR_ABOVE_NYQUIST = 1,        /* VqtError::AboveNyquist{highest_frequency, nyquist_frequency} */
    PVQ_ERR_WINDOW_EXCEEDS_NFFT = 2,  /* VqtError::WindowExceedsNFft{window_length, n_fft} */
    PVQ_ERR_BAD_LENGTH = 3,           /* assert_eq!(x.len(), n_fft) vqt.rs:867-871 */
    PVQ_ERR_INVALID_ARG = 4,
    PVQ_ERR_NO_DEVICE = 5,            /* handle has no GPU context (created with device_id < 0) */
    PVQ_ERR_DEVICE = 6,               /* a HIP call failed; see pvq_last_error() */
    PVQ_ERR_UNSUPPORTED = 7,          /* geometry outside what the kernels support */
    PVQ_ERR_INTERNAL = 8,             /* out of host memory or an unexpected C++ exception, caught at the ABI; pvq_last_error() has the text */
    PVQ_ERR_NONFINITE_INPUT = 9       /* a NaN / Inf sample reached a frame (see pvq_vqt_input_status) */
} pvq_status;

const char *pvq_status_string(pvq_status s);
/* thread-local text of the last failing call on this thread */
const char *pvq_last_error(void);
uint32_t pvq_abi_version(void);

/* replaces `impl Default for VqtParameters` (vqt.rs:333-348) and DEFAULT_* (vqt.rs:180-214) */
void pvq_vqt_default_params(pvq_vqt_params *p);

typedef struct pvq_vqt pvq_vqt;

/*
 * replaces Vqt::new (vqt.rs:465-505).  Builds the multi-rate sparse kernel on the host
 * (vqt.rs:517-852) and, when device_id >= 0, uploads it to that GPU.  device_id < 0 creates a
 * host-only "plan" handle: getters work, compute entry points return PVQ_ERR_NO_DEVICE.
 * On PVQ_ERR_ABOVE_NYQUIST / PVQ_ERR_WINDOW_EXCEEDS_NFFT err_detail receives the two fields of
 * the corresponding VqtError variant.
 */
pvq_status pvq_vqt_create(const pvq_vqt_params *params, int device_id, pvq_vqt **out,
                          float err_detail[2]);
/* replaces Drop for Vqt (the viewer swaps the instance at runtime, pitchvis_viewer/src/app/common.rs:1133) */
void pvq_vqt_destroy(pvq_vqt *v);

/* replaces Vqt::params() (vqt.rs:507-509) */
void pvq_vqt_get_params(const pvq_vqt *v, pvq_vqt_params *out);
/* replaces VqtRange::n_buckets() (vqt.rs:259-261) */
uint32_t pvq_vqt_n_bins(const pvq_vqt *v);
/* replaces `pub delay: Duration` (vqt.rs:449, :756), in seconds */
double pvq_vqt_delay_seconds(const pvq_vqt *v);
/* number of trailing samples of the n_fft buffer that any window group reads (the window union) */
uint32_t pvq_vqt_window_union(const pvq_vqt *v);
/* replaces Filter::bandwidth_3db_in_hz (vqt.rs:421, :817-818; find_3db_points / calculate_bandwidth, vqt.rs:956-989):
 * the -3 dB band of every bin's filter in Hz, read off its decimated frequency response; n_bins floats each */
pvq_status pvq_vqt_bandwidths_3db(const pvq_vqt *v, float *lo_hz, float *hi_hz);
/* the warn!() lines of the kernel construction (vqt.rs:695-709: a coverage gap between the -3 dB bands of neighbouring
 * filters — "decrease quality to close the gap"), in bin order: their number, and line i copied NUL-terminated into buf
 * (truncated to cap bytes) */
uint32_t pvq_vqt_warning_count(const pvq_vqt *v);
pvq_status pvq_vqt_warning(const pvq_vqt *v, uint32_t i, char *buf, size_t cap);

/* replaces Vqt::kernel() (vqt.rs:511-513) -> VqtKernel{window_groups} (vqt.rs:388-415) */
uint32_t pvq_vqt_n_groups(const pvq_vqt *v);
/* info[0]=window.0, [1]=window.1, [2]=filter_bank.rows(), [3]=filter_bank.nnz(),
 * [4]=negative_filter_bank nnz (0 <=> None) */
pvq_status pvq_vqt_group_info(const pvq_vqt *v, uint32_t group, uint32_t info[5]);
/* CSR copy-out of WindowGroup::filter_bank (negative=0) or ::negative_filter_bank (negative=1);
 * values are interleaved (re, im) Complex32 */
pvq_status pvq_vqt_group_csr(const pvq_vqt *v, uint32_t group, int negative, uint32_t *row_ptr,
                             uint32_t *col_idx, float *values);
/* per-bin FilterParams (vqt.rs:370-384), arrays of n_bins */
pvq_status pvq_vqt_filter_params(const pvq_vqt *v, float *freq, float *window_length,
                                 uint32_t *sr_downscaling_factor, uint32_t *minimum_needed_window_size);

/*
 * replaces Vqt::calculate_vqt_instant_in_db (vqt.rs:866-916): x = exactly n_fft host samples,
 * the last of which is "now"; out_db = n_bins host floats.  len != n_fft -> PVQ_ERR_BAD_LENGTH
 * (the reference panics).  Synchronous, and shaped for latency: only the window union of x (its last
 * pvq_vqt_window_union samples: the kernel reads nothing before them) is staged, page-locked, on a stream of the handle's
 * own; a non-finite sample among them returns PVQ_ERR_NONFINITE_INPUT before anything is launched (out_db untouched).
 * Always the FFT path (one frame has nothing to share with a neighbour), whatever pvq_vqt_set_algo says.
 */
pvq_status pvq_vqt_calculate_instant_db(pvq_vqt *v, const float *x, size_t len, float *out_db);

/*
 * Batched form of the same call, the data-parallel path the reference runs with one Vqt per
 * rayon worker (pitchvis_train/src/train.rs:146-155, :276-310, :341).
 * Framing: a ring buffer of n_fft zeros; hop f (0-based) shifts `hop` samples in, then frame f
 * analyses the last n_fft samples (pitchvis_audio/src/audio_desktop.rs:113-115 shift semantics).
 * `pcm` holds n_lead + n_frames*hop samples; the first n_lead are history that precedes hop 0
 * (0 at stream start, > 0 for a shard that carries a halo); samples before pcm[0] are zeros.
 * out_db: [n_frames][n_bins] row-major.  Host pointers; synchronous.
 */
pvq_status pvq_vqt_calculate_batch_db(pvq_vqt *v, const float *pcm, size_t n_lead, size_t hop,
                                      size_t n_frames, float *out_db);

/*
 * Device-pointer form: d_pcm, d_out_db (and optional d_out_cplx: [n_frames][n_bins][2], the
 * complex coefficients before power_to_db, may be NULL) are device memory on the handle's GPU.
 * Enqueued on `stream` (a hipStream_t; NULL = default stream); returns without synchronising.
 *
 * Bin counts.  pvq_vqt_create takes any geometry; what a call can compute depends on the path.  The block-DFT path takes
 * 3..1024 bins, as do peak detection (pvq_analyze_batch*, pvq_vqt_analyze_batch*) and the batched AnalysisState; above 1024 they
 * return PVQ_ERR_UNSUPPORTED with a message and leave their outputs untouched.  The FFT path (PVQ_ALGO_AUTO above 1024 bins, and
 * pvq_vqt_calculate_instant_db) takes up to 4096 bins while a frame's largest FFT and its bins fit 160 KB of LDS (about 3000 bins
 * beside a 32 768-sample window); beyond that the call returns PVQ_ERR_UNSUPPORTED with a message, before anything is launched.
 */
pvq_status pvq_vqt_calculate_batch_db_device(pvq_vqt *v, const float *d_pcm, size_t n_lead,
                                             size_t hop, size_t n_frames, float *d_out_db,
                                             float *d_out_cplx, void *stream);

/*
 * NaN / Inf policy.  The reference's callers never pass non-finite samples to the transform (the audio
 * callback drops such chunks, pitchvis_audio/src/audio_desktop.rs:102-105), and the NaNs they would cause make its peak
 * stage panic (peak_detection.rs:145 `partial_cmp().unwrap()`).  Here a non-finite sample inside one of a frame's windows
 * raises a sticky flag on the device while the frame's dB values are computed; the frames it touches are unspecified.
 * The synchronous host-buffer batch entry points (pvq_vqt_calculate_batch_db, pvq_train_frames_db) check the flag themselves
 * and return PVQ_ERR_NONFINITE_INPUT; such a call reports its own input only — it clears, unreported, whatever an earlier
 * asynchronous call of the same handle raised and nobody polled.  pvq_vqt_calculate_instant_db does not use the flag at all: it
 * checks its window union on the host while staging it, launches nothing on a non-finite sample, and neither reads nor clears what
 * an earlier asynchronous call left behind.  For the asynchronous device-pointer entry points call this: it waits for `stream`,
 * returns PVQ_ERR_NONFINITE_INPUT if the flag is up (PVQ_OK otherwise) and clears it (read and clear are one stream-ordered step on
 * `stream`: poll on the stream the work was queued on).  The flag is per handle.
 *
 * Ordering of one handle's calls.  The handle owns its workspaces, so its device calls are ordered: a call on another stream than
 * the handle's previous call — pvq_vqt_calculate_instant_db and pvq_stream_frame_db run on streams of their own — first makes its
 * stream wait, on the device, for everything the previous call queued (the host does not block; calls that stay on one stream pay
 * nothing).  The handle itself is still not thread-safe: one handle per thread, as one `&mut Vqt` in the reference.
 */
pvq_status pvq_vqt_input_status(pvq_vqt *v, void *stream);

/* algorithm selection for the batch path (default PVQ_ALGO_AUTO) */
typedef enum pvq_algo {
    PVQ_ALGO_AUTO = 0,
    PVQ_ALGO_FFT = 1,      /* per-frame LDS FFT per window group (any hop) */
    PVQ_ALGO_BLOCKDFT = 2  /* hop-block DFT on fp32 MFMA + phase combine: every hop block is transformed once for all the frames that
                            * share it.  Takes a power-of-two hop (>= 64) that divides every window (doubling tree); a multiple of 64 that
                            * the longest window holds at most 16 times, e.g. 1 600 (whole blocks + the window's remainder, Horner combine);
                            * or a hop whose 2-, 4-, 8- or 16-fold is one of those, e.g. 800 or 320 (that many interleaved block grids).
                            * PVQ_ALGO_AUTO picks it where it applies and pays (pvq_vqt_resolve_algo); forcing it on another hop
                            * (735, say) returns PVQ_ERR_UNSUPPORTED */
} pvq_algo;
pvq_status pvq_vqt_set_algo(pvq_vqt *v, pvq_algo algo);
/* which algorithm the last batch call actually used */
pvq_algo pvq_vqt_last_algo(const pvq_vqt *v);
/* which algorithm a batch of n_frames frames (all streams of a *_streams call together) at this hop takes under the current setting.
 * PVQ_ALGO_AUTO takes the block-DFT path where it applies and is the faster one: from 384 frames on for a power-of-two hop; for a
 * general hop (1 600, 800 ...) from where its launch floor — a K loop hop / 2 deep per tile — is paid back, ~1 700 frames at
 * 48 kHz / 252 bins / hop 1 600 (smaller batches: the FFT path, a workgroup per frame).  The two paths agree to the parity bars, not
 * bit for bit: a caller that needs the same bits for every batch size fixes the path with pvq_vqt_set_algo. */
pvq_algo pvq_vqt_resolve_algo(pvq_vqt *v, size_t hop, size_t n_frames);

/* arithmetic of the block-DFT GEMM and kernel product (default PVQ_GEMM_F32).  Both accumulate in fp32 and meet the
 * same parity bars; PVQ_GEMM_BF16X3 writes each fp32 operand exactly as three bf16 terms and uses the bf16 matrix
 * cores (six exact partial products per fp32 product, dropped terms < 2^-24): ~10 % faster end to end. */
typedef enum pvq_gemm_precision {
    PVQ_GEMM_F32 = 0,     /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32)  */
    PVQ_GEMM_BF16X3 = 1   /* split-bf16: 6 bf16 MFMAs per fp32 product block, error at fp32 rounding level */
} pvq_gemm_precision;
pvq_status pvq_vqt_set_gemm_precision(pvq_vqt *v, pvq_gemm_precision p);
/* twiddle tables (FFT twiddles, real-split factors, block-DFT matrix and combine phases) rounded to IEEE half
 * before use, accumulation in fp32: the "fp16 FFT twiddles" variant of BASELINE.json configs[3].  Off by default;
 * switching rebuilds the device tables.  Expect ~1e-3 relative error (tests/test_configs_gpu.py reports it). */
pvq_status pvq_vqt_set_twiddle_fp16(pvq_vqt *v, int enable);
/* Upper bound, in bytes, of the block-DFT path's intermediate spectrum workspace of this handle (grow-only device memory,
 * ~5.6 KB per frame of a sub-batch at 48 kHz / 252 bins, more with more spectrum columns).  A batch longer than the workspace
 * holds is processed in sub-batches of a multiple of 64 frames, at most 147 456.  Default (and bytes == 0): 1 GiB.  The
 * reference's trainer keeps one Vqt per worker thread (pitchvis_train/src/train.rs:146-155): size this per handle. */
pvq_status pvq_vqt_set_workspace_limit(pvq_vqt *v, uint64_t bytes);
/* complex spectrum columns per hop block the block-DFT GEMM computes (padded), 0 before its first use */
uint32_t pvq_vqt_blockdft_columns(const pvq_vqt *v);

/* ---- peak / note detection: analysis_modules/peak_detection.rs + analysis.rs:332-361 ---- */

/* replaces the peak-related fields of AnalysisParameters (analysis.rs:36-65, defaults :72-98) */
typedef struct pvq_analysis_params {
    float peak_min_prominence;     /* peak_config.min_prominence = 10.0 */
    float peak_min_height;         /* peak_config.min_height = 4.0 */
    float bass_min_prominence;     /* bassline_peak_config.min_prominence = 5.0 */
    float bass_min_height;         /* bassline_peak_config.min_height = 3.5 */
    uint32_t highest_bassnote;     /* 28 */
    float harmonic_threshold;      /* 0.3 */
} pvq_analysis_params;
void pvq_analysis_default_params(pvq_analysis_params *a);

/*
 * Per-frame stateless analysis of dB frames, i.e. AnalysisState::preprocess's peak pipeline
 * (analysis.rs:332-361: find_peaks bass/general split -> enhance_peaks_continuous ->
 * promote_bass_peaks_with_harmonics) with the EMA in pass-through mode
 * (update_vqt_smoothing_duration(None), analysis.rs:251-269).
 * d_db: [n_frames][n_bins] device.  Outputs (device, any may be NULL):
 *   d_peak_mask  [n_frames][ceil(n_bins/32)] u32 bitmask of AnalysisState::peaks
 *   d_peak_count [n_frames] number of peaks
 *   d_center/d_size [n_frames][max_peaks] AnalysisState::peaks_continuous, ascending center;
 *                   entries beyond the frame's count are untouched.
 */
pvq_status pvq_analyze_batch_device(pvq_vqt *v, const float *d_db, size_t n_frames,
                                    const pvq_analysis_params *a, uint32_t *d_peak_mask,
                                    uint32_t *d_peak_count, float *d_center, float *d_size,
                                    uint32_t max_peaks, void *stream);

/* Host-pointer convenience wrapper of the above (uploads, runs on the GPU, downloads). */
pvq_status pvq_analyze_batch(pvq_vqt *v, const float *db, size_t n_frames,
                             const pvq_analysis_params *a, uint32_t *peak_mask, uint32_t *peak_count,
                             float *center, float *size, uint32_t max_peaks);

/* The whole hot path in one call: PCM -> VQT dB frames -> peaks (device pointers, async). */
pvq_status pvq_vqt_analyze_batch_device(pvq_vqt *v, const float *d_pcm, size_t n_lead, size_t hop,
                                        size_t n_frames, const pvq_analysis_params *a,
                                        float *d_out_db, uint32_t *d_peak_mask,
                                        uint32_t *d_peak_count, float *d_center, float *d_size,
                                        uint32_t max_peaks, void *stream);


/* ---- many streams, one call ----------------------------------------------------------------------------
 * The reference's batch driver analyses MANY independent files side by side, one Vqt per rayon worker
 * (pitchvis_train/src/train.rs:146-163), and a stereo recording is two streams.  Here one handle takes all of them in one
 * call: d_pcm is a HOST array of n_streams device pointers; stream s holds n_lead[s] + n_frames[s] * hop samples (n_lead
 * NULL: no history anywhere) and is framed exactly as by pvq_vqt_calculate_batch_db_device; its frame f goes to row
 * s * out_stride_frames + f of d_out_db [n_streams][out_stride_frames][n_bins] (out_stride_frames >= every n_frames[s]) — the
 * layout pvq_analysis_batch_preprocess_device reads, so PCM -> VQT -> AnalysisState::preprocess of many streams never leaves
 * the device.  Rows a stream does not fill are zero frames.  With a power-of-two hop (the block-DFT path) every stage covers
 * ALL streams with one launch — 64 streams of 2 048 frames cost what one 131 072-frame stream costs, not 64 launch ramps and
 * tails per stage; every value equals, bit for bit, what the single-stream call computes for that stream.  Streams of at most
 * 2 048 frames are first copied one behind the other into a staging buffer of the handle (grow-only device memory, at most 512 MiB:
 * a tile of the GEMM then never stops at a stream's end; 256 streams of 512 frames run at 0.86 instead of 0.61 of the single-stream
 * rate); longer ones are read where they are.  Asynchronous on `stream`; NaN / Inf policy as for the device-pointer entry points
 * (pvq_vqt_input_status). */
pvq_status pvq_vqt_calculate_batch_db_streams(pvq_vqt *v, const float *const *d_pcm, const size_t *n_lead,
                                              const size_t *n_frames, uint32_t n_streams, size_t hop, float *d_out_db,
                                              size_t out_stride_frames, void *stream);
/* The same with the per-frame peak pipeline behind it (as pvq_vqt_analyze_batch_device): peak outputs are laid out by the
 * same rows, [n_streams][out_stride_frames][...]; any may be NULL (center and size go together). */
pvq_status pvq_vqt_analyze_batch_streams(pvq_vqt *v, const float *const *d_pcm, const size_t *n_lead,
                                         const size_t *n_frames, uint32_t n_streams, size_t hop,
                                         const pvq_analysis_params *a, float *d_out_db, size_t out_stride_frames,
                                         uint32_t *d_peak_mask, uint32_t *d_peak_count, float *d_center, float *d_size,
                                         uint32_t max_peaks, void *stream);

/* ---- several devices, one stream ---------------------------------------------------------------------
 * The reference's only data-parallel driver hands every rayon worker its own Vqt (pitchvis_train/src/train.rs:146-155:
 * par_iter().map_init(|| Vqt::new(..), ..)).  The same shape here: one handle per worker (each on its own device, or
 * several on one), ONE long stream split into contiguous frame ranges, each with a halo of window_union - hop samples of
 * history, kernel tables replicated, no collective on the data path. */
typedef struct pvq_shard {
    uint64_t first_frame;   /* global index of the shard's first frame */
    uint64_t n_frames;
    uint64_t sample_begin;  /* first sample of the stream the shard must hold, counted from the stream's first hop */
    uint64_t sample_end;    /* one past the last */
    uint64_t n_lead;        /* samples of [sample_begin, sample_end) that are history before the shard's first hop */
} pvq_shard;
/* contiguous split of n_frames_total frames over `world` shards (the first n_frames_total % world take one more) */
pvq_status pvq_plan_shard(uint64_t n_frames_total, uint64_t hop, uint64_t window_union, uint32_t rank, uint32_t world,
                          pvq_shard *out);
/* PCM -> dB frames -> peaks of one HOST stream on n_handles handles at once, one host thread each; the handles must have
 * been created with the same parameters, and none may appear twice.  pcm: [n_lead + n_frames * hop]; outputs are host
 * arrays laid out as for pvq_vqt_analyze_batch_device (peak outputs may be NULL; center and size go together).  Every
 * output value equals, bit for bit, what one handle computes for the whole stream. */
pvq_status pvq_vqt_analyze_batch_multi(pvq_vqt *const *handles, uint32_t n_handles, const float *pcm, size_t n_lead,
                                       size_t hop, size_t n_frames, const pvq_analysis_params *a, float *out_db,
                                       uint32_t *peak_mask, uint32_t *peak_count, float *center, float *size,
                                       uint32_t max_peaks);

/* ---- stateful per-stream analysis: AnalysisState (analysis.rs:119-410), host side ------------------
 * preprocess() is a recurrence over frames (bin EMAs, calmness EMAs and the scene calmness feed the
 * next frame's smoothing horizons: analysis.rs:295-319, calmness.rs:23-95), so it is sequential per
 * stream and runs on the host, fed with dB frames computed on the GPU.  One handle per stream. */

/* replaces AnalysisParameters (analysis.rs:36-65), Default at :72-98; durations in nanoseconds */
typedef struct pvq_analysis_full_params {
    uint32_t spectrogram_length;                       /* 400 (unused by the crate itself) */
    float peak_min_prominence, peak_min_height;        /* peak_config 10.0 / 4.0 */
    float bass_min_prominence, bass_min_height;        /* bassline_peak_config 5.0 / 3.5 */
    uint32_t highest_bassnote;                         /* 28 */
    uint64_t vqt_smoothing_duration_base_ns;           /* 70 ms */
    float vqt_smoothing_calmness_min, vqt_smoothing_calmness_max;  /* 0.6 / 2.0 */
    uint64_t note_calmness_smoothing_duration_ns;      /* 3500 ms */
    uint64_t scene_calmness_smoothing_duration_ns;     /* 800 ms */
    uint64_t tuning_inaccuracy_smoothing_duration_ns;  /* 4000 ms */
    float harmonic_threshold;                          /* 0.3 */
} pvq_analysis_full_params;
void pvq_analysis_full_default_params(pvq_analysis_full_params *p);

typedef struct pvq_analysis_state pvq_analysis_state;
/* replaces AnalysisState::new(range, params) (analysis.rs:192) */
pvq_status pvq_analysis_state_create(float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                     const pvq_analysis_full_params *params, pvq_analysis_state **out);
void pvq_analysis_state_destroy(pvq_analysis_state *s);
/* replaces update_vqt_smoothing_duration(Option<Duration>) (analysis.rs:251); has_duration = 0 is None */
pvq_status pvq_analysis_state_update_vqt_smoothing_duration(pvq_analysis_state *s, int has_duration, uint64_t duration_ns);
/* replaces preprocess(&[f32], Duration) (analysis.rs:288); a wrong length returns PVQ_ERR_BAD_LENGTH
 * where the reference panics (analysis.rs:289) */
pvq_status pvq_analysis_state_preprocess(pvq_analysis_state *s, const float *x_vqt, size_t len, uint64_t frame_time_ns);
/* replaces bin_to_frequency (analysis.rs:407) */
float pvq_analysis_state_bin_to_frequency(const pvq_analysis_state *s, uint32_t bin);

/* the `pub` result fields (analysis.rs:119-177); arrays have n_buckets entries */
typedef enum pvq_analysis_field {
    PVQ_FIELD_X_VQT_SMOOTHED = 0,  /* x_vqt_smoothed[i].get() */
    PVQ_FIELD_X_VQT_PEAKFILTERED = 1,
    PVQ_FIELD_X_VQT_AFTERGLOW = 2,
    PVQ_FIELD_CALMNESS = 3,        /* calmness[i].get() */
    PVQ_FIELD_PITCH_ACCURACY = 4,
    PVQ_FIELD_PITCH_DEVIATION = 5
} pvq_analysis_field;
uint32_t pvq_analysis_state_n_buckets(const pvq_analysis_state *s);
pvq_status pvq_analysis_state_get_field(const pvq_analysis_state *s, pvq_analysis_field f, float *out);
/* peaks (ascending bin indices) and peaks_continuous (ascending center); return the total count */
uint32_t pvq_analysis_state_get_peaks(const pvq_analysis_state *s, uint32_t *out, uint32_t capacity);
uint32_t pvq_analysis_state_get_peaks_continuous(const pvq_analysis_state *s, float *center, float *size, uint32_t capacity);
float pvq_analysis_state_scene_calmness(const pvq_analysis_state *s);            /* smoothed_scene_calmness.get() */
float pvq_analysis_state_tuning_grid_inaccuracy(const pvq_analysis_state *s);    /* smoothed_tuning_grid_inaccuracy.get() */

/* ---- AnalysisState for MANY streams, on the GPU ------------------------------------------------------
 * preprocess() cannot be split over time, but streams are independent (the trainer analyses many files side by side,
 * pitchvis_train/src/train.rs:146-155): one wavefront owns one stream and walks its frames in order, thousands of streams in
 * parallel ("replicas only": no exchange between streams or devices).  Same arithmetic, same operation order as the host
 * pvq_analysis_state above; every stream starts as AnalysisState::new leaves it (analysis.rs:192-241) and keeps its state
 * between calls. */
typedef struct pvq_analysis_batch pvq_analysis_batch;
/* per-frame results, DEVICE pointers, any may be NULL (center and size go together, with max_peaks > 0).  Per-bin fields:
 * [n_streams][n_frames][n_bins]; peak_mask [..][..][ceil(n_bins/32)]; center / size [..][..][max_peaks] (ascending center, entries
 * beyond the frame's count untouched); peak_count, scene_calmness, tuning_grid_inaccuracy [n_streams][n_frames]. */
typedef struct pvq_analysis_batch_outputs {
    float *x_vqt_smoothed, *x_vqt_peakfiltered, *x_vqt_afterglow, *calmness, *pitch_accuracy, *pitch_deviation;
    uint32_t *peak_mask, *peak_count;
    float *center, *size;
    uint32_t max_peaks;
    float *scene_calmness, *tuning_grid_inaccuracy;
} pvq_analysis_batch_outputs;
/* n_streams AnalysisState::new(range, params) on device `device_id` (params NULL: AnalysisParameters::default) */
pvq_status pvq_analysis_batch_create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                     const pvq_analysis_full_params *params, uint32_t n_streams, pvq_analysis_batch **out);
void pvq_analysis_batch_destroy(pvq_analysis_batch *b);
/* AnalysisState::update_vqt_smoothing_duration (analysis.rs:251) on every stream */
pvq_status pvq_analysis_batch_update_vqt_smoothing_duration(pvq_analysis_batch *b, int has_duration, uint64_t duration_ns);
/* AnalysisState::preprocess (analysis.rs:288) for n_frames frames of every stream, in order: d_db [n_streams][n_frames][n_bins]
 * (device).  frame_time_ns applies to every frame unless frame_times_ns (HOST array of n_frames) is given.  Asynchronous on
 * `stream` — except that a call whose frame time(s) differ from the previous call's first waits for `stream` (the table of EMA weights
 * 1 - exp(-2 frame_time / horizon), built on the host with its libm so that the device follows the host AnalysisState bit for bit, is
 * replaced). */
pvq_status pvq_analysis_batch_preprocess_device(pvq_analysis_batch *b, const float *d_db, size_t n_frames, uint64_t frame_time_ns,
                                                const uint64_t *frame_times_ns, const pvq_analysis_batch_outputs *outs,
                                                void *stream);
/* The consumers' loop in one call, for many streams: per stream and hop what pitchvis_viewer does per rendered frame
 * (vqt_system.rs:40-68 -> Vqt::calculate_vqt_instant_in_db, analysis_system.rs:10-20 -> AnalysisState::preprocess) and pitchvis_serial
 * per 1 / 30 s (main.rs:205-215).  d_pcm / n_lead as for pvq_vqt_calculate_batch_db_streams, n_frames frames of EVERY stream (the
 * batch's n_streams of them); the dB frames [n_streams][n_frames][n_bins] go through a buffer of the batch object (grow-only device
 * memory) — or through d_db if the caller wants them — and never leave the device.  v and b must sit on the same device and share
 * the VqtRange.  frame_time_ns: the hop's duration (hop / sr, what a live consumer measures between two analyses).  Asynchronous. */
pvq_status pvq_analysis_batch_preprocess_pcm(pvq_analysis_batch *b, pvq_vqt *v, const float *const *d_pcm, const size_t *n_lead,
                                             size_t n_frames, size_t hop, uint64_t frame_time_ns, float *d_db,
                                             const pvq_analysis_batch_outputs *outs, void *stream);
/* the state of one stream after the last call (synchronises): a pub field as pvq_analysis_state_get_field, and the two scalars */
pvq_status pvq_analysis_batch_get_field(pvq_analysis_batch *b, uint32_t stream_index, pvq_analysis_field f, float *out);
pvq_status pvq_analysis_batch_get_scalars(pvq_analysis_batch *b, uint32_t stream_index, float *scene_calmness,
                                          float *tuning_grid_inaccuracy);

/* ------------------------------------------------------------------------------------------------
 * Callers either side of the path: host code around the GPU frames.
 * ---------------------------------------------------------------------------------------------- */

/* dagc::MonoAgc (dagc_fork/src/lib.rs:19-87).  create: PVQ_ERR_INVALID_ARG with the reference's Error text
 * for a bad desired_output_rms / distortion_factor (lib.rs:36-49). */
typedef struct pvq_mono_agc pvq_mono_agc;
pvq_status pvq_mono_agc_create(float desired_output_rms, float distortion_factor, pvq_mono_agc **out);
void pvq_mono_agc_destroy(pvq_mono_agc *a);
void pvq_mono_agc_freeze_gain(pvq_mono_agc *a, int freeze);      /* lib.rs:62 */
int pvq_mono_agc_is_gain_frozen(const pvq_mono_agc *a);           /* lib.rs:67 */
float pvq_mono_agc_gain(const pvq_mono_agc *a);                   /* lib.rs:72 */
void pvq_mono_agc_process(pvq_mono_agc *a, float *samples, size_t n);   /* lib.rs:76-86, in place */

/* pitchvis_train as a batch (pitchvis_train/src/train.rs).
 * chunk length: (delay_ms * sr / 1000) / 64 * 64, train.rs:128-129 */
size_t pvq_train_chunk_samples(const pvq_vqt *v);
/* train.rs:286-310 over n_chunks rendered chunks of `chunk` samples: downmix (l + r) / 2 (right may be NULL),
 * silence gate (sum of squares < 1e-6 freezes the gain for the chunk), AGC in place.  mono_out
 * [n_chunks * chunk]; gain_out [n_chunks] (may be NULL) = agc.gain() after each chunk. */
pvq_status pvq_train_condition_stream(pvq_mono_agc *a, const float *left, const float *right, size_t n_chunks,
                                      size_t chunk, float *mono_out, float *gain_out);
/* The same conditioning for MANY streams on the device (the trainer's par_iter over files, train.rs:146-163): one MonoAgc per
 * stream, a lane per stream for the recurrence, nothing leaves the device between conditioning and transform.  Every sample and
 * every gain carries the bits pvq_train_condition_stream gives that stream.
 * create: n_streams dagc::MonoAgc::new(desired_output_rms, distortion_factor) (dagc_fork/src/lib.rs:35-53) on device_id; the
 * argument checks and texts of pvq_mono_agc_create, PVQ_ERR_INVALID_ARG before any device is touched; device_id < 0: a host-only
 * handle whose condition call returns PVQ_ERR_NO_DEVICE. */
typedef struct pvq_agc_batch pvq_agc_batch;
pvq_status pvq_agc_batch_create(int device_id, uint32_t n_streams, float desired_output_rms, float distortion_factor,
                                pvq_agc_batch **out);
void pvq_agc_batch_destroy(pvq_agc_batch *b);
/* train.rs:286-301 for every stream: d_left / d_right / d_mono_out are HOST arrays of n_streams DEVICE pointers (d_right NULL,
 * or an entry NULL: that stream is mono); stream s has n_chunks[s] chunks of `chunk` samples and nothing past them is written.
 * d_gain_out (device, may be NULL): [n_streams][gain_stride], agc.gain() after each chunk; entries past a stream's n_chunks are
 * left alone.  In place is allowed (d_mono_out[s] == d_left[s]); rows that overlap in any other way are not.  Every stream's gain
 * persists between calls, like one MonoAgc per stream on the host.  PVQ_ERR_INVALID_ARG (chunk == 0, a null table, a null left or
 * output pointer of a stream with chunks, gain_stride smaller than a stream's n_chunks) before anything is launched.  Asynchronous
 * on `stream`; the calls of one handle go to one stream.  d_mono_out is what pvq_vqt_calculate_batch_db_streams takes as d_pcm
 * with hop = chunk * step, n_lead = NULL, n_frames[s] = n_chunks[s] / step: the many-streams form of pvq_train_frames_db. */
pvq_status pvq_agc_batch_condition_device(pvq_agc_batch *b, const float *const *d_left, const float *const *d_right,
                                          const size_t *n_chunks, size_t chunk, float *const *d_mono_out,
                                          float *d_gain_out, size_t gain_stride, void *stream);
/* lib.rs:72 for every stream after the last call: gains [n_streams] (synchronises) */
pvq_status pvq_agc_batch_get_gains(pvq_agc_batch *b, float *gains);
/* train.rs:341 for every step-th chunk (STEP_SIZE_IN_CHUNKS = 3, train.rs:44), on the GPU: frame f = VQT dB of
 * the last n_fft conditioned samples after chunk (f+1)*step (zeros before the stream, the ring buffer of
 * train.rs:268-269).  out_db [n_chunks / step][n_bins]. */
pvq_status pvq_train_frames_db(pvq_vqt *v, const float *mono, size_t n_chunks, size_t chunk, size_t step, float *out_db);
/* train.rs:317-337, 347, 443-460: row f = n_bins dB values, then 128 targets from the active keys of frame
 * f-1 (a key's value: largest (mix_left + mix_right) / 2 * agc_gain over its voices; target = value > 0.5).
 * voice_ptr [n_frames + 1] indexes the voice arrays; agc_gain [n_frames].  out_rows [n_frames][n_bins + 128].
 * PVQ_ERR_INVALID_ARG for a key outside 0..127 (the reference would panic). */
pvq_status pvq_train_rows(const float *db, size_t n_frames, uint32_t n_bins, const uint32_t *voice_ptr,
                          const int32_t *voice_key, const float *voice_gain_left, const float *voice_gain_right,
                          const float *agc_gain, float *out_rows);
/* train.rs:192-208: flat little-endian f32 .npy, shape (n,) */
pvq_status pvq_npy_write_f32(const char *path, const float *data, uint64_t n);

/* Streaming front end: the pitchvis_audio RingBuffer contract (pitchvis_audio/src/lib.rs:17-22,
 * audio_desktop.rs:88-131) with the ring resident on the device.  The ring holds buf_size samples, zeros at
 * start; push() is the audio callback: a chunk containing a non-finite sample is dropped (audio_desktop.rs:
 * 97-100), otherwise the silence gate + MonoAgc(0.07, 0.0001) run over it (with_agc != 0), it is shifted into
 * the ring (drain + extend) and gain / chunk_size_ms are updated.  frame_db() is the consumer of
 * pitchvis_serial/src/main.rs:205-211: the VQT of the newest n_fft samples.  Not thread-safe: serialise push
 * and frame_db like the reference's mutex does. */
typedef struct pvq_stream pvq_stream;
pvq_status pvq_stream_create(pvq_vqt *v, size_t buf_size, int with_agc, pvq_stream **out);
void pvq_stream_destroy(pvq_stream *s);
pvq_status pvq_stream_push(pvq_stream *s, const float *data, size_t n);
float pvq_stream_gain(const pvq_stream *s);             /* RingBuffer.gain */
float pvq_stream_chunk_size_ms(const pvq_stream *s);    /* RingBuffer.chunk_size_ms */
pvq_status pvq_stream_frame_db(pvq_stream *s, float *out_db);
/* host copy of the newest n_last samples of the ring (n_last <= buf_size) */
pvq_status pvq_stream_read(pvq_stream *s, float *out, size_t n_last);

/* pitchvis_colors::calculate_color (pitchvis_colors/src/lib.rs:86-117); colors: 12 RGB triples in [0, 1] */
void pvq_calculate_color(uint16_t buckets_per_octave, float bucket, const float *colors, float gray_level,
                         float easing_pow, float out_rgb[3]);
/* pitchvis_serial::update_serial (pitchvis_serial/src/main.rs:122-175): 0xFF, 16-bit triple count (big endian),
 * then one RGB triple (each byte <= 0xFE) per bucket.  center/size: AnalysisState::peaks_continuous.  out must
 * hold 3 + 3 * n_buckets bytes; returns the number of bytes written. */
size_t pvq_led_frame(uint32_t n_buckets, uint16_t buckets_per_octave, const float *center, const float *size,
                     uint32_t n_peaks, const float *colors, float gray_level, float easing_pow, uint8_t *out);

/* ---- what the viewer and the LED strip show, from AnalysisState alone ---------------------------------
 * pitchvis_viewer/src/display_system/update.rs turns an AnalysisState into a spectrogram texture row (update_spectrogram_system,
 * update.rs:929-1087, both SpectrogramModes) and twelve chroma strengths (update_chroma_system, update.rs:1090-1144);
 * pitchvis_serial turns it into an LED frame (pvq_led_frame above).  Stateless: texture management (the ring of rows, its vertical
 * flip, clearing the next line, the scroll offset) stays with the caller, or with the overlay stage further down, which keeps it. */
typedef enum pvq_spectrogram_mode {
    PVQ_SPECTROGRAM_VQT = 0,   /* SpectrogramMode::VQT (update.rs:962-1004): x_vqt_smoothed, brightness against the row's maximum */
    PVQ_SPECTROGRAM_PEAKS = 1  /* SpectrogramMode::Peaks (update.rs:1005-1065): peaks_continuous, a radius of 2 bins each */
} pvq_spectrogram_mode;
/* replaces the match of update_spectrogram_system (update.rs:961-1065): the RGBA row the reference writes at write_index,
 * out_rgba [n_buckets][4].  PVQ_SPECTROGRAM_VQT reads x_vqt_smoothed [n_buckets] (center / size may be NULL); every channel is
 * (x * 255 * 1.2).clamp(0, 255) as u8, alpha from (1 - (1 - v / (max + 0.001))^2) * 1.5 clamped to 0..1, RGB written whether or not
 * the row has a positive maximum.  PVQ_SPECTROGRAM_PEAKS reads center / size [n_peaks] in the given order (x_vqt_smoothed may be
 * NULL): the row starts as zeros, every peak overwrites all four bytes of the bins within 2 of its centre (floor(c - 2).max(0) ..
 * ceil(c + 2).min(n_buckets), upper bound exclusive), alpha = brightness * exp(-d^2 / 2); the last writer wins; nothing is drawn
 * unless the largest size is > 0.  A NaN gives bytes 0 (`as u8`), and f32::max ignores it.  colors: 12 RGB triples in [0, 1].
 * PVQ_ERR_INVALID_ARG for an unknown mode, buckets_per_octave == 0 or a missing array. */
pvq_status pvq_spectrogram_row(int mode, uint32_t n_buckets, uint16_t buckets_per_octave, const float *x_vqt_smoothed,
                               const float *center, const float *size, uint32_t n_peaks, const float *colors, float gray_level,
                               float easing_pow, uint8_t *out_rgba);
/* replaces the chroma of update_chroma_system (update.rs:1102-1131): out12[class] = sum of 10^(x_vqt_smoothed[bin] / 10) over the
 * bins of the pitch class ((round(bin * 12 / bpo) + bin_0_pitch_class) % 12, bin_0_pitch_class from round(12 log2(min_freq /
 * 261.626))), summed in ascending bin order in f32, divided by the largest of the twelve when that is > 0. */
pvq_status pvq_chroma_row(float min_freq, uint32_t n_buckets, uint16_t buckets_per_octave, const float *x_vqt_smoothed,
                          float out12[12]);

/* The same for MANY rows on the GPU: a row is one frame of one stream, the inputs are the arrays pvq_analysis_batch_outputs
 * describes, flattened to n_rows = n_streams * n_frames, so PCM -> VQT -> AnalysisState::preprocess -> picture never leaves the
 * device.  Same arithmetic in the same f32 operation order as the three host functions; the device's powf / expf / cosf / sinf
 * are what may differ (a byte one level apart where a product sits on an integer, chroma to ~1e-6 relative). */
typedef struct pvq_render_batch pvq_render_batch;
/* per-row results, DEVICE pointers, any may be NULL */
typedef struct pvq_render_outputs {
    uint8_t *spectrogram_vqt;    /* [n_rows][n_bins][4]: pvq_spectrogram_row(PVQ_SPECTROGRAM_VQT); 4-byte aligned */
    uint8_t *spectrogram_peaks;  /* [n_rows][n_bins][4]: pvq_spectrogram_row(PVQ_SPECTROGRAM_PEAKS); 4-byte aligned */
    float *chroma;               /* [n_rows][12]: pvq_chroma_row */
    uint8_t *led;                /* [n_rows][3 + 3 * n_bins]: the bytes of pvq_led_frame (0xFF hi lo, then triples <= 0xFE) */
} pvq_render_outputs;
/* One geometry (VqtRange) and one palette (update.rs:985-992 / pitchvis_serial/src/main.rs:155-160: colors NULL = pitchvis_colors::
 * COLORS; the LED strip's own palette is SERIAL_COLORS with gray 5.0 and easing 2.3, on a handle of its own).  The arguments are
 * checked before any device is touched; takes the bin counts pvq_analysis_batch_create takes (PVQ_ERR_UNSUPPORTED beyond);
 * device_id < 0: a host-only handle whose rows call returns PVQ_ERR_NO_DEVICE after its argument checks. */
pvq_status pvq_render_batch_create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave,
                                   const float *colors, float gray_level, float easing_pow, pvq_render_batch **out);
void pvq_render_batch_destroy(pvq_render_batch *r);
/* update.rs:961-1065, :1102-1131 and pitchvis_serial/src/main.rs:122-175 for n_rows rows.  d_x_vqt_smoothed [n_rows][n_bins];
 * d_center / d_size [n_rows][max_peaks] with d_peak_count [n_rows] (a count above max_peaks is taken as max_peaks) — device
 * pointers.  Inputs an output does not read may be NULL; PVQ_ERR_INVALID_ARG for a requested output whose inputs are missing
 * (spectrogram_vqt / chroma without x_vqt_smoothed; spectrogram_peaks / led without center, size, peak_count or with
 * max_peaks == 0).  Asynchronous on `stream`; the handle keeps no state between calls, calls on several streams may overlap. */
pvq_status pvq_render_batch_rows_device(pvq_render_batch *r, size_t n_rows, const float *d_x_vqt_smoothed, const float *d_center,
                                        const float *d_size, const uint32_t *d_peak_count, uint32_t max_peaks,
                                        const pvq_render_outputs *outs, void *stream);

/* ---- the viewer's main picture: pitch balls, bass spiral, bloom --------------------------------------
 * pitchvis_viewer/src/display_system/update.rs:38-426 (update_display) turns an AnalysisState, frame after frame, into
 *   - a ball per bin (setup.rs:89-125) that lights on a peak, fades between frames and hides beside a stronger neighbour,
 *   - the bass spiral (setup.rs:127-172) lit up to the lowest note,
 *   - the bloom intensity, driven by the scene's calmness.
 * Unlike the render stage above the scene is STATEFUL: a ball's scale, alpha and depth carry from frame to frame
 * (fade_pitch_balls, update.rs:136-178), and a frame without peaks leaves balls, bass spiral and bloom as the previous frame left
 * them (the early return at update.rs:85-87).
 *
 * Construction (setup.rs:89-125, :127-172, util.rs:3-20): ball idx sits at bin_to_spiral(bpo, idx) with z = -0.01; its scale is 3.0
 * and it is visible if idx % 17 == 0, otherwise scale 0 and hidden; its colour is LinearRgba::from(Color::srgb(1.0, 0.7, 0.6)), its
 * params {calmness 0, pitch_accuracy 0, pitch_deviation 0}.  The bass spiral has min(octaves * 72, 168) - 1 segments, all hidden,
 * colour srgb(0.8, 0.7, 0.6).  Bloom intensity starts at 0 (the reference leaves Bevy's default there until the first frame with
 * peaks).
 *
 * One frame with (peaks_continuous, calmness[], pitch_accuracy[], pitch_deviation[], scene_calmness, dt), in this order:
 *  1. fade (update.rs:147-178), every ball: size = scale / F; if size * F >= 0.019 { visible; size *= dropoff; scale = size * F;
 *     alpha = max(alpha * dropoff, 0.7); z -= 0.001 * 30.0 * dt }; if size * F < 0.019 { hidden }, with F = 1.0f / 305.0f and
 *     dropoff = (0.85 - 0.15 * (idx as f32 / n as f32)).powf(30 * dt).
 *  2. no peaks: return, nothing else changes (update.rs:85-87).
 *  3. update_pitch_balls (update.rs:199-334): max_size by util::arg_max (first wins); balls keyed by trunc(center) as usize, the
 *     LATER list entry of a key wins (HashMap::insert); translation (bin_to_spiral(bpo, center).xy, (size / max_size - 1.01) * 12.5);
 *     colour LinearRgba::from(Color::srgba(r, g, b, 1 - (1 - size / max_size).powf(2.0))) with (r, g, b) = calculate_color at
 *     (center + (bpo - 3 (bpo / 12))) % bpo, clamped to 0..1 (r, g, b only, update.rs:276-284); params calmness =
 *     clamp(calmness[idx] - 0.27, 0, 1), pitch_accuracy[idx], pitch_deviation[idx] (both DisplayMode variants take this branch);
 *     scale = size * (Performance ? 0.7 : 1.0) * F * (1 + 0.2 * calmness), visible if scale >= 0.002.  Hide pass (update.rs:307-330):
 *     radius = (bpo / 12) as f32 * 0.23; the bins round(center - radius).max(0) ..= round(center + radius).min(n - 1) of every entry
 *     the map kept are marked, the keyed bins unmarked; visible marked balls become hidden and keep their scale.
 *     A peak with trunc(center) >= n_bins is ignored (the reference would index out of range); it still counts for max_size.
 *  4. update_bloom (update.rs:336-351): 0 when bloom is disabled or the mode is Performance, else clamp(scene_calmness * 1.3, 0, 1).
 *  5. update_bass_spiral (update.rs:369-425): all segments hidden; nothing more in Galaxy mode; otherwise, from the FIRST peak,
 *     c = center / bpo * 12; nothing is lit if round(c) * 6 >= n_segments; otherwise segments [0, (round(c) * 6) as usize) are lit, all
 *     in one colour: calculate_color at (round(c) * bpo / 12 + (bpo - 3 (bpo / 12))) % bpo with alpha 1 - (1 - size / max_size)^2 — a
 *     Color, not converted to linear.  The visible state is (lit count, rgba); rgba keeps its last value while nothing is lit.
 *  6. The `ml` branch (update.rs:247-255, display_system/util.rs:23-31), only through the pvq_ml_ entry points below with a non-NULL
 *     probability row (AnalysisState::ml_midi_base_pitches [128], what pvq_note_model_outputs.d_prob holds).  For a ball the frame
 *     keys (idx = trunc(center) < n_bins, the later list entry winning as in step 3): m = (uint) round((idx as f32 / bpo as f32) *
 *     12.0) + 33, the division and the product each rounded to f32, round half away from zero, 33 = FREQ_A1_MIDI_KEY_ID.  m <= 127:
 *     alpha = prob[m] > 0.35 ? 1.0 : color_coefficient * 0.1 (one f32 product; a NaN probability takes the dim side).  m > 127 (the
 *     reference's None): alpha stays color_coefficient.  Nothing else changes: the bass spiral's alpha, scale, z, the hide pass and
 *     the fade are as above — so the fade's max(alpha * dropoff, 0.7) lifts a dim ball to 0.7 on its next frame, as in the viewer.
 *     A row of zeros reads as "nothing inferred", like the reference's initial vec![0.0; 128].
 * Left out: params.time (the caller's clock).  The debug meshes (update_spectrum, the calmness histogram and graph) are the panels stage below.
 * Every libm call of steps 3 and 5 is the double-precision function rounded once to f32, on the host and on the device (DESIGN.md
 * 6c); the fade's powf is the host's, also for the device stage. */
typedef enum pvq_visuals_mode { PVQ_VISUALS_FULL = 0, PVQ_VISUALS_ZEN = 1, PVQ_VISUALS_PERFORMANCE = 2, PVQ_VISUALS_GALAXY = 3 } pvq_visuals_mode;
/* fixed at create; a change needs a new handle (as a palette does for pvq_render_batch_create) */
typedef struct pvq_scene_settings {
    int visuals_mode;          /* pvq_visuals_mode (SettingsState::visuals_mode) */
    int enable_bloom;          /* SettingsState::enable_bloom */
    const float *colors;       /* 12 RGB triples in [0, 1]; NULL: pitchvis_colors::COLORS */
    float gray_level, easing_pow;   /* GRAY_LEVEL 60.0, EASING_POW 1.3 (lib.rs:56-57) */
} pvq_scene_settings;
void pvq_scene_default_settings(pvq_scene_settings *s);   /* Full, bloom on, COLORS, 60.0, 1.3 */

/* One stream on the host: the one-stream face of the stage, in the manner of pvq_analysis_state_*.  settings NULL: the defaults.
 * PVQ_ERR_INVALID_ARG for octaves or buckets_per_octave 0 or an unknown mode. */
typedef struct pvq_scene_state pvq_scene_state;
pvq_status pvq_scene_state_create(uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings *settings,
                                  pvq_scene_state **out);
void pvq_scene_state_destroy(pvq_scene_state *s);
uint32_t pvq_scene_state_n_bins(const pvq_scene_state *s);
uint32_t pvq_scene_state_n_segments(const pvq_scene_state *s);   /* min(octaves * 72, 168) - 1 */
/* replaces update_display (update.rs:38-134) for one frame: center / size [n_peaks] (peaks_continuous, in list order), calmness /
 * pitch_accuracy / pitch_deviation [n_bins], smoothed_scene_calmness, and the frame's Time::delta in nanoseconds */
pvq_status pvq_scene_state_update(pvq_scene_state *s, const float *center, const float *size, uint32_t n_peaks,
                                  const float *calmness, const float *pitch_accuracy, const float *pitch_deviation,
                                  float scene_calmness, uint64_t frame_time_ns);
/* The same frame with step 6: ml_prob [128] (HOST), the frame's ml_midi_base_pitches.  ml_prob NULL: pvq_scene_state_update, bit
 * for bit. */
pvq_status pvq_ml_scene_state_update(pvq_scene_state *s, const float *center, const float *size, uint32_t n_peaks,
                                     const float *calmness, const float *pitch_accuracy, const float *pitch_deviation,
                                     float scene_calmness, uint64_t frame_time_ns, const float *ml_prob);
/* step 6's pitch of a bin (util.rs:23-31 bin_to_midi_pitch): PVQ_OK and *out_pitch <= 127, or *out_pitch = UINT32_MAX for None.
 * PVQ_ERR_INVALID_ARG for buckets_per_octave 0 or a NULL out_pitch. */
pvq_status pvq_ml_midi_pitch(uint32_t buckets_per_octave, uint32_t bin, uint32_t *out_pitch);
/* the scene as it stands; any pointer may be NULL.  ball_xyzs [n_bins][4]: x, y, z, scale; ball_rgba [n_bins][4] (linear r, g, b and
 * alpha); ball_params [n_bins][3]: calmness, pitch_accuracy, pitch_deviation; ball_visible [ceil(n_bins / 32)]: bit bin % 32 of word
 * bin / 32 (the bit order of peak_mask); bass_lit: the number of lit segments; bass_rgba [4]; bloom: Bloom::intensity */
pvq_status pvq_scene_state_get(const pvq_scene_state *s, float *ball_xyzs, float *ball_rgba, float *ball_params,
                               uint32_t *ball_visible, uint32_t *bass_lit, float *bass_rgba, float *bloom);

/* The same for MANY streams on the GPU: n_streams scenes in one handle, their state kept on the device between calls, so PCM ->
 * VQT -> AnalysisState::preprocess -> scene never leaves the device.  A frame-parallel kernel turns every peak into a finished
 * record (all the libm of a frame), a wavefront per stream then fades and applies records frame after frame.  scale, z, the visible
 * mask, the params, bass_lit and bloom carry the bits of pvq_scene_state_update; x, y and the colours too but for a libm rounding. */
typedef struct pvq_scene_batch pvq_scene_batch;
/* per-frame inputs, DEVICE pointers laid out as pvq_analysis_batch_outputs describes: center / size [n_streams][n_frames][max_peaks]
 * with peak_count [n_streams][n_frames] (a count above max_peaks is taken as max_peaks); calmness / pitch_accuracy / pitch_deviation
 * [n_streams][n_frames][n_bins]; scene_calmness [n_streams][n_frames].  All are needed. */
typedef struct pvq_scene_inputs {
    const float *center, *size;
    const uint32_t *peak_count;
    uint32_t max_peaks;
    const float *calmness, *pitch_accuracy, *pitch_deviation, *scene_calmness;
} pvq_scene_inputs;
/* per-frame results, DEVICE pointers, any may be NULL: the scene after each frame, as pvq_scene_state_get gives it */
typedef struct pvq_scene_outputs {
    float *ball_xyzs;        /* [n_streams][n_frames][n_bins][4]; 16-byte aligned */
    float *ball_rgba;        /* [n_streams][n_frames][n_bins][4]; 16-byte aligned */
    float *ball_params;      /* [n_streams][n_frames][n_bins][3] */
    uint32_t *ball_visible;  /* [n_streams][n_frames][ceil(n_bins / 32)] */
    uint32_t *bass_lit;      /* [n_streams][n_frames] */
    float *bass_rgba;        /* [n_streams][n_frames][4]; 16-byte aligned */
    float *bloom;            /* [n_streams][n_frames] */
} pvq_scene_outputs;
/* n_streams scenes as constructed above on device_id.  The arguments are checked before any device is touched; takes the bin counts
 * pvq_analysis_batch_create takes, 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond); device_id < 0: a host-only handle whose frames call
 * returns PVQ_ERR_NO_DEVICE after its argument checks. */
pvq_status pvq_scene_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings *settings,
                                  uint32_t n_streams, pvq_scene_batch **out);
void pvq_scene_batch_destroy(pvq_scene_batch *b);
uint32_t pvq_scene_batch_n_segments(const pvq_scene_batch *b);
/* Every stream advances by n_frames frames, in order.  frame_time_ns applies to every frame unless frame_times_ns (HOST array of
 * n_frames) is given.  PVQ_ERR_INVALID_ARG for a missing input, max_peaks == 0 or a misaligned output, before anything is launched.
 * Asynchronous on `stream`, one handle's calls are stream-ordered — except that a call whose frame time differs from the previous
 * call's, or that brings per-frame times, first waits for `stream` (the fade table, built with the host's libm, is replaced). */
pvq_status pvq_scene_batch_frames_device(pvq_scene_batch *b, size_t n_frames, const pvq_scene_inputs *in, uint64_t frame_time_ns,
                                         const uint64_t *frame_times_ns, const pvq_scene_outputs *outs, void *stream);
/* The same frames with step 6.  d_ml_prob (DEVICE) is [n_streams][ml_stride_frames][128]: row (s, f) reads
 * d_ml_prob[(s * ml_stride_frames + f) * 128 + m], so the d_prob buffer pvq_note_model_rows_device or
 * pvq_note_model_rows_carry_device wrote is taken where it lies, whatever its stride_frames.  ml_stride_frames < n_frames is
 * PVQ_ERR_INVALID_ARG; rows f >= n_frames are never read.  d_ml_prob NULL: pvq_scene_batch_frames_device, bit for bit (the stride is
 * not looked at).  Alpha carries the bits of pvq_ml_scene_state_update. */
pvq_status pvq_ml_scene_batch_frames_device(pvq_scene_batch *b, size_t n_frames, const pvq_scene_inputs *in,
                                            const float *d_ml_prob, size_t ml_stride_frames, uint64_t frame_time_ns,
                                            const uint64_t *frame_times_ns, const pvq_scene_outputs *outs, void *stream);
/* the state of one stream after the last call (synchronises), laid out as pvq_scene_state_get */
pvq_status pvq_scene_batch_get_state(pvq_scene_batch *b, uint32_t stream_index, float *ball_xyzs, float *ball_rgba,
                                     float *ball_params, uint32_t *ball_visible, uint32_t *bass_lit, float *bass_rgba, float *bloom);

/* ---- the pitch balls as pixels: the ball material's fragment, z-order, alpha blend -------------------------------
 * What the viewer's renderer makes of the ball records the scene stage above produces — the last data-parallel piece of its
 * per-frame work.  Restated from behaviour, all of it f32 without FMA contraction, components left to right; sin, cos and atan2
 * are the double-precision functions rounded once to f32, sqrt and `/` IEEE f32, so the host face and the device carry the same
 * bits (DESIGN.md 6e has the table of the WGSL built-ins and the Bevy semantics assumed).
 *
 *  - The material (pitchvis_viewer/src/display_system/material.rs:33-35 names assets/shaders/noisy_color_rings_2d.wgsl; its
 *    fragment is :395-428): from the ball's linear rgba and (calmness, time, pitch_accuracy, pitch_deviation), at mesh uv (u, v)
 *    with p = 2 uv - 1 and r = |p|: noise = clamp(simplex3(4.3 u, 4.3 v, 0.8 time) - 0.15, 0, 1) (:408-409; the 3-D simplex noise
 *    of McEwan and Gustavson, :6-75); ring = sin(r sqrt(r) PI)^2 (:116-120); ring colour (mix(rgb, 1, noise calmness ring), a ring)
 *    (:413); the centre dot for pitch_accuracy >= 0.85 (:126-141) and the six-armed tuning star for 0.01 <= r <= 0.25 (:231-260)
 *    added with strength 0.4 (:422-423); the result mixed with the plain colour by clamp(1 - 1.65 calmness, 0, 1)^3 (:426-427); the
 *    rim smoothstep(0.96, 1, r) towards alpha 0 (:100-102).  Alpha is exactly 0 where r >= 1: such pixels are left untouched.
 *  - A ball is a 20 x 20 rectangle (setup.rs:110-112) scaled by `scale` at (x, y); mesh v runs downwards.
 *  - The camera (setup.rs:359-365) is orthographic, FixedVertical: 38 * 0.41421357 world units over the image height, centred on
 *    the origin; pixel (i, j) is column i, row j with row 0 at the top, sampled at its centre.
 *  - Composition: the clear colour LinearRgba::from(srgb(0.23, 0.23, 0.25)), in Galaxy mode srgb(0.05, 0, 0.05) (mod.rs:19-21,
 *    update.rs:914-915), alpha 1 — or the caller's background; then the balls back to front, ascending z, ties by ascending bin
 *    (assumed for Bevy's Transparent2d sort), each blended as AlphaMode2d::Blend: rgb = src.rgb src.a + dst.rgb (1 - src.a),
 *    a = src.a + dst.a (1 - src.a).  Not drawn: a ball whose visible bit is clear, whose scale is <= 0, or one of whose values
 *    (x, y, z, scale, rgba, the three params, time) is not finite.
 *  - params.time is per-ball state: update_pitch_balls sets it to Time::elapsed_secs() only for the balls a peak keys in the frame
 *    (update.rs:239), so a fading ball's noise and pulses freeze.  It starts at 0 (Params::default()).
 * The output is the linear HDR target before bloom and tone mapping, f32 [H][W][4]; bloom, the display transform and the sRGB
 * bytes are the present stage further down, which takes that target.
 * Left out: noisy_color_2d.wgsl, which nothing references.  The spider net, the bass spiral and the debug panels are the backdrop stage further down, which draws the picture the
 * balls go over, the spectrogram quad and the chroma boxes the overlay stage after it, which draws in front of the balls; the
 * pitch-name text the text stage between the two, which draws over the balls and under the overlay; the other parts the backdrop
 * section lists stay left out. */
/* one fragment: rgba linear, params = (calmness, time, pitch_accuracy, pitch_deviation) */
pvq_status pvq_raster_shade(const float *rgba, const float *params, float u, float v, float *out4);
/* the time update of one frame: every entry of the list sets time[trunc(center)] = elapsed (keys >= n_bins are ignored, as the
 * scene ignores them).  time_inout [n_bins]. */
pvq_status pvq_raster_touch(uint32_t n_bins, const float *center, uint32_t n_peaks, float elapsed, float *time_inout);
/* One frame on the host.  ball_xyzs / ball_rgba [n_bins][4], ball_params [n_bins][3], ball_visible [ceil(n_bins / 32)] as
 * pvq_scene_state_get gives them, ball_time [n_bins]; viewport_height 0: the viewer's; background [height][width][4] or NULL: the
 * clear colour of visuals_mode.  image_out [height][width][4].  width, height 1 .. 4096. */
pvq_status pvq_raster_frame(uint32_t n_bins, uint32_t width, uint32_t height, float viewport_height, int visuals_mode,
                            const float *ball_xyzs, const float *ball_rgba, const float *ball_params, const uint32_t *ball_visible,
                            const float *ball_time, const float *background, float *image_out);

/* The same for MANY streams on the GPU, fed with what pvq_scene_batch_frames_device leaves in device memory.  The handle keeps
 * every ball's time between calls. */
typedef struct pvq_raster_batch pvq_raster_batch;
/* DEVICE pointers laid out as pvq_scene_outputs and pvq_scene_inputs lay them out.  center, peak_count and max_peaks are always
 * needed (a count above max_peaks is taken as max_peaks); the four ball arrays when an image is asked for. */
typedef struct pvq_raster_inputs {
    const float *ball_xyzs;        /* [n_streams][n_frames][n_bins][4]; 16-byte aligned */
    const float *ball_rgba;        /* [n_streams][n_frames][n_bins][4]; 16-byte aligned */
    const float *ball_params;      /* [n_streams][n_frames][n_bins][3] */
    const uint32_t *ball_visible;  /* [n_streams][n_frames][ceil(n_bins / 32)] */
    const float *center;           /* [n_streams][n_frames][max_peaks] */
    const uint32_t *peak_count;    /* [n_streams][n_frames] */
    uint32_t max_peaks;
    const float *background;       /* optional: [height][width][4], shared by all rows; 16-byte aligned */
} pvq_raster_inputs;
/* The arguments are checked before any device is touched: bin counts 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond), width and height
 * 1 .. 4096, viewport_height 0 (the viewer's) or positive and finite — at seven octaves the spiral reaches radius 9.2 and the
 * viewer's view only +-7.87, so callers may widen it.  device_id < 0: a host-only handle whose frames call returns
 * PVQ_ERR_NO_DEVICE after its argument checks. */
pvq_status pvq_raster_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                   uint32_t n_streams, uint32_t width, uint32_t height, pvq_raster_batch **out);
void pvq_raster_batch_destroy(pvq_raster_batch *b);
/* n_frames frames of every stream, in order: first frame f's peak list sets the times of its key bins to elapsed_s[f] (HOST array
 * of n_frames, shared by all streams; balls the scene's hide pass hides take it too), then frame f is drawn with those times.
 * d_image (optional) [n_streams][n_frames][height][width][4], 16-byte aligned; d_ball_time (optional) [n_streams][n_frames][n_bins]:
 * the times each frame was drawn with.  PVQ_ERR_INVALID_ARG for a missing input, max_peaks == 0 or a misaligned pointer, before
 * anything is launched.  One handle's calls are stream-ordered; the kernels run asynchronously on `stream`, but every call first
 * waits for `stream` (the frame clocks go through a buffer of the handle), and a call that needs a larger workspace than any
 * before it waits for the device. */
pvq_status pvq_raster_batch_frames_device(pvq_raster_batch *b, size_t n_frames, const pvq_raster_inputs *in, const float *elapsed_s,
                                          float *d_image, float *d_ball_time, void *stream);
/* one stream's ball times after the last call (synchronises); out [n_bins] */
pvq_status pvq_raster_batch_get_times(pvq_raster_batch *b, uint32_t stream_index, float *out);

/* ---- the viewer's debug panels: spectrum line with peak discs, calmness histogram, scene calmness graph ------
 * The three meshes of DisplayMode::Debugging (pitchvis_viewer/src/display_system/update.rs:474-869), the last part of update_display
 * the stages above leave out.  A mesh is positions [vertices][3] (z = 0) and colours [vertices][4]; indices, UVs and the normal
 * (0, 0, 1) of every vertex depend on the counts alone: pvq_panel_topology.  The reference's transforms (the histogram's y flip, the
 * placement relative to the camera), the visibility toggles and the concatenation of line and discs into one mesh stay with the caller.
 *
 * Thick-line quad of a segment (p, q) with thickness t (update.rs:531-541, :691-700, :815-827): dx = p.x - q.x, dy = p.y - q.y,
 * l = dx.hypot(dy), u = dx * t * 0.5 / l, v = dy * t * 0.5 / l; v0 = (p.x + v, p.y - u), v1 = (p.x - v, p.y + u), v2 = (q.x - v,
 * q.y + u), v3 = (q.x + v, q.y - u).  hypot is the double-precision function rounded once to f32.
 *  - Spectrum line (update.rs:506-579), t = 0.02: point i = (i * 0.011, x[i] / 10), n - 1 segments; the four vertices of segment i
 *    carry [r, g, b, 1 - (0.5 - x[i] / max / 2).powf(0.5)] with max = x[util::arg_max(x)] (the first maximum) and (r, g, b) =
 *    calculate_color(bpo, (i + 0.5 + (bpo - 3 (bpo / 12))) % bpo, colors, gray_level, 10.0); powf(0.5) is the correctly rounded sqrt.
 *  - Peak discs (update.rs:582-615, :435-471), one per entry of peaks_continuous in list order: 13 vertices, the centre (center *
 *    0.011, size / 10), then (cx + 0.08 cos a_i, cy + 0.08 sin a_i) with a_i = (i / 12) * TAU; all carry [r, g, b, 0.9], the colour
 *    above at bucket (center.round() as usize) % bpo.
 *  - Calmness histogram (update.rs:787-845), t = 0.01: p = (i * 0.011, c[i] * 0.5), q = ((i + 1) * 0.011, c[i + 1] * 0.5); colour by
 *    (c[i] + c[i + 1]) / 2: > 0.7 (0.5, 0.8, 1.0, 1.0), > 0.3 (1.0, 1.0, 0.5, 1.0), else (1.0, 0.5, 0.5, 1.0).  Always n - 1 quads:
 *    the reference's `l < 0.0001` skip cannot fire at a point spacing of 0.011.
 *  - Scene calmness graph (update.rs:652-718), t = 0.01, capacity C (300 in the viewer): after pushing the frame's value, point i =
 *    (i / C - 0.5, h[i]) with h the last C pushed values, oldest first, zeros where nothing was pushed; C - 1 segments, segment i
 *    coloured by the class of h[i]. */

/* One stream on the host.  colors: 12 RGB triples in [0, 1].  Any output may be NULL.  line_pos [4 (n - 1)][3], line_rgba
 * [4 (n - 1)][4], disc_pos [n_peaks][13][3], disc_rgba [n_peaks][13][4].  PVQ_ERR_INVALID_ARG for n_buckets < 2,
 * buckets_per_octave == 0, colors NULL or a requested output whose input is missing. */
pvq_status pvq_spectrum_mesh(uint32_t n_buckets, uint16_t buckets_per_octave, const float *x_vqt_smoothed, const float *center,
                             const float *size, uint32_t n_peaks, const float *colors, float gray_level, float *line_pos,
                             float *line_rgba, float *disc_pos, float *disc_rgba);
/* pos [4 (n - 1)][3], rgba [4 (n - 1)][4]; either may be NULL */
pvq_status pvq_calmness_histogram_mesh(uint32_t n_buckets, const float *calmness, float *pos, float *rgba);
/* the graph and its history ring (SceneCalmnessHistory, mod.rs:114-133).  capacity 2 .. 1024, 0: 300 */
typedef struct pvq_calmness_graph pvq_calmness_graph;
pvq_status pvq_calmness_graph_create(uint32_t capacity, pvq_calmness_graph **out);
void pvq_calmness_graph_destroy(pvq_calmness_graph *g);
uint32_t pvq_calmness_graph_capacity(const pvq_calmness_graph *g);
pvq_status pvq_calmness_graph_push(pvq_calmness_graph *g, float value);
/* pos [4 (C - 1)][3], rgba [4 (C - 1)][4], history [C] (oldest first); any may be NULL */
pvq_status pvq_calmness_graph_mesh(const pvq_calmness_graph *g, float *pos, float *rgba, float *history);
/* n_quads quads followed by n_circles discs: indices [6 n_quads + 36 n_circles] (a quad with base b: b+2, b+1, b, b+2, b, b+3; a
 * disc with base b: triangles (b, b+1+i, b+1+(i+1)%12)), uvs [4 n_quads + 13 n_circles][2] ((0,1), (0,0), (1,0), (1,1) per quad;
 * (0.5, 0.5), then (0.5 + 0.5 cos a_i, 0.5 + 0.5 sin a_i) per disc).  Either may be NULL. */
pvq_status pvq_panel_topology(uint32_t n_quads, uint32_t n_circles, uint32_t *indices, float *uvs);

/* The same for MANY streams on the GPU, from the arrays pvq_analysis_batch_outputs describes.  The device evaluates only IEEE + - * /
 * and sqrt on the host's inputs and tables: every output carries the bits of the host functions above. */
typedef struct pvq_panels_batch pvq_panels_batch;
/* per-row results, DEVICE pointers, any may be NULL.  Line and disc parts are separate arrays (the caller draws both, the disc
 * indices offset), so a row's line part stays a multiple of 16 bytes. */
typedef struct pvq_panels_outputs {
    float *line_pos;    /* [n_rows][4 (n_bins - 1)][3]; 16-byte aligned */
    float *line_rgba;   /* [n_rows][4 (n_bins - 1)][4]; 16-byte aligned */
    float *disc_pos;    /* [n_rows][max_peaks][13][3]; slots beyond a row's count are zeros (degenerate triangles) */
    float *disc_rgba;   /* [n_rows][max_peaks][13][4]; likewise */
    float *hist_pos;    /* [n_rows][4 (n_bins - 1)][3]; 16-byte aligned */
    float *hist_rgba;   /* [n_rows][4 (n_bins - 1)][4]; 16-byte aligned */
} pvq_panels_outputs;
/* One geometry, one palette (colors NULL: pitchvis_colors::COLORS), n_streams graph histories of graph_capacity values (2 .. 1024,
 * 0: 300), all zeros.  The arguments are checked before any device is touched; takes the bin counts pvq_analysis_batch_create takes,
 * 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond); device_id < 0: a host-only handle whose device calls return PVQ_ERR_NO_DEVICE after their
 * argument checks. */
pvq_status pvq_panels_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const float *colors, float gray_level,
                                   uint32_t n_streams, uint32_t graph_capacity, pvq_panels_batch **out);
void pvq_panels_batch_destroy(pvq_panels_batch *b);
uint32_t pvq_panels_batch_graph_capacity(const pvq_panels_batch *b);
/* Spectrum and histogram meshes of n_rows rows (n_streams * n_frames, flattened as for pvq_render_batch_rows_device); stateless.
 * d_x_vqt_smoothed / d_calmness [n_rows][n_bins]; d_center / d_size [n_rows][max_peaks] with d_peak_count [n_rows] (a count above
 * max_peaks is taken as max_peaks; list entries beyond a row's count are never read).  Inputs an output does not read may be NULL;
 * PVQ_ERR_INVALID_ARG for a requested output whose inputs are missing or that is misaligned, before anything is launched.
 * Asynchronous on `stream`; calls on several streams may overlap. */
pvq_status pvq_panels_batch_rows_device(pvq_panels_batch *b, size_t n_rows, const float *d_x_vqt_smoothed, const float *d_center,
                                        const float *d_size, const uint32_t *d_peak_count, uint32_t max_peaks,
                                        const float *d_calmness, const pvq_panels_outputs *outs, void *stream);
/* The graph: stateful, the handle keeps every stream's last C values between calls.  d_scene_calmness [n_streams][n_frames]; every
 * stream's history advances by all n_frames values; meshes are written for frames first_emitted .. n_frames - 1 only (a viewer
 * draws the newest): graph_pos [n_streams][n_frames - first_emitted][4 (C - 1)][3], graph_rgba [..][..][4 (C - 1)][4], 16-byte
 * aligned, either may be NULL.  Asynchronous on `stream`; one handle's calls are stream-ordered. */
pvq_status pvq_panels_batch_graph_device(pvq_panels_batch *b, size_t n_frames, const float *d_scene_calmness, size_t first_emitted,
                                         float *graph_pos, float *graph_rgba, void *stream);
/* one stream's history after the last call, oldest first, out [C] (synchronises) */
pvq_status pvq_panels_batch_get_history(pvq_panels_batch *b, uint32_t stream_index, float *out);

/* ---- the backdrop: spider net, debug panels and lit bass spiral as pixels, the picture the balls go over -------
 * The rest of the 2-D layer of setup_display (pitchvis_viewer/src/display_system/setup.rs, update.rs).  Every layer is a list of
 * flat-coloured triangles in world units, seen by the raster section's camera (orthographic, viewport_height over the image height,
 * pixel centres, row 0 at the top) and blended with its blend into linear f32, back to front:
 *  0. the clear colour of the mode, or the caller's shared background;
 *  1. the net spiral (setup.rs:208-222): thick-line quads (mod.rs:277-306, thickness 0.05) between consecutive points of
 *     calculate_spiral_points(octaves, 72), 72 octaves - 1 quads, LinearRgba::from(srgb(0.3, 0.3, 0.3)), alpha 1 — an opaque
 *     material, so it is drawn first;
 *  2. the net rays (setup.rs:181-206): 12 thick-line quads from the origin to radius octaves as f32 * 2.2 at angle i / 12 * 2 PI,
 *     thickness 0.05, the same grey;
 *  3. the spectrum line, n_bins - 1 quads, then a 12-triangle fan for each of the row's peak discs;
 *  4. the scene-calmness graph, C - 1 quads;
 *  5. the calmness histogram, n_bins - 1 quads;
 *  6. the lit bass segments (setup.rs:127-172, update.rs:369-425): segments [0, bass_lit) of min(72 octaves, 168) - 1 rectangles,
 *     each 0.05 wide and h + 0.01 long, centred on the midpoint of consecutive spiral points p, q with h = |p - q| and the long
 *     axis along p - q, coloured LinearRgba::from(srgba(bass_rgba)) with the alpha as it is.  A bass_lit above the segment count is
 *     taken as the segment count.
 *  7. the balls: the raster stage, unchanged, through pvq_backdrop_balls_over_device or the background argument of its host face.
 * Layers 1, 2 and 6 are absent in Galaxy mode (update.rs:888-895, :374-376).  Layers 3 - 5 are meshes as the panels section lays
 * them out, drawn where their pointers are given; vertex colours are linear and not converted, a triangle takes the colour of its
 * quad's first vertex or of its disc's centre.  Each of them carries its own transform (tx, ty, sx, sy), applied as x * sx + tx,
 * y * sy + ty; pvq_backdrop_panel_transforms gives the reference's.  Within a mesh the triangles are blended in index order, the
 * topology being pvq_panel_topology's: quad triangles (2, 1, 0), (2, 0, 3), disc fans.  Neighbouring line quads overlap at their
 * joints and are blended twice there, as the reference's GPU would.  The static geometry goes through bin_to_spiral with every
 * libm call the double-precision function rounded once to f32; it is built once on the host, for the device stage too.
 *
 * The coverage rule — one rule, carried bit for bit by the test model, the host face and the device; f32 without FMA contraction.
 * One sample per pixel at its centre p (Msaa::Off).  Both windings are drawn (the 2-D mesh pipeline does not cull, and the
 * histogram's sy = -1 flips its winding).  An edge is evaluated from its canonically ordered endpoints, lo being the endpoint with
 * the smaller x, then the smaller y:
 *     e = (hi.x - lo.x) * (p.y - lo.y) - (hi.y - lo.y) * (p.x - lo.x)
 * so two triangles that share an edge compute the same number for it.  A triangle's sign for an edge is the sign of e at its third
 * vertex.  A pixel is inside when, for all three edges, e has the triangle's sign, or e == 0 and the triangle's sign is positive:
 * an edge through a pixel centre goes to exactly one of the two triangles beside it.  A triangle with a zero or non-finite sign, a
 * non-finite vertex (after its transform) or a non-finite colour draws nothing.  Pixel boxes are an acceleration only and err
 * outwards.
 *
 * Left out: MSAA other than the backdrop's own (the pvq_msaa_ entries below, samples = 4; the border pixels of the overlay's
 * spectrogram quad stay one-sample); a ball whose z has fallen below -12.7, which in the
 * reference would go under the bass spiral — here the balls are always on top (at keying z >= -12.625, and the fade lowers it by
 * 0.03 per second while the ball lives).  The pitch-name text at z = -0.02 is the text stage below (the caller brings the font),
 * the spectrogram quad at z = 5 and the chroma boxes are the overlay stage after it, bloom and tone mapping the present stage after
 * that (which names what stays out of the displayed picture: MSAA of the overlay quad's border, the deband dither and a draw of
 * the boxes in display space). */
enum { PVQ_BACKDROP_NET_SPIRAL = 0, PVQ_BACKDROP_NET_RAYS = 1, PVQ_BACKDROP_BASS = 2 };
/* the static quads of one layer: quads_out [n][4][2] (v0 .. v3 as x, y; triangles (2, 1, 0), (2, 0, 3)), n_out: their number —
 * 72 octaves - 1, 12, min(72 octaves, 168) - 1.  Either may be NULL.  octaves 1 .. 1024. */
pvq_status pvq_backdrop_geometry(uint32_t octaves, int what, float *quads_out, uint32_t *n_out);
/* the reference's transforms, out [3][4]: spectrum (max.x - n_bins * 0.011 - 0.2, max.y - 4.2, 1, 1) with max = (vh / 2 * W / H,
 * vh / 2) (update.rs:496-500), histogram the same with sy = -1 (:776-781), graph (-5, -6.5, 3, 1) (setup.rs:284-288).
 * viewport_height 0: the viewer's. */
pvq_status pvq_backdrop_panel_transforms(uint32_t n_bins, uint32_t width, uint32_t height, float viewport_height, float *out);
/* The rule's one-mesh face: n_triangles triangles, pos [n][3][2], rgba [n][4] (linear), blended in index order into image_inout
 * [height][width][4]; transform [4] or NULL.  width, height 1 .. 4096; viewport_height 0: the viewer's. */
pvq_status pvq_backdrop_draw_mesh(uint32_t width, uint32_t height, float viewport_height, size_t n_triangles, const float *pos,
                                  const float *rgba, const float *transform, float *image_inout);
/* the panels of one frame, HOST pointers as pvq_spectrum_mesh, pvq_calmness_histogram_mesh and pvq_calmness_graph_mesh fill them;
 * a mesh is drawn where its pos and rgba are given (PVQ_ERR_INVALID_ARG for one without the other, or a graph with a capacity
 * below 2) */
typedef struct pvq_backdrop_panels {
    const float *line_pos, *line_rgba;   /* [4 (n_bins - 1)][3], [..][4] */
    const float *disc_pos, *disc_rgba;   /* [n_peaks][13][3], [..][13][4] */
    uint32_t n_peaks;
    const float *hist_pos, *hist_rgba;
    const float *graph_pos, *graph_rgba; /* [4 (C - 1)][3], [..][4] */
    uint32_t graph_capacity;
    float spectrum_transform[4], histogram_transform[4], graph_transform[4];   /* tx, ty, sx, sy */
} pvq_backdrop_panels;
/* One frame on the host: layers 0 - 6.  bass_rgba [4] (needed with bass_lit > 0), panels NULL: none; background [height][width][4]
 * or NULL: the clear colour of visuals_mode.  image_out [height][width][4]. */
pvq_status pvq_backdrop_frame(uint32_t octaves, uint32_t buckets_per_octave, uint32_t width, uint32_t height, float viewport_height,
                              int visuals_mode, uint32_t bass_lit, const float *bass_rgba, const pvq_backdrop_panels *panels,
                              const float *background, float *image_out);

/* The same for MANY streams on the GPU, fed with what the scene and panels stages leave in device memory.  Stateless. */
typedef struct pvq_backdrop_batch pvq_backdrop_batch;
/* DEVICE pointers laid out as pvq_scene_outputs and pvq_panels_outputs lay them out, a row being (stream, frame); the graph as
 * pvq_panels_batch_graph_device writes it with first_emitted == 0.  Every group is optional: bass_lit with bass_rgba; line_pos with
 * line_rgba; disc_pos with disc_rgba, peak_count and max_peaks > 0 (a count above max_peaks is taken as max_peaks; slots beyond a
 * row's count are not drawn); hist_pos with hist_rgba; graph_pos with graph_rgba and graph_capacity >= 2.  The rgba arrays, bass_rgba
 * and background are 16-byte aligned. */
typedef struct pvq_backdrop_inputs {
    const uint32_t *bass_lit;     /* [n_streams][n_frames] */
    const float *bass_rgba;       /* [n_streams][n_frames][4] */
    const float *line_pos, *line_rgba;
    const float *disc_pos, *disc_rgba;
    const uint32_t *peak_count;   /* [n_streams][n_frames] */
    uint32_t max_peaks;
    const float *hist_pos, *hist_rgba;
    const float *graph_pos, *graph_rgba;
    uint32_t graph_capacity;
    float spectrum_transform[4], histogram_transform[4], graph_transform[4];   /* tx, ty, sx, sy */
    const float *background;      /* optional: [height][width][4], shared by all rows */
} pvq_backdrop_inputs;
/* Takes the argument ranges of pvq_raster_batch_create and checks them before any device is touched; device_id < 0: a host-only
 * handle whose frames call returns PVQ_ERR_NO_DEVICE after its argument checks. */
pvq_status pvq_backdrop_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                     uint32_t n_streams, uint32_t width, uint32_t height, pvq_backdrop_batch **out);
void pvq_backdrop_batch_destroy(pvq_backdrop_batch *b);
/* Layers 0 - 6 of n_frames frames of every stream into d_image [n_streams][n_frames][height][width][4], 16-byte aligned.
 * PVQ_ERR_INVALID_ARG before anything is launched for a half-given group or a misaligned pointer.  Asynchronous on `stream`; a call
 * that needs a larger workspace than any before it waits for the device. */
pvq_status pvq_backdrop_batch_frames_device(pvq_backdrop_batch *b, size_t n_frames, const pvq_backdrop_inputs *in, float *d_image,
                                            void *stream);
/* Layer 7: pvq_raster_batch_frames_device, except that each row's balls are blended over what d_image_inout already holds for that
 * row (in place: a pixel is read and written by the same lane).  in->background must be NULL and d_image_inout is needed. */
pvq_status pvq_backdrop_balls_over_device(pvq_raster_batch *b, size_t n_frames, const pvq_raster_inputs *in, const float *elapsed_s,
                                          float *d_image_inout, float *d_ball_time, void *stream);

/* ---- the backdrop multisampled: four samples a pixel, resolved at the end of the stage --------------------------------
 * The reference sets Msaa::Off under target_os = "android" only (setup.rs:379-382); its desktop and wasm builds keep Bevy's
 * default, Msaa::Sample4.  The backdrop's triangles are almost all thin (0.05 world units: 2.3 pixels at 1280 x 720, 0.8 at
 * 256 x 256), so nearly every pixel they cover is an edge pixel.  The entries here are the backdrop's faces with a sample count in
 * front; samples is 1 or 4, anything else is PVQ_ERR_INVALID_ARG before anything else is looked at and before any device is
 * touched.  With samples = 1 they give the bits of the one-sample faces above.
 *
 * The rule, samples = 4.  A pixel (i, j) has four samples at these positions, in pixel units from its top-left corner, in this order:
 *     0: (0.375, 0.125)   1: (0.875, 0.375)   2: (0.125, 0.625)   3: (0.625, 0.875)        (samples = 1: (0.5, 0.5))
 * Sample k's world position is the raster section's pixel position with 0.5 replaced by the fractions, f32 without FMA contraction:
 *     s = vh / (float)H;  wx = ((float)i + fx_k - 0.5f * (float)W) * s;  wy = (0.5f * (float)H - ((float)j + fy_k)) * s
 * (i + fx_k is exact: sides <= 4096, fractions in eighths; with (0.5, 0.5) this is the pixel centre bit for bit).  Every sample has a
 * destination of its own, which starts from the clear colour or from the shared background's pixel.  Each sample runs the coverage
 * rule of the section above unchanged at its own position — canonical edges, a tie e == 0 going to the triangle whose sign is
 * positive, so an edge through a sample goes to exactly one of the two triangles beside it — and a covered sample is blended with
 * the triangle's flat colour against its own destination, in list order.  After layer 6 the pixel is resolved, per channel
 *     ((s0 + s1) + (s2 + s3)) * 0.25f
 * in that order: four equal finite samples x with |x| < 2^126 resolve to exactly x; pictures with channels beyond that bound are
 * not promised.  The pixel boxes are those of the one-sample rule: widened by a whole pixel, they hold every pixel with a covered
 * sample, none of which is further than 0.375 pixel from its centre.  No per-sample picture leaves the stage.
 *
 * What is assumed:
 *   sample positions   the standard four-sample pattern; wgpu does not expose the positions, but Vulkan's standard sample
 *                      locations, D3D and Metal share them                                        (confidence: high for desktop)
 *   shading            once per pixel in the reference, per covered sample here: the same for a flat colour
 *   resolve            an unweighted mean of the linear target before bloom: Bevy resolves the main pass's texture before
 *                      post-processing; its target is 16-bit float, ours f32
 *   not multisampled   the balls — the fragment's alpha is exactly 0 at and beyond the unit radius, so the edge of a ball's quad
 *                      never shows; the text, whose coverage is analytic; the chroma boxes, which are UI and which Bevy does not
 *                      multisample.  A layer that covers all four samples of a pixel with one colour and one alpha blends every
 *                      sample by the same affine map, and the mean commutes with an affine map: blending it over the resolved
 *                      picture equals resolving after it, up to rounding.  So the later stages run on the resolved picture as they are.
 *   left out           the border pixels of the overlay's spectrogram quad, the one partial coverage outside the backdrop;
 *                      sample counts other than 1 and 4; a per-sample picture kept after the backdrop; centroid or per-sample
 *                      shading; the deband dither; the UI boxes in display space */
/* xy_out [samples][2]: the positions above */
pvq_status pvq_msaa_sample_positions(uint32_t samples, float *xy_out /* [samples][2] */);
/* The one-mesh face.  image_inout is a resolved picture: every sample starts from its pixel, the mesh is drawn, and the result is
 * resolved back.  The other arguments and their checks are the one-sample face's. */
pvq_status pvq_msaa_draw_mesh(uint32_t samples, uint32_t width, uint32_t height, float viewport_height, size_t n_triangles, const float *pos,
                              const float *rgba, const float *transform, float *image_inout);
/* One frame on the host: layers 0 - 6, resolved.  The other arguments and their checks are the one-frame host face's.  The four
 * sample planes are host memory of 4 x the picture's size for the length of the call. */
pvq_status pvq_msaa_frame(uint32_t samples, uint32_t octaves, uint32_t buckets_per_octave, uint32_t width, uint32_t height,
                          float viewport_height, int visuals_mode, uint32_t bass_lit, const float *bass_rgba,
                          const pvq_backdrop_panels *panels, const float *background, float *image_out);
/* Many streams on the GPU.  The handle is an ordinary backdrop batch handle: the batched backdrop's frames call draws it — with
 * samples = 4 through a tile kernel that keeps a pixel's four samples in registers and stores the resolved pixel, the output bytes
 * being the one-sample call's — and its destroy frees it.  The other arguments and their checks are the batched create's;
 * device_id < 0 makes a host-only handle as there. */
pvq_status pvq_msaa_batch_create(uint32_t samples, int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode,
                                 float viewport_height, uint32_t n_streams, uint32_t width, uint32_t height, pvq_backdrop_batch **out);
/* the sample count a backdrop batch handle was made with (1 for one from the one-sample create); 0 for NULL */
uint32_t pvq_msaa_batch_samples(const pvq_backdrop_batch *b);

/* ---- the overlay: scrolling spectrogram quad and chroma boxes, in front of the balls -------------------------------
 * The last two parts of the DisplayMode::Debugging picture (pitchvis_viewer/src/display_system/setup.rs:418-541, update.rs:929-1172,
 * material.rs:42-71, assets/shaders/spectrogram_scroll.wgsl), blended in place over a finished image of the raster section's camera:
 * layer 8 the quad, layer 9 the boxes.  In the other display modes the caller does not call this stage, and the reference's ring
 * does not advance either.  Restated from behaviour; f32 without FMA contraction, `/` and floor IEEE f32, so the test model, the
 * host face and the device carry the same bits (DESIGN.md 6g has the table of assumed semantics).
 *
 * The texture.  Rgba8UnormSrgb, n_bins wide, history_rows (h, 200 in the viewer) high, all zeros at start, sampled nearest with
 * clamp-to-edge.  A frame's row — what pvq_spectrogram_row returns, in either mode — is written to texture row h - 1 - write_index;
 * then the row of next = (write_index + 1) % h is zeroed, write_index = next, and the material's scroll_offset = next as f32 / h as f32.
 *
 * The rule, per pixel (i, j) with (wx, wy) its centre's world position as the raster section places it:
 *  8. the quad (cx, cy, ex, ey) — centre, extent along x (time) and along y (frequency); the reference's is (-7, 6, 12,
 *     12 * (h as f32 / n_bins as f32)): Rectangle(12 * h / n_bins, 12) at (-7, 6, 5), turned by -PI / 2 (taken as the exact quarter
 *     turn) and mirrored, so bins run bottom to top and time leftwards, the newest row at the right edge, the zeroed row at the
 *     left.  u = (wy - cy) / ey + 0.5, v = 0.5 - (wx - cx) / ex; the pixel is covered when 0 <= u < 1 and 0 <= v < 1 (a NaN covers
 *     nothing).  t = v + (1 - scroll), v2 = t - floor(t) (the fragment's fract); texture row ty = min(floor(v2 * h), h - 1), column
 *     tx = min(floor(u * n_bins), n_bins - 1).  The texel's colour bytes decode through srgb_to_linear(byte / 255) (the curve of the
 *     scene section), its alpha is byte / 255; a texel with alpha byte 0 leaves the pixel as it is, any other is blended with the
 *     raster section's blend.
 *  9. the chroma boxes, with s = ui_scale and the pixel's centre at (i + 0.5, j + 0.5) measured from the top left: box pc of twelve
 *     spans x from (400 + 45 pc) s, 40 s wide, and y from height - 50 s to height - 10 s, each half-open; in the four 4 s corner
 *     squares the centre must lie within 4 s of the corner circle's centre (<=).  The boxes do not overlap.  Colour
 *     srgb_to_linear(colors[pc]), alpha the strength pvq_chroma_row gives; a strength that is not finite or is <= 0 draws nothing.
 *     No edge anti-aliasing.  (Bevy draws UI after tone mapping; here the boxes are blended in the same linear target.)
 * Left out of the 2-D picture after this stage: what the backdrop section lists. */
/* the reference's quad for n_bins (3 .. 1024) and history_rows (0: 200, or 2 .. 4096): out4 = (cx, cy, ex, ey) */
pvq_status pvq_overlay_quad(uint32_t n_bins, uint32_t history_rows, float *out4);
/* One stream's texture on the host, kept literally as the reference keeps it.  n_bins 3 .. 1024; history_rows 0 (200) or 2 .. 4096. */
typedef struct pvq_overlay_state pvq_overlay_state;
pvq_status pvq_overlay_state_create(uint32_t n_bins, uint32_t history_rows, pvq_overlay_state **out);
void pvq_overlay_state_destroy(pvq_overlay_state *s);
/* one frame's row, row_rgba [n_bins][4], as update.rs:1066-1087 stores it */
pvq_status pvq_overlay_state_push(pvq_overlay_state *s, const uint8_t *row_rgba);
/* the texture as it stands, out [history_rows][n_bins][4], and the write index; either may be NULL */
pvq_status pvq_overlay_state_texture(const pvq_overlay_state *s, uint8_t *out, uint32_t *write_index);
/* Both layers over image_inout [height][width][4], in place: the frame whose row was pushed last is the one drawn (scroll =
 * write_index / h).  state NULL: no quad; quad NULL: the reference's for the state; chroma12 NULL: no boxes (both NULL:
 * PVQ_ERR_INVALID_ARG); colors 12 RGB triples in [0, 1], NULL: pitchvis_colors::COLORS.  width, height 1 .. 4096; viewport_height
 * 0: the viewer's; ui_scale 0: 1, else positive and finite; quad finite with positive extents. */
pvq_status pvq_overlay_frame(const pvq_overlay_state *state, uint32_t width, uint32_t height, float viewport_height, float ui_scale,
                             const float *quad, const float *chroma12, const float *colors, float *image_inout);

/* The same for MANY streams on the GPU, fed with what pvq_render_batch_rows_device leaves in device memory.  The handle keeps every
 * stream's last history_rows rows — n_streams * history_rows * n_bins * 4 bytes of device memory (201,600 bytes a stream at 252
 * bins and 200 rows) — and the number of frames seen. */
typedef struct pvq_overlay_batch pvq_overlay_batch;
/* The arguments are checked before any device is touched: bin counts 3 .. 1024 (PVQ_ERR_UNSUPPORTED beyond), the other ranges as
 * for pvq_overlay_frame.  device_id < 0: a host-only handle whose device calls return PVQ_ERR_NO_DEVICE after their argument checks. */
pvq_status pvq_overlay_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, uint32_t history_rows,
                                    float viewport_height, float ui_scale, const float *quad, const float *colors, uint32_t n_streams,
                                    uint32_t width, uint32_t height, pvq_overlay_batch **out);
void pvq_overlay_batch_destroy(pvq_overlay_batch *b);
/* n_frames frames of every stream, in order, each blended over its row of d_image_inout [n_streams][n_frames][height][width][4]
 * (16-byte aligned) in place: a pixel is read and written by the same lane, and a pixel neither layer draws on is not touched.
 * d_rows [n_streams][n_frames][n_bins][4] bytes, 4-byte aligned, as pvq_render_outputs.spectrogram_vqt or .spectrogram_peaks;
 * d_chroma [n_streams][n_frames][12].  d_rows NULL: no quad, and the rings do not advance; d_chroma NULL: no boxes; both NULL:
 * PVQ_ERR_INVALID_ARG.  Frame f of a call reads the rows of frames f - (h - 2) .. f: the call's own where they are in the call, the
 * handle's ring otherwise; after the draw the call's last min(n_frames, h) rows go to the ring.  Asynchronous on `stream`; one
 * handle's calls are stream-ordered. */
pvq_status pvq_overlay_batch_frames_device(pvq_overlay_batch *b, size_t n_frames, const uint8_t *d_rows, const float *d_chroma,
                                           float *d_image_inout, void *stream);
/* one stream's ring as the reference's texture would stand after the frames seen (synchronises): out [history_rows][n_bins][4],
 * write_index may be NULL */
pvq_status pvq_overlay_batch_get_texture(pvq_overlay_batch *b, uint32_t stream_index, uint8_t *out, uint32_t *write_index);

/* ---- the text: pitch-name labels from font outlines, over the balls and under the overlay ----------------------------
 * The twelve Text2d labels of the viewer (pitchvis_viewer/src/display_system/setup.rs:386-416; names pitchvis_colors/src/lib.rs:36-38)
 * sit at z = -0.02: above every ball (z <= -0.125) and below the spectrogram quad (z = 5) and the UI.  So the stage is an in-place
 * blend over a finished image of the raster section's camera, run after pvq_backdrop_balls_over_device and before
 * pvq_overlay_batch_frames_device, and only in the Full and Performance visuals modes (update.rs:871-885 hides the labels in the
 * others: there the caller does not call it).  Bevy's text pipeline (shaping, rasteriser, glyph atlas, sampling of the scaled
 * quad) is not in the reference tree; the rule below is this library's own, and DESIGN.md 6i lists what it assumes.  The library
 * embeds no font: the caller brings one (the viewer's is DejaVuSans).
 *
 * Font.  Per codepoint a TrueType outline — contours of on- and off-curve points in font units, y upwards, an implied on-curve
 * point between two consecutive off-curve points — and an advance; units per em, hhea ascent and hhea descent (negative below the
 * baseline).  From TrueType bytes the reader takes head, maxp, hhea, hmtx, cmap (a Unicode subtable of format 12, else 4), loca
 * (both formats) and glyf, simple glyphs only: a composite glyph, or a font without glyf (CFF), is PVQ_ERR_UNSUPPORTED when a label
 * asks for it.  Hinting instructions are skipped, never interpreted; kern and GPOS are ignored; there is no shaping (one glyph per
 * codepoint, left to right).  Every offset and count is checked against the bytes before use: bad bytes are PVQ_ERR_INVALID_ARG
 * with a text that names the table.
 *
 * Layout of a label, in font pixels with y downwards about the label's position: k = font_px / units_per_em; the pen advances by
 * advance * k; the block's width is the sum of the advances, its height the line height 1.2 font_px; the block is centred on
 * (x, y), so left = -width / 2 and top = -0.6 font_px; baseline = top + (line height - (ascent - descent) k) / 2 + ascent k.  A
 * point (gx, gy) of the glyph at pen p lies at (left + p + gx k, baseline - gy k); times scale (world units per font pixel) about
 * (x, y) it is a world position, which the raster section's camera maps to output pixel coordinates (pixel (i, j) is the square
 * [i, i + 1] x [j, j + 1]): px = wx / s + width / 2, py = height / 2 - wy / s, s = viewport_height / height in f32.  All of this in
 * double, rounded once to f32.  A codepoint the font lacks is PVQ_ERR_INVALID_ARG naming it (Bevy would draw a replacement box).
 *
 * Outline to segments.  A quadratic p0 p1 p2 (output pixels, double) is cut into n = max(1, ceil(sqrt(|p0 - 2 p1 + p2| / (4 tol))))
 * chords of equal parameter, tol = 1 / 64 pixel; the chord ends are rounded once to f32.  A label's outline is one list of
 * directed segments, glyph by glyph, contour by contour; horizontal segments, segments that meet no pixel row of the image and
 * segments left of the image are dropped (they add nothing).
 *
 * Coverage of pixel (X, Y) by a label: for each segment in list order, clip it to the pixel's rows Y .. Y + 1 and integrate
 * clamp(x(y) - X, 0, 1) over y — piecewise linear after the cuts at x = X and x = X + 1 —, positive where the segment runs to
 * larger y; the coverage is min(|sum|, 1): the exact area of the outline inside the pixel square for a winding number of 0 or +-1
 * (overlapping contours of one sense count once where they fill the pixel).  f32 without FMA contraction, so the host face and the
 * device carry the same bits.  A label's pixel box is the pixel squares its outline's bounding box meets; outside it the coverage
 * is 0.  No hinting, no grid fitting, no MSAA on top.
 *
 * Blend.  Colour srgb_to_linear(rgb) (the curve of the scene section), alpha the coverage, the raster section's blend; a pixel
 * whose coverage is exactly 0 is not touched.  Labels blend in label order where they overlap.
 *
 * Limits: 1 .. 64 labels of 1 .. 8 codepoints; width, height 1 .. 4096; an em (font_px * scale / s) of at most 1024 output
 * pixels; at most 65536 segments a label; units per em 16 .. 16384; coordinates within +-65536 font units; a batch handle's
 * coverage layer (1 KB per tile a label's box meets) at most 256 MiB, PVQ_ERR_UNSUPPORTED beyond.  A font handle caches the glyphs
 * it has read and is not to be used from two threads at once. */
typedef struct pvq_text_font pvq_text_font;
pvq_status pvq_text_font_from_ttf(const uint8_t *bytes, size_t n_bytes, pvq_text_font **out);
/* The same data given directly: codepoints, advances, n_contours and n_points are [n_glyphs]; contour_ends holds, glyph after
 * glyph, the index of each contour's last point among the glyph's own points (ascending, the last one n_points - 1); points
 * [total][2] and on_curve [total] hold the glyphs' points one after the other. */
pvq_status pvq_text_font_from_outlines(uint32_t n_glyphs, const uint32_t *codepoints, const float *advances, const uint32_t *n_contours,
                                       const uint32_t *contour_ends, const uint32_t *n_points, const float *points, const uint8_t *on_curve,
                                       uint32_t units_per_em, float ascent, float descent, pvq_text_font **out);
void pvq_text_font_destroy(pvq_text_font *f);
/* any of the three may be NULL */
pvq_status pvq_text_font_metrics(const pvq_text_font *f, uint32_t *units_per_em, float *ascent, float *descent);
/* A glyph as the font holds it.  advance, n_contours, n_points may be NULL; contour_ends [cap_contours], points [cap_points][2] and
 * on_curve [cap_points] are filled where given and large enough (PVQ_ERR_INVALID_ARG where given and too small): ask for the
 * counts first. */
pvq_status pvq_text_font_glyph(pvq_text_font *f, uint32_t codepoint, float *advance, uint32_t *n_contours, uint32_t *n_points,
                               uint32_t cap_contours, uint32_t cap_points, uint32_t *contour_ends, float *points, uint8_t *on_curve);
typedef struct pvq_text_label {
    char text[36];          /* NUL-terminated UTF-8, 1 .. 8 codepoints */
    float x, y;             /* the block's centre, world units */
    float font_px, scale;   /* the viewer's 40 and 0.02: an em of 0.8 world units */
    float rgb[3];           /* sRGB, 0 .. 1 */
} pvq_text_label;
/* The reference's twelve: the last twelve of calculate_spiral_points(octaves, 12), each times 0.85 + 0.025 |x|, named
 * PITCH_NAMES[(idx + 12 - 3) % 12] and coloured colors[that] (12 RGB triples, NULL: pitchvis_colors::COLORS), font_px 40, scale
 * 0.02.  octaves 1 .. 255. */
pvq_status pvq_text_pitch_labels(uint32_t octaves, const float *colors, pvq_text_label *out12);
/* what the layout makes of a label on a width x height image */
typedef struct pvq_text_layout {
    uint32_t on_image;          /* 0: nothing of the label lies on the image; the box and n_tiles are 0 */
    uint32_t x0, y0, x1, y1;    /* its pixel box: first and last column and row */
    uint32_t n_segments;        /* of its list, after the drops */
    uint32_t n_tiles;           /* the 16 x 16 tiles the box meets: columns x0 / 16 .. x1 / 16, rows y0 / 16 .. y1 / 16 */
    float origin_x, baseline_y; /* the first glyph's origin, output pixel coordinates */
} pvq_text_layout;
pvq_status pvq_text_layout_query(pvq_text_font *font, const pvq_text_label *labels, uint32_t n, uint32_t width, uint32_t height,
                                 float viewport_height, pvq_text_layout *out_n);
/* One picture on the host: the labels over image_inout [height][width][4] in place, and / or every label's coverage to
 * coverage_out [n][height][width]; either may be NULL, both NULL is PVQ_ERR_INVALID_ARG.  viewport_height 0: the viewer's. */
pvq_status pvq_text_frame(pvq_text_font *font, const pvq_text_label *labels, uint32_t n, uint32_t width, uint32_t height,
                          float viewport_height, float *image_inout, float *coverage_out);

/* The same for MANY rows on the GPU.  The text is the same for every row, so the handle owns a compact coverage layer, computed on
 * the device once at create: one f32 per pixel of each (tile, label) pair, over the 16 x 16 tiles the labels' boxes meet only. */
typedef struct pvq_text_batch pvq_text_batch;
/* The arguments are checked, and the labels laid out, before any device is touched; the font is not needed after the call.
 * device_id < 0: a host-only handle whose device calls return PVQ_ERR_NO_DEVICE after their argument checks. */
pvq_status pvq_text_batch_create(int device_id, pvq_text_font *font, const pvq_text_label *labels, uint32_t n, float viewport_height,
                                 uint32_t width, uint32_t height, pvq_text_batch **out);
void pvq_text_batch_destroy(pvq_text_batch *b);
/* The labels over each of n_rows pictures d_image_inout [n_rows][height][width][4] (16-byte aligned), in place: a pixel is read and
 * written by the same lane, and a pixel no label covers is not touched.  A handle whose labels all lie off the image launches
 * nothing.  n_rows at most 2^31 - 1.  Asynchronous on `stream`; one handle's calls are stream-ordered. */
pvq_status pvq_text_batch_rows_device(pvq_text_batch *b, size_t n_rows, float *d_image_inout, void *stream);
/* the layer copied back as a full image out [height][width] (synchronises): label 0 .. n - 1, or -1: the largest over the labels */
pvq_status pvq_text_batch_get_coverage(pvq_text_batch *b, int label, float *out);

/* ---- the readout: the tuning-drift text, formatted and drawn row by row ----------------------------------------------
 * The bottom-right readout "Tuning drift: NNN" of the viewer's Debugging display mode (pitchvis_viewer/src/app/common.rs:348-432:
 * setup_analysis_text, update_analysis_text_system, analysis_text_showhide): a half-transparent black box, a white prefix, and the
 * rounded smoothed tuning-grid inaccuracy coloured green -> yellow -> red.  The stage is an in-place blend over a finished linear
 * image, run after pvq_overlay_batch_frames_device and before the present stage, in the Debugging display mode only (in the others
 * the caller does not call it).  Like the chroma boxes it is UI and stays in the linear target.  The value is one f32 a row,
 * laid out as pvq_analysis_batch_* writes tuning_grid_inaccuracy.  Bevy's UI text pipeline is not in the reference tree; the rule
 * below is this library's own, and DESIGN.md 6k lists what it assumes.  The font is the caller's (a pvq_text_font).  The FPS
 * counter (wall clock) and the bottom-left dump of settings are not drawn.
 *
 * Text.  r = roundf(v) (half away from zero, f32::round); the value text is Rust's format!("{r:>3.0}"): the integer's decimal
 * digits, '-' for a negative r, spaces on the left up to three characters.  Negative zero counts as negative (-0.4 gives " -0");
 * NaN gives "NaN", +inf "inf", -inf "-inf".  A finite |r| above 2 147 483 520 (the largest f32 below 2^31) is formatted as that
 * bound, so the value text has at most 11 characters: a deviation from the reference, which would print up to 39 digits; the
 * analysis cannot produce such a value.  The string is "Tuning drift: " and the value text: at most 25 glyph slots.
 *
 * Colour of the value text (common.rs:404-413), a = |r|, in f32 in the reference's order: a <= 10: (0, 1, 0); a <= 20:
 * ((a - 10) / 10, 1, 0); a <= 30: (1, 1 - (a - 20) / 10, 0); otherwise, NaN included, (1, 0, 0).  sRGB; each channel goes through
 * the scene section's srgb_to_linear.  The prefix is white.
 *
 * Atlas.  s = ui_scale (0: 1), the font size is F = 16 s output pixels (f32), k = F / units_per_em (double).  Each codepoint the
 * stage can emit — T u n i g d r f t, the space, ':', 0-9, '-', N, a — is rasterised once: its origin at pixel column 0, its
 * baseline on pixel row 0, a point (gx, gy) at (gx k, -gy k) in double; flattened as the text section's (tolerance 1 / 64 pixel,
 * chord ends rounded once to f32, horizontal chords dropped); coverage of a pixel by the text section's rule, unchanged.  A glyph's
 * cell is the pixel box its outline's bounding box meets, relative to (origin column, baseline row): a left bearing makes it
 * start at a negative column.  A codepoint the font lacks is PVQ_ERR_INVALID_ARG naming it, at create.
 *
 * Layout, f32 in this order, pixel coordinates from the top left: adv[c] = (float)(advance_c k), rounded once; the pen is the
 * sequential left fold p_0 = 0, p_(i+1) = p_i + adv[c_i], the text's width Wt = p_n; the node's box xr = W - 0.01f W,
 * yb = H - 0.01f H, xl = xr - Wt, yt = yb - 1.2f F; glyph i's origin column is floorf(xl + p_i + 0.5f), the baseline row
 * floorf(yt + b + 0.5f), b = (float)((1.2f F - (ascent - descent) k) / 2 + ascent k) in double: the text section's baseline inside
 * a line.  There is no sub-pixel glyph positioning: that is what makes an atlas valid.
 *
 * Blend.  First the box: the pixels whose centre (i + 0.5, j + 0.5) lies in [xl, xr) x [yt, yb), black at alpha 0.5, the raster
 * section's blend.  Then the glyphs in string order, each its span's colour at alpha = the atlas coverage; a coverage of exactly
 * 0 is not blended.  A pixel that neither the box nor a glyph covers is neither read nor written; glyph cells may reach outside
 * the box and are drawn there.  Everything is clipped to the image.  f32 without FMA contraction: the host face and the device
 * carry the same bits.
 *
 * Limits: width, height 1 .. 4096; ui_scale 0 or positive and finite with F at most 1024; at most 65536 chords a glyph; an atlas of
 * at most 256 MiB, PVQ_ERR_UNSUPPORTED beyond; n_rows at most 2^31 - 1; the image 16-byte aligned. */
#define PVQ_READOUT_MAX_SLOTS 25
/* The value text of `value` (NUL-terminated, at most 11 characters) and its sRGB colour; either may be NULL. */
pvq_status pvq_readout_text(float value, char text_out[12], float srgb_out[3]);
/* what the layout makes of a value on a width x height image */
typedef struct pvq_readout_layout {
    float xl, xr, yt, yb;                        /* the node's box */
    float text_width, font_px, baseline;         /* Wt, F, b */
    int32_t baseline_row;
    uint32_t n_slots;                            /* glyph slots of the string, 17 .. 25 */
    char text[PVQ_READOUT_MAX_SLOTS + 3];        /* the whole string, NUL-terminated */
    int32_t origin_x[PVQ_READOUT_MAX_SLOTS];     /* each slot's origin column */
    int32_t cell_x0[PVQ_READOUT_MAX_SLOTS];      /* each slot's placed cell on the image (not clipped): first column and row, */
    int32_t cell_y0[PVQ_READOUT_MAX_SLOTS];
    uint32_t cell_w[PVQ_READOUT_MAX_SLOTS];      /* width and height; 0 x 0: no outline (the space) */
    uint32_t cell_h[PVQ_READOUT_MAX_SLOTS];
    float value_srgb[3], value_linear[3];        /* the value text's colour */
} pvq_readout_layout;
pvq_status pvq_readout_layout_query(pvq_text_font *font, float value, uint32_t width, uint32_t height, float ui_scale,
                                    pvq_readout_layout *out);
/* One picture on the host: the readout of `value` over image_inout [height][width][4], in place. */
pvq_status pvq_readout_frame(pvq_text_font *font, float value, uint32_t width, uint32_t height, float ui_scale, float *image_inout);

/* The same for MANY rows on the GPU, each row its own value: the device formats the value, lays the string out and draws it.  The
 * handle owns the glyph atlas, computed on the device once at create. */
typedef struct pvq_readout_batch_s pvq_readout_batch;
/* The arguments are checked, and the atlas laid out, before any device is touched; the font is not needed after the call.
 * device_id < 0: a host-only handle whose rows_device returns PVQ_ERR_NO_DEVICE after its argument checks, and whose atlas is the
 * host face's. */
pvq_status pvq_readout_batch_create(int device_id, pvq_text_font *font, uint32_t width, uint32_t height, float ui_scale,
                                    pvq_readout_batch **out);
void pvq_readout_batch_destroy(pvq_readout_batch *b);
/* The readout of d_values[row] over each of n_rows pictures d_image_inout [n_rows][height][width][4] (16-byte aligned), in place:
 * a pixel is read and written by the same lane.  d_values [n_rows] f32 in device memory, as pvq_analysis_batch_* leaves
 * tuning_grid_inaccuracy [stream][frame].  Asynchronous on `stream`; one handle's calls are stream-ordered. */
pvq_status pvq_readout_batch_rows_device(pvq_readout_batch *b, size_t n_rows, const float *d_values, float *d_image_inout, void *stream);
/* A codepoint's atlas cell: its box relative to (origin column, baseline row), its advance in pixels, and its coverages to
 * out [h][w] where out is given (cap_floats at least w h; ask for the size first).  Any pointer may be NULL.  Synchronises.  A
 * codepoint the readout never emits is PVQ_ERR_INVALID_ARG. */
pvq_status pvq_readout_batch_get_atlas(pvq_readout_batch *b, uint32_t codepoint, int32_t *x0, int32_t *y0, uint32_t *w, uint32_t *h,
                                       float *advance, size_t cap_floats, float *out);

/* ---- the present stage: bloom, display transform and sRGB bytes ----------------------------------------------------
 * What turns the linear HDR target [H][W][4] of the sections above into something a screen, a PNG or a video encoder takes: the
 * camera's Bloom, its Tonemapping::SomewhatBoringDisplayTransform and the surface's sRGB encode.  The reference fixes the settings
 * (pitchvis_viewer/src/display_system/setup.rs:347-383: Hdr, low_frequency_boost 1.0, low_frequency_boost_curvature 1.0,
 * high_pass_frequency 0.52, prefilter threshold 0.17 and softness 0.82, Additive) and the intensity (update.rs:346-347, the scene
 * section's `bloom`); the passes themselves are Bevy's and not in the reference tree, so the rule below is restated from Bevy's
 * published behaviour (DESIGN.md 6h has the table of assumed semantics).  All arithmetic is f32 without FMA contraction, `/` IEEE,
 * every sum in the order written.  The first pass's pow is taken in double arithmetic without libm and rounded once to f32 on host and device,
 * so both carry the same bits in the bloomed linear picture; the bytes go through each side's own expf and powf and agree within a level.
 *
 * Mips.  d = max_mip_dimension, n_mips = max(floor(log2 d), 2) - 1; mip 0 is max(1, round(W r)) x max(1, round(H r)) with r = d as
 * f32 / H as f32, mip k is max(1, w0 >> k) x max(1, h0 >> k).  A mip holds RGB in f32 (Bevy: Rg11b10Ufloat).
 * Sampling.  A texture (w, h) at uv, bilinear with clamp-to-edge: p = uv * (w, h) - 0.5, i0 = floor(p), f = p - i0, indices clamped
 * to 0 .. size - 1, x interpolated before y, lerp(a, b, t) = a + (b - a) * t.  Target texel (i, j) of (wt, ht) has uv = ((i + 0.5) /
 * wt, (j + 0.5) / ht).
 * Downsample.  13 taps at uv + (ox / ws, oy / hs): a (-2, 2) b (0, 2) c (2, 2) d (-2, 0) e (0, 0) f (2, 0) g (-2, -2) h (0, -2) i (2,
 * -2) j (-1, 1) k (1, 1) l (-1, -1) m (1, -1).  Mip k -> k + 1: (a + c + g + i) * 0.03125 + (b + d + f + h) * 0.0625 + (e + j + k +
 * l + m) * 0.125.  The picture -> mip 0 (its RGB; alpha ignored): g0 = (a + b + d + e) * 0.03125, g1 = (b + c + e + f) * 0.03125, g2 =
 * (d + e + g + h) * 0.03125, g3 = (e + f + h + i) * 0.03125, g4 = (j + k + l + m) * 0.125, each times 1 / (1 + luma(pow(max(g, 0),
 * 1 / 2.2)) / 4) with luma(v) = 0.2126 r + 0.7152 g + 0.0722 b, summed in order; then per channel fmin(fmax(x, 1e-4), 3.40282347e37)
 * (a NaN becomes 1e-4); then, unless threshold == 0, with knee = threshold * softness and br = max(r, g, b): s = clamp(br -
 * (threshold - knee), 0, 2 knee), s = s * s * (0.25 / (knee + 1e-5)), colour *= max(br - threshold, s) / max(br, 1e-5).
 * Upsample.  k = n_mips - 1 .. 1 into mip k - 1, in place: tent = e * 0.25 + (b + d + f + h) * 0.125 + (a + c + g + i) * 0.0625 of
 * mip k at uv offsets (+-x, +-y), x = 0.004 / (W / H), y = 0.004 (a .. i placed as above); additive dst += B_k * tent, energy-conserving
 * dst = dst * (1 - B_k) + B_k * tent.  The last step takes the tent of mip 0 at the picture's pixel with B_0 into the picture's RGB;
 * alpha passes through.
 * Blend factor.  r = k / (n_mips - 1) (0 when n_mips is 1); lf = (1 - powf(1 - r, 1 / (1 - curvature))) * low_frequency_boost (at
 * curvature 1 the exponent is +inf: powf(1, inf) = 1, powf(x < 1, inf) = 0); hp = 1 - clamp((r - high_pass_frequency) /
 * high_pass_frequency, 0, 1); energy-conserving: lf *= 1 - intensity; B_k = (intensity + lf) * hp.
 * A picture whose intensity is not finite or is <= 0 skips bloom (as Bevy's node does at 0) and still gets the rest.
 * Display transform (SOMEWHAT_BORING).  c = max(c, 0); y = luma(c); cb = dot(c, (-0.1146, -0.3854, 0.5)), cr = dot(c, (0.5, -0.4542,
 * -0.0458)); curve(v) = 1 - expf(-v); bt = curve(sqrtf(cb cb + cr cr) * 2.4); desat = max((bt - 0.7) * 0.8, 0) squared; desat_col =
 * lerp(c, (y, y, y), desat); tm0 = c * max(0, curve(y) / max(1e-5, y)); tm1 = curve(desat_col); out = lerp(tm0, tm1, bt * bt) * 0.97.
 * NONE passes max(c, 0) through.
 * Encode.  v = clamp(out, 0, 1), v <= 0.0031308 ? 12.92 v : 1.055 powf(v, 1 / 2.4) - 0.055, byte = floor(v * 255 + 0.5); alpha:
 * floor(clamp(a, 0, 1) * 255 + 0.5); a NaN encodes as 0.
 * Left out of the displayed picture, here and in every section above: MSAA beyond the backdrop's (which the pvq_msaa_ entries
 * draw with samples = 4; the overlay quad's border pixels are left out), the deband dither, colour grading
 * (the reference leaves it at identity) and a draw of the chroma boxes in display space — they stay where the overlay stage blends
 * them, in the linear target, and so pass through the transform.  The Debugging mode's tuning-drift text is drawn: the readout
 * section above, also in the linear target; the FPS counter and the dump of settings are not. */
enum { PVQ_PRESENT_ENERGY_CONSERVING = 0, PVQ_PRESENT_ADDITIVE = 1 };          /* composite_mode */
enum { PVQ_PRESENT_TONEMAP_NONE = 0, PVQ_PRESENT_TONEMAP_SOMEWHAT_BORING = 1 }; /* tonemapping */
typedef struct pvq_present_settings {
    float low_frequency_boost, low_frequency_boost_curvature, high_pass_frequency, threshold, threshold_softness;
    int composite_mode;
    uint32_t max_mip_dimension;   /* 0: 512, else 4 .. 4096 */
    int tonemapping;
} pvq_present_settings;
void pvq_present_default_settings(pvq_present_settings *s);   /* 1.0, 1.0, 0.52, 0.17, 0.82, ADDITIVE, 512, SOMEWHAT_BORING */
/* the mip sizes of a width x height picture (1 .. 4096 each): *out_count = n_mips (at most 11), out_sizes [n_mips][2] as (w, h);
 * either may be NULL.  PVQ_ERR_UNSUPPORTED where mip 0 would be wider than 16384 texels (a picture far wider than high). */
pvq_status pvq_present_mips(uint32_t width, uint32_t height, uint32_t max_mip_dimension, uint32_t *out_count, uint32_t *out_sizes);
/* B_0 .. B_{n_mips - 1} (n_mips 1 .. 11) at an intensity; settings NULL: the defaults.  The settings are checked wherever they are
 * given: every float finite, high_pass_frequency > 0, the enums and max_mip_dimension in range. */
pvq_status pvq_present_blend_factors(const pvq_present_settings *settings, float intensity, uint32_t n_mips, float *out);
/* one picture on the host: image [height][width][4] -> out_rgba8 [height][width][4] bytes and, unless NULL, out_hdr
 * [height][width][4], the bloomed linear picture before the display transform (it may be `image`) */
pvq_status pvq_present_frame(const pvq_present_settings *settings, uint32_t width, uint32_t height, const float *image, float intensity,
                             uint8_t *out_rgba8, float *out_hdr);

/* The same for MANY pictures on the GPU.  Stateless; the handle owns one grow-only workspace for the mip chains of a piece of a
 * call's rows (the sum of w_k h_k * 16 bytes a row: 9.9 MB at 1280 x 720 and 512). */
typedef struct pvq_present_batch pvq_present_batch;
/* The arguments are checked before any device is touched.  device_id < 0: a host-only handle whose device call returns
 * PVQ_ERR_NO_DEVICE after its argument checks. */
pvq_status pvq_present_batch_create(int device_id, const pvq_present_settings *settings, uint32_t width, uint32_t height,
                                    pvq_present_batch **out);
void pvq_present_batch_destroy(pvq_present_batch *b);
/* upper bound of the workspace in bytes (default 1 GiB): a call whose rows need more runs in pieces of rows, with the same bits;
 * one row's chains are always allocated */
pvq_status pvq_present_batch_set_workspace_limit(pvq_present_batch *b, uint64_t bytes);
/* d_image [n_rows][height][width][4] f32, 16-byte aligned, never written; d_intensity [n_rows] f32 — pvq_scene_outputs.bloom as it
 * lies —, NULL: no bloom in any row; d_rgba8 [n_rows][height][width][4] bytes, 4-byte aligned; d_hdr NULL or
 * [n_rows][height][width][4] f32, 16-byte aligned, which may be d_image (a picture pixel is read only by the lane that writes it).
 * A row's result depends neither on its place in the call nor on the cut into pieces.  n_rows at most 2^31 - 1.  Asynchronous on
 * `stream`; one handle's calls are stream-ordered. */
pvq_status pvq_present_batch_rows_device(pvq_present_batch *b, size_t n_rows, const float *d_image, const float *d_intensity,
                                         uint8_t *d_rgba8, float *d_hdr, void *stream);

/* The note model the dataset of pitchvis_train exists for (pitchvis_train/train.py:67-99), which the viewer runs per rendered frame
 * through TorchScript on a CUDA device (pitchvis_viewer/src/ml_system.rs:24-69): a window of t_frames consecutive dB frames,
 * flattened to L = t_frames * n_bins values -> Conv1d(1, 16, kernel 5, stride 2, no padding) -> ReLU -> max_pool1d(2) -> flatten
 * (channel-major: feature c * O_pool + p) -> Linear(n_features, mlp_size) -> ReLU -> mlp_layers x (Linear(mlp_size, mlp_size) ->
 * ReLU) -> Linear(mlp_size, 128) -> sigmoid.  O_conv = (L - 5) / 2 + 1, O_pool = O_conv / 2 (integer divisions: an odd O_conv
 * loses its last position, as max_pool1d does), n_features = 16 * O_pool.  A handle made by pvq_note_model_create computes all of
 * it in f32.  The reference's "TODO: Half" (ml_system.rs:26) is an option of the handle, pvq_note_model_create_precision, under
 * one rule for PVQ_NOTE_BF16 and PVQ_NOTE_F16:
 *   - the conv, its ReLU and the pool are f32, the fmaf chain of the f32 path, so the pooled features are the same f32 values;
 *   - each pooled feature is rounded to the type once;
 *   - every dense weight (fc1, layers, output) is rounded to the type once, at create;
 *   - every product accumulates in f32; bias and ReLU are f32;
 *   - a hidden activation is rounded to the type when it is stored;
 *   - logits, the sigmoid and the mask are f32, as on an f32 handle.
 * Every rounding is to nearest, ties to even (pvq_note_round).  Subnormals: the 16-bit matrix instructions take their A and B
 * operands as they are, f16 subnormals included (only f32 / f64 matrix operands follow the wave's denormal mode, and the kernels
 * are built with the mode that keeps them in any case), so a value below 2^-14 in magnitude rounds to a multiple of 2^-24 and is
 * not flushed; pvq_note_round and pvq_note_model_infer do the same.  bf16 has f32's exponent range: an f32 subnormal rounds to a
 * bf16 subnormal.
 * f16 range: a dense weight beyond +-65504 is refused at create (PVQ_ERR_INVALID_ARG, the layer named).  A row in which a pooled
 * feature or a hidden activation leaves the f16 range (rounds to infinity) has unspecified values in that row only, as a row with
 * a non-finite dB value has.  bf16 has no such case. */
typedef struct pvq_note_model pvq_note_model;
typedef enum { PVQ_NOTE_F32 = 0, PVQ_NOTE_BF16 = 1, PVQ_NOTE_F16 = 2 } pvq_note_precision;
/* replaces the constructor arguments of train.py:67-75 (kernel_size 5, stride 2, 16 channels, pool 2 and 128 outputs are fixed, as
 * in train.py:75,90 and ml_system.rs:7).  n_bins 3 .. 1024; t_frames 1 .. 8 with t_frames * n_bins >= 8; mlp_size a multiple of 16
 * in 16 .. 4096; mlp_layers 0 .. 8 */
typedef struct pvq_note_model_params {
    uint32_t n_bins;     /* train.py:14 n_bins / ml_system.rs: the VqtRange's bucket count */
    uint32_t t_frames;   /* train.py:15 T (5); 3 in the viewer */
    uint32_t mlp_size;   /* train.py:69 mlp_size (1024) */
    uint32_t mlp_layers; /* train.py:69 mlp_layers (2) */
} pvq_note_model_params;
/* replaces the module's state_dict (train.py:205-208 saves it inside a TorchScript file): HOST pointers to f32 arrays in PyTorch's
 * layout.  layer_weight / layer_bias are arrays of mlp_layers pointers (may be NULL when mlp_layers == 0) */
typedef struct pvq_note_model_weights {
    const float *conv_weight;          /* conv1.weight [16][1][5] */
    const float *conv_bias;            /* conv1.bias [16] */
    const float *fc1_weight;           /* fc1.weight [mlp_size][n_features] */
    const float *fc1_bias;             /* fc1.bias [mlp_size] */
    const float *const *layer_weight;  /* layers.i.weight [mlp_size][mlp_size] */
    const float *const *layer_bias;    /* layers.i.bias [mlp_size] */
    const float *output_weight;        /* output.weight [128][mlp_size] */
    const float *output_bias;          /* output.bias [128] */
} pvq_note_model_weights;
/* per-row results of pvq_note_model_rows_device, DEVICE pointers, any may be NULL */
typedef struct pvq_note_model_outputs {
    float *d_prob;     /* [n_streams][stride_frames][128]: AnalysisState::ml_midi_base_pitches (ml_system.rs:56-59) */
    float *d_logits;   /* [n_streams][stride_frames][128]: the same before the sigmoid */
    uint32_t *d_mask;  /* [n_streams][stride_frames][4]: bit k (word k / 32, bit k % 32) set when logit_k > 0, the pitches
                          ml_system.rs:61-65 reports (p > 0.5); 4-byte aligned */
} pvq_note_model_outputs;
/* replaces NoteModel.__init__ + load_state_dict (train.py:67-87) / tch::CModule::load_on_device (ml_system.rs:13-20).  The sizes
 * are checked before any device is touched (PVQ_ERR_INVALID_ARG for a null pointer, a zero field or an mlp_size that is no
 * multiple of 16, PVQ_ERR_UNSUPPORTED for a value beyond the ranges above).  The weights are copied; every dense matrix is
 * repacked once on the host into the order the kernels' matrix instructions read.  device_id < 0: a host-only handle
 * (pvq_note_model_infer works, pvq_note_model_rows_device returns PVQ_ERR_NO_DEVICE after its argument checks). */
pvq_status pvq_note_model_create(int device_id, const pvq_note_model_params *params, const pvq_note_model_weights *weights,
                                 pvq_note_model **out);
/* The same with the precision of the dense layers chosen (the rule above); pvq_note_model_create is this with PVQ_NOTE_F32, and a
 * PVQ_NOTE_F32 handle made here gives that one's bits.  A value that is none of the enum's is PVQ_ERR_INVALID_ARG.  Every other
 * entry point takes a handle of any precision; the outputs stay f32. */
pvq_status pvq_note_model_create_precision(int device_id, const pvq_note_model_params *params, const pvq_note_model_weights *weights,
                                           pvq_note_precision precision, pvq_note_model **out);
/* the precision a handle was made with */
pvq_status pvq_note_model_precision(const pvq_note_model *m, pvq_note_precision *out);
/* The rounding of that rule as a pure host function: out[i] = in[i] rounded to nearest even to the type, returned as f32
 * (PVQ_NOTE_F32: the identity).  bf16: beyond the largest finite value to infinity.  f16: magnitudes of 65520 and above to
 * infinity, below 2^-14 to multiples of 2^-24 (subnormals are kept), below or at 2^-25 to a signed zero.  NaN stays NaN.  in may
 * be out. */
pvq_status pvq_note_round(pvq_note_precision precision, const float *in, size_t n, float *out);
void pvq_note_model_destroy(pvq_note_model *m);
/* the derived sizes: out4 = { L, O_conv, O_pool, n_features } */
pvq_status pvq_note_model_sizes(const pvq_note_model *m, uint32_t out4[4]);
/* replaces ml_system.rs::infer (ml_system.rs:24-69) for one row, on the host in plain f32: window_host [L] (t_frames frames, oldest
 * first) -> out_prob [128].  Works on a host-only handle.  The one-row face beside pvq_note_model_rows_device, as
 * pvq_spectrogram_row is beside pvq_render_batch_rows_device.  On a PVQ_NOTE_BF16 / PVQ_NOTE_F16 handle it rounds where the rule
 * above says (pvq_note_round) and sums in f32 in ascending index order, so a host-only handle predicts the device to within
 * what the type itself costs. */
pvq_status pvq_note_model_infer(const pvq_note_model *m, const float *window_host, float out_prob[128]);
/* The same for MANY rows on the GPU.  d_db is [n_streams][stride_frames][n_bins] (DEVICE), exactly what
 * pvq_vqt_calculate_batch_db_streams writes; n_frames is a HOST array of n_streams frame counts (each <= stride_frames; NULL: every
 * stream has stride_frames).  Row (s, f) is the model on frames f - t_frames + 1 .. f of stream s, one contiguous run of L floats:
 * train.py:120-131's window_data with the label aligned to the last frame.  Rows with f < t_frames - 1 or f >= n_frames[s] are
 * written as zeros in every output.  A row whose window holds a non-finite dB value has unspecified values in that row only.
 * Asynchronous on `stream`; hidden activations live in a grow-only workspace of the handle (no allocation on the call path once
 * it has grown), so one handle serves one stream at a time.  A PVQ_NOTE_BF16 / PVQ_NOTE_F16 handle stores four values at a time:
 * its d_prob and d_logits must be 16-byte aligned (PVQ_ERR_INVALID_ARG otherwise). */
pvq_status pvq_note_model_rows_device(pvq_note_model *m, const float *d_db, const size_t *n_frames, uint32_t n_streams,
                                      size_t stride_frames, const pvq_note_model_outputs *outs, void *stream);
/* Windows that continue from call to call: what a caller needs who feeds frames as they arrive (one frame per call is the
 * viewer's cadence, ml_system.rs:50-69), where pvq_note_model_rows_device starts afresh at every call and gives rows
 * f < t_frames - 1 as zeros.  A carry keeps, per stream, the last t_frames - 1 frames it was given (on the device) and
 * seen[s], the number of frames stream s has been given since create or reset — a HOST counter, as n_frames is a host array.
 * It belongs to the model's n_bins, t_frames and device, and to n_streams streams (n_streams 0: PVQ_ERR_INVALID_ARG); a
 * host-only model gives a host-only carry.
 *
 * pvq_note_model_rows_carry_device: d_db, n_frames, stride_frames and outs as for pvq_note_model_rows_device, but n_frames[s]
 * (NULL: stride_frames each) counts the NEW frames of stream s, which continue its sequence.  Row (s, f), f < n_frames[s], is the
 * model on the last t_frames frames of the stream's whole sequence ending at that frame, and is a model row exactly when
 * seen[s] + f >= t_frames - 1; every other row of every output is written as zeros.  Afterwards the carry holds the stream's last
 * min(t_frames - 1, seen + n) frames and seen += n: a call with n_frames[s] < t_frames - 1 merges old and new frames, one with
 * n_frames[s] == 0 leaves the stream alone.  d_db rows f >= n_frames[s] are never read.  t_frames == 1: nothing is carried, the
 * rows are still packed.
 * The model rows of ALL streams are packed into tiles of 128 (a tile is 128 consecutive rows of the call's row list, whatever
 * streams they come from): a call of R model rows launches ceil(R / 128) tiles' worth of workgroups per layer, where
 * pvq_note_model_rows_device spends a tile per stream.  A row's logits, probability and mask carry the bits
 * pvq_note_model_rows_device gives the same window, at every precision.
 * Asynchronous on `stream`, with no host synchronisation and no device-to-host copy (the per-stream descriptors of a call go out
 * from pinned host memory, one of 8 slots in turn: only a host that has queued 8 calls the device has not begun waits, for the
 * oldest one's descriptor copy); no allocation on the call path once the
 * carry's row table and the model's workspace have grown (the table is 16 bytes a model row and outside the workspace limit,
 * which cuts the call into chunks of whole tiles with the same bits).  Every frame the call or a later one needs is copied inside
 * the call, so d_db may be overwritten in stream order right after it.  One carry, like one model, serves one stream at a time.
 * All argument checks of pvq_note_model_rows_device apply, the 16-byte alignment of a 16-bit handle's outputs included; a carry
 * made for another n_streams, for a model of other n_bins or t_frames, or on another device is PVQ_ERR_INVALID_ARG; 2^31 model
 * rows or more in one call too.  On host-only handles the call returns PVQ_ERR_NO_DEVICE after these checks.
 * pvq_note_carry_reset: stream_index < 0: every stream; else that stream (>= n_streams: PVQ_ERR_INVALID_ARG).  seen returns to 0
 * at once, the kept frames are cleared in stream order. */
struct pvq_note_carry;   /* opaque; named by its tag: the set of handle typedefs of this header stays as it was */
pvq_status pvq_note_carry_create(const pvq_note_model *m, uint32_t n_streams, struct pvq_note_carry **out);
void pvq_note_carry_destroy(struct pvq_note_carry *c);
pvq_status pvq_note_carry_reset(struct pvq_note_carry *c, int64_t stream_index, void *stream);
pvq_status pvq_note_carry_frames_seen(const struct pvq_note_carry *c, uint32_t stream_index, uint64_t *out);
pvq_status pvq_note_model_rows_carry_device(pvq_note_model *m, struct pvq_note_carry *c, const float *d_db, const size_t *n_frames,
                                            uint32_t n_streams, size_t stride_frames, const pvq_note_model_outputs *outs,
                                            void *stream);
/* Upper bound in bytes for that workspace (default 256 MiB): a call processes its rows in chunks of whole 128-row tiles that fit;
 * results do not depend on the chunking.  One tile (1 KiB * mlp_size + its table entry) is the least a call works with.  A
 * PVQ_NOTE_BF16 / PVQ_NOTE_F16 handle keeps, per tile, the 128 rounded feature rows and two hidden rows each, every row padded
 * to whole chunks of 32 values: 256 * (pad32(n_features) + 2 * pad32(mlp_size)) bytes + its table entry. */
pvq_status pvq_note_model_set_workspace_limit(pvq_note_model *m, uint64_t bytes);

/* The trainer's optimisation step for that model (pitchvis_train/train.py:108-162): forward in training mode, BCELoss, backward,
 * optim.Adam with weight decay, on a batch of rows gathered by index from a dataset that already sits in device memory (what
 * train_dataset_streams leaves there).  The handle owns, on the device, the parameters in PyTorch layout, their gradients, Adam's two
 * moments and the step counter, plus a workspace sized once from max_batch: 4 x the parameter count in floats, and per row of
 * max_batch (2 n_features + (mlp_layers + 3) mlp_size + 355) floats, and 16 MiB of partial sums.  Nothing is allocated by a step.
 *
 * Dataset (train.py:17-21,34,46).  d_db is [n_rows][n_bins] f32, d_targets is [n_rows][128] f32, contiguous DEVICE buffers that are
 *   never written.  Sample i (t_frames - 1 <= i < n_rows) has as input the t_frames * n_bins contiguous values of rows
 *   i - t_frames + 1 .. i (window_data followed by the flat reshape) and as target row i of d_targets; a target is any value in [0, 1].
 * Batch.  idx is a HOST array of `batch` sample indices.  It is validated before anything is launched: an index outside
 *   [t_frames - 1, n_rows) or a batch outside 1 .. max_batch gives PVQ_ERR_INVALID_ARG.  It is copied to a pinned buffer of the
 *   handle before the call returns and goes to the device on `stream`.  Duplicates are legal; their contributions add.
 * Forward (train.py:87-99, training mode).  conv(1 -> 16, k 5, s 2) -> ReLU -> max_pool1d(2) -> flatten channel-major -> fc1 -> ReLU
 *   -> mlp_layers x (Linear -> ReLU -> dropout) -> output.  Dropout follows the hidden `layers` only, not fc1 (train.py:93-95); it is
 *   inverted dropout: a kept value is multiplied by 1 / (1 - p), rounded to f32.
 * Dropout mask.  No stateful generator: a counter-based hash of (seed, step counter, layer, row in the batch, column).  With 64-bit
 *   unsigned arithmetic modulo 2^64 and
 *       mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31   (splitmix64's finaliser)
 *       key   = mix(mix(seed + 0x9E3779B97F4A7C15 * (step + 1)) ^ layer)
 *       u     = mix(key ^ (row * 2^32 + col)) >> 40                                 (24 bits)
 *   element (row, col) of the output of hidden layer `layer` (0-based) is KEPT when u >= floor(dropout * 2^24), the product taken in
 *   double.  `step` is pvq_note_trainer_steps at the time of the call (the same for PVQ_TRAIN_GRAD and the PVQ_TRAIN_STEP that
 *   follows it), `row` the position in idx.  pvq_note_trainer_dropout_keep evaluates it on the host.
 * Loss (train.py:136,154).  The mean over batch * 128 of the binary cross-entropy, computed from the logits z in the stable form
 *   max(z, 0) - z y + log1p(exp(-|z|)), terms in f32, their sum in double.  One difference from nn.BCELoss on sigmoid(z) in f32:
 *   BCELoss clamps each logarithm at -100, so a saturated sigmoid (|z| beyond about 17 in f32, where 1 - sigmoid(z) rounds to 0)
 *   costs at most 100 there; this form keeps the exact value |z| and its gradient.
 * Backward (train.py:155).  dZ_out = (sigmoid(z) - y) / (batch * 128).  Per Linear layer dW = dZ^T H, db = sum over rows of dZ,
 *   dH = (dZ W) * mask * 1 / (1 - p) * [H > 0].  Through the pool to the larger of each pair, the first on a tie (max_pool1d);
 *   through the ReLU with gradient 0 at 0; to conv1.weight [16][5] and conv1.bias [16].
 * Adam (train.py:141-144: torch.optim.Adam, L2 weight decay added to the gradient, not AdamW).  With t = steps + 1, per element
 *   g += wd w;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  w -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 *   The element's arithmetic is carried out in double and each stored value (w, m, v) rounded once to f32; the stored gradient is
 *   left as the backward pass wrote it (without the decay term).
 * Determinism.  Equal weights, hyper-parameters, seed, counter, dataset and idx give equal bits in every gradient and every updated
 *   weight, run after run: no floating-point atomics, every reduction in an order fixed by the shapes. */
typedef struct pvq_note_trainer pvq_note_trainer;
/* replaces the optimiser's and the module's constructor arguments, train.py:111,131-144 */
typedef struct pvq_note_trainer_hyper {
    double lr;            /* train.py:111 (1e-5); > 0 */
    double beta1, beta2;  /* torch.optim.Adam's defaults 0.9 / 0.999; 0 <= beta < 1 */
    double eps;           /* train.py:143 torch.finfo(torch.float32).eps = 1.1920929e-7; > 0 */
    double weight_decay;  /* train.py:144 (5e-4); >= 0 */
    double dropout;       /* train.py:131-138 (0.1); 0 <= dropout < 1 */
    uint64_t seed;        /* of the dropout mask */
} pvq_note_trainer_hyper;
typedef enum pvq_train_mode {
    PVQ_TRAIN_STEP = 0, /* train.py:153-158: dropout on, backward, Adam, counter + 1 */
    PVQ_TRAIN_GRAD = 1, /* the same without Adam and without advancing the counter: the gradients stay readable */
    PVQ_TRAIN_EVAL = 2  /* train.py:164-176 model.eval(): dropout off, forward and loss only (the validation loss) */
} pvq_train_mode;
typedef enum pvq_train_array { PVQ_TRAIN_WEIGHTS = 0, PVQ_TRAIN_GRADS = 1, PVQ_TRAIN_ADAM_M = 2, PVQ_TRAIN_ADAM_V = 3 } pvq_train_array;
/* lr 1e-5, betas 0.9 / 0.999, eps 1.1920929e-7 (2^-23), weight decay 5e-4, dropout 0.1 (train.py:111,131-144), seed 0 */
void pvq_note_trainer_hyper_default(pvq_note_trainer_hyper *h);
/* replaces NoteModel(...) + optim.Adam(...) (train.py:131-144).  params and weights as for pvq_note_model_create, with its size
 * checks; then lr > 0, 0 <= beta < 1, eps > 0, weight_decay >= 0, 0 <= dropout < 1, 1 <= max_batch <= 4096 (PVQ_ERR_INVALID_ARG).
 * All checks run before any device is touched.  The weights are copied; gradients, moments and the counter start at zero.
 * device_id < 0: a host-only handle (argument checks work, pvq_note_trainer_step returns PVQ_ERR_NO_DEVICE after them; no CPU
 * fallback). */
pvq_status pvq_note_trainer_create(int device_id, const pvq_note_model_params *params, const pvq_note_model_weights *weights,
                                   const pvq_note_trainer_hyper *hyper, uint32_t max_batch, pvq_note_trainer **out);
/* The same with the precision of the dense products chosen.  PVQ_NOTE_F32 is exactly pvq_note_trainer_create (its bits).
 * PVQ_NOTE_F16 and any value that is none of the enum's are refused before a device is touched (PVQ_ERR_INVALID_ARG, the reason in
 * pvq_last_error): dZ = (sigmoid(z) - y) / (128 * batch) is about 1e-5 and underflows f16 without loss scaling, which is not offered.
 * PVQ_NOTE_BF16 is mixed-precision training: bf16 operands on the 16-bit matrix instructions, f32 accumulation, f32 master
 * weights, gradients and Adam moments, under this rule (every rounding is pvq_note_round's: nearest, ties to even, subnormals kept):
 *   Kept in f32.  The four arrays of pvq_note_trainer_read stay f32 in state_dict order and layout; pvq_note_trainer_read, the
 *     step's loss and logits, the test pass and Adam are those of an f32 handle.
 *   Forward.  Conv, ReLU and pool in f32 by the fmaf chain of the f32 path; each pooled feature rounded once (the point of the
 *     inference rule above).  Each dense weight is rounded once per step from its f32 master value: the handle keeps a 16-bit
 *     shadow of the dense weights, written at create and refreshed after every Adam update.  A hidden activation is bias + ReLU +
 *     (dropout keep * 1 / (1 - p)) in f32 on the f32 accumulator, then rounded once and stored in 16 bits; the backward gate
 *     [H > 0] reads the stored value.  Logits, loss and the output layer's (sigmoid(z) - y) / (batch * 128) are f32.
 *   Backward.  Every back-propagated dZ is rounded once when it is stored: the output layer's, and each hidden layer's and fc1's
 *     after gate and scale were applied in f32.  The weight gradient, the bias gradient and the data gradient of a layer all read
 *     that one rounded value.  The gradient with respect to the pooled features is the exception: it stays f32, and the conv
 *     gradients are computed from it as on an f32 handle.
 *   Sums.  Every product accumulates in f32; partial sums and every stored gradient are f32; every order is fixed by the shapes,
 *     nothing is accumulated atomically: equal inputs give equal bits, as in f32.
 * The handle holds in addition, in 16 bits: both orientations of every dense weight, and per row of max_batch both orientations of
 * the features, the hidden activations and the back-propagated gradients, rows padded to whole chunks of 32 values. */
pvq_status pvq_note_trainer_create_precision(int device_id, const pvq_note_model_params *params, const pvq_note_model_weights *weights,
                                             const pvq_note_trainer_hyper *hyper, uint32_t max_batch, pvq_note_precision precision,
                                             pvq_note_trainer **out);
/* the precision a handle was made with, a pvq_note_precision value (0, PVQ_NOTE_F32, for a null handle, as every getter answers
 * its zero); a pure query */
int pvq_note_trainer_precision(const pvq_note_trainer *t);
void pvq_note_trainer_destroy(pvq_note_trainer *t);
/* One step of `mode` (a pvq_train_mode) on the batch idx[0 .. batch) of the dataset (d_db, d_targets, n_rows), as laid out above.
 * d_loss (DEVICE, one float, may be NULL) receives the mean loss, d_logits (DEVICE, [batch][128], may be NULL) the logits; nothing
 * else outside the handle is written, and the call never synchronises.  A refused call launches nothing and leaves the counter.
 * Asynchronous on `stream`; the workspace belongs to the handle, so one handle serves one stream at a time. */
pvq_status pvq_note_trainer_step(pvq_note_trainer *t, int mode, const float *d_db, const float *d_targets, size_t n_rows, const uint32_t *idx,
                                 uint32_t batch, float *d_loss, float *d_logits, void *stream);
/* completed PVQ_TRAIN_STEP calls: Adam's t - 1 and the `step` of the dropout mask */
uint64_t pvq_note_trainer_steps(const pvq_note_trainer *t);
/* number of parameters: 96 + mlp_size (n_features + 1) + mlp_layers mlp_size (mlp_size + 1) + 128 (mlp_size + 1) */
uint64_t pvq_note_trainer_param_count(const pvq_note_trainer *t);
/* Copies array `what` (a pvq_train_array) to out_host, param_count floats (capacity: floats out_host holds, PVQ_ERR_INVALID_ARG if
 * fewer), in state_dict order and layout: conv1.weight [16][1][5], conv1.bias [16], fc1.weight [mlp_size][n_features], fc1.bias,
 * layers.i.weight [mlp_size][mlp_size], layers.i.bias for i = 0 .., output.weight [128][mlp_size], output.bias [128].
 * Synchronises the device. */
pvq_status pvq_note_trainer_read(pvq_note_trainer *t, int what, float *out_host, size_t capacity);
/* The dropout mask above as a pure host function: out_keep[j] = 1 when element (row, col0 + j) of hidden layer `layer` is kept at
 * `step`, else 0, for j in 0 .. n.  Needs no handle; PVQ_ERR_INVALID_ARG for a null array or a dropout outside [0, 1). */
pvq_status pvq_note_trainer_dropout_keep(uint64_t seed, uint64_t step, uint32_t layer, uint32_t row, uint32_t col0, uint32_t n, double dropout,
                                         uint8_t *out_keep);

/* The test pass of the trainer (pitchvis_train/train.py:164-198): model.eval(), the test set in batches, per batch
 * f1_score(labels > 0.5, outputs > 0.5, average='micro'), then the mean of those scores and the element-wise accuracy.
 *
 * Rows.  idx is a HOST array of n_idx sample indices (t_frames - 1 <= i < n_rows, as for a step; duplicates are legal and count once
 *   each), 1 <= n_idx <= 2^25.  Batch k is idx[k * batch .. min((k + 1) * batch, n_idx)): the last batch may be short and still
 *   counts as one batch in the mean, because the DataLoader keeps it (train.py:65).  The caller's permutation is the shuffle.
 *   batch >= 1 and is NOT bounded by max_batch: it shapes only the metric.  Dropout is off (model.eval()), so a row's forward
 *   depends on no other row: the forward runs in chunks of at most max_batch consecutive entries of idx, whatever `batch` is.
 * Decisions.  The prediction is z > 0 on the f32 logit z: sigmoid(z) > 0.5 (train.py:177) in exact arithmetic, and the rule of
 *   pvq_note_model_outputs.d_mask.  The two differ only for 0 < z <~ 6e-8, where the f32 sigmoid rounds to 0.5.  The label is
 *   y > 0.5 (train.py:178).  tp, fp, fn count the elements of a batch that are (predicted and labelled), (predicted, not
 *   labelled), (labelled, not predicted); `correct` those where prediction and label agree (train.py:190).
 * Loss.  Per element the stable form of the step (above), terms in f32; a row's 128 terms are added as a tree in double, a batch's
 *   rows in double in an order that depends only on its number of rows; `loss` is that sum / (rows * 128), the batch's mean BCE.
 * Scalars (pvq_note_test_metrics).  The F1 of a batch is 2 tp / (2 tp + fp + fn), and 0 when that denominator is 0 (sklearn's
 *   zero-division value); mean_f1 is the plain mean over the batches (train.py:193); accuracy is sum(correct) / (128 * sum(rows))
 *   (train.py:198); mean_loss is the plain mean of the batch losses, as running_loss / len(loader) is for training (train.py:162).
 * Determinism.  Equal handles and equal inputs give equal bits.  The logits may differ in their last bits between handles of
 *   different max_batch, and from pvq_note_trainer_step(PVQ_TRAIN_EVAL) on the same rows: the split of a product along K follows
 *   its number of rows, and a chunk has other rows than a batch. */
typedef struct pvq_note_test_batch {   /* one record per test batch, 32 bytes */
    uint32_t rows, tp, fp, fn, correct, _pad;
    double   loss;                      /* mean BCE of the batch: sum / (rows * 128) */
} pvq_note_test_batch;
/* One test pass over idx[0 .. n_idx) of the dataset (d_db, d_targets, n_rows: DEVICE, as for a step, never written).  out_batches
 * (HOST, ceil(n_idx / batch) records) receives one record per batch; out_pitch (HOST, [128][3] tp, fp, fn per output over the whole
 * pass, may be NULL) the counts behind a per-note F1; d_logits (DEVICE, [n_idx][128], may be NULL) the logits, row r those of
 * idx[r].  Bad arguments (a null d_db, d_targets, idx or out_batches, batch 0, n_idx outside 1 .. 2^25, an index outside
 * [t_frames - 1, n_rows)) give PVQ_ERR_INVALID_ARG with a message and launch nothing; a host-only handle returns PVQ_ERR_NO_DEVICE
 * after these checks, as pvq_note_trainer_step does.  The call runs on `stream`, is synchronous with respect to its host outputs and
 * waits on the stream once, at the end.  It neither advances pvq_note_trainer_steps nor touches the weights, the gradients or
 * Adam's moments.  Per-row records and masks (56 bytes per row of idx) live in a grow-only buffer of the handle, allocated by the
 * first pass that needs it. */
pvq_status pvq_note_trainer_test(pvq_note_trainer *t, const float *d_db, const float *d_targets, size_t n_rows,
                                 const uint32_t *idx, size_t n_idx, uint32_t batch,
                                 pvq_note_test_batch *out_batches /* host, ceil(n_idx / batch) */,
                                 uint32_t *out_pitch /* host [128][3] tp, fp, fn over the whole pass, or NULL */,
                                 float *d_logits /* device [n_idx][128] or NULL */, void *stream);
/* pure host: what train.py:193-198 prints, from the records (formulas above).  Each output may be NULL.  PVQ_ERR_INVALID_ARG for
 * null records, n_batches 0 or records without rows. */
pvq_status pvq_note_test_metrics(const pvq_note_test_batch *b, size_t n_batches,
                                 double *mean_f1, double *accuracy, double *mean_loss);

/* The epoch loop of the trainer (pitchvis_train/train.py:147-162): DataLoader(train_dataset, batch_size, shuffle=True), one
 * optimisation step per batch, running_loss / len(train_loader).
 *
 * Order.  The shuffle has no stateful generator either: the order of an epoch is a counter-based permutation of [0, n), a function
 *   of (seed, epoch, n) evaluated per element.  With mix as for the dropout mask, 64-bit unsigned arithmetic modulo 2^64 and n the
 *   number of samples:
 *       n == 1:  order(0) = 0.  Otherwise
 *       b      = max(2, bit_length(n - 1)) rounded up to an even number;  h = b / 2;  mask = 2^h - 1
 *       base   = mix(mix(seed + 0x9E3779B97F4A7C15 * (epoch + 1)) ^ 0x45504F4348)
 *       key_i  = mix(base ^ i)                                                      for i = 0 .. 3
 *       pass(x), x < 2^b:  l = x >> h;  r = x & mask;  four rounds i = 0 .. 3 of  (l, r) = (r, l ^ (mix(key_i ^ r) & mask));
 *                          the result is (l << h) | r
 *       order(j), j < n:   x = pass(j);  while x >= n: x = pass(x)
 *   pass is a four-round Feistel network, a bijection of [0, 2^b) whatever mix is; the walk along its cycle back below n makes order
 *   a bijection of [0, n).  2^b <= 4 n for n >= 2, so a walk is a few passes long.  pvq_note_epoch_order evaluates it on the host.
 * Batches.  idx is a HOST array of n_idx sample indices, the train split (1 <= n_idx <= 2^25; duplicates are legal).  Batch k is the
 *   samples idx[order(k * batch + r)], r = 0 .. min(batch, n_idx - k * batch), with n = n_idx: the last batch may be short and still
 *   counts, because the DataLoader keeps it (train.py:64).
 * Steps.  Each batch is one PVQ_TRAIN_STEP, with the bits of pvq_note_trainer_step called with that batch as its host idx at that
 *   counter: weights, gradients, moments, dropout keys, loss.  pvq_note_trainer_steps advances by ceil(n_idx / batch).
 * Loss.  out_losses[k] is the float d_loss would receive for batch k; out_mean_loss their sum in double, in batch order, divided by
 *   the number of batches (train.py:162). */
/* One epoch over the dataset (d_db, d_targets, n_rows: DEVICE, as for a step, never written).  out_losses (HOST, ceil(n_idx / batch)
 * floats) and out_mean_loss (HOST) may each be NULL.  Bad arguments (a null d_db, d_targets or idx, a batch outside 1 .. max_batch,
 * n_idx outside 1 .. 2^25, an index outside [t_frames - 1, n_rows)) give PVQ_ERR_INVALID_ARG with a message, launch nothing and leave
 * the counter; a host-only handle returns PVQ_ERR_NO_DEVICE after these checks.  idx goes to the device once per call; the split,
 * its order and the batch losses (8 bytes per entry of idx, 4 per batch) live in a grow-only buffer of the handle.  The call is a
 * loop of launches on `stream`, is synchronous with respect to its host outputs and waits on the stream once, at the end. */
pvq_status pvq_note_trainer_epoch(pvq_note_trainer *t, const float *d_db, const float *d_targets, size_t n_rows,
                                  const uint32_t *idx, size_t n_idx, uint32_t batch, uint64_t shuffle_seed, uint64_t epoch,
                                  float *out_losses /* host, ceil(n_idx / batch), or NULL */, double *out_mean_loss /* host or NULL */,
                                  void *stream);
/* pure host: out[j] = order(first + j) for j in 0 .. count, the order above for (seed, epoch, n).  PVQ_ERR_INVALID_ARG for n outside
 * 1 .. 2^32, first + count > n or a null out. */
pvq_status pvq_note_epoch_order(uint64_t seed, uint64_t epoch, uint64_t n, uint64_t first, uint64_t count, uint32_t *out);
/* The inverse of pvq_note_trainer_read: array `what` (a pvq_train_array) of the handle is replaced by host[0 .. count), in
 * state_dict order and layout; count must equal pvq_note_trainer_param_count (PVQ_ERR_INVALID_ARG otherwise, as for an unknown
 * array or a null host).  On a PVQ_NOTE_BF16 handle writing PVQ_TRAIN_WEIGHTS refreshes the 16-bit shadow, as a step's Adam does.
 * Synchronises the device; a host-only handle returns PVQ_ERR_NO_DEVICE after the checks. */
pvq_status pvq_note_trainer_write(pvq_note_trainer *t, int what, const float *host, size_t count);
/* Sets the counter pvq_note_trainer_steps reports (Adam's t - 1, the `step` of the dropout mask); steps < 2^53.  The weights and both
 * moments written back and the counter set make a handle continue a run with the bits of the handle they were read from. */
pvq_status pvq_note_trainer_set_steps(pvq_note_trainer *t, uint64_t steps);

/* Page-locked host memory for the host-buffer entry points (pvq_vqt_calculate_batch_db, pvq_analyze_batch,
 * pvq_train_frames_db): with pageable buffers those calls are bound by staged PCIe copies (~16 GB/s); buffers from
 * here are DMA-able directly.  NULL on failure (pvq_last_error). */
void *pvq_host_alloc(size_t bytes);
void pvq_host_free(void *p);

/* timing hook for bench.py: elapsed GPU milliseconds of the dominant kernel launches of the
 * last batch call, measured with HIP events on the stream the kernels were launched on.
 * Enable with pvq_vqt_set_profiling(v, 1) (resets the statistics); reading synchronises.  enable == 2 times only the transform's
 * main kernel (the fused GEMM + tree, or the FFT-path kernel): two event records per step instead of eight — the events themselves
 * cost ~3 us each on the stream. */
pvq_status pvq_vqt_set_profiling(pvq_vqt *v, int enable);
/* out_ms[i] for kernel slot i (see pvq_vqt_kernel_name); returns the number of slots filled */
uint32_t pvq_vqt_last_kernel_ms(pvq_vqt *v, float *out_ms, uint32_t capacity);
/* out_n[i] = launches of kernel slot i recorded since profiling was enabled (a batch call may
 * launch a kernel once per sub-batch); out_ms above is the mean per launch */
uint32_t pvq_vqt_last_kernel_launches(pvq_vqt *v, uint32_t *out_n, uint32_t capacity);
/* flop issued by the matrix instructions of the last block-DFT GEMM launch (tiles x rows x columns x depth x 2, padding and
 * recomputed rows included); 0 after a call that took the FFT path */
double pvq_vqt_last_gemm_flop(const pvq_vqt *v);
/* shader clock (MHz) the chip held inside the GEMM kernel's K loop during the last profiled launch: median over sampled
 * workgroups of shader-clock ticks / 100 MHz ticks; 0 if nothing was measured.  Synchronises the device. */
float pvq_vqt_last_sclk_mhz(pvq_vqt *v);
/* frames one launch of the frame kernels processed in the last batch call (the sub-batch size) */
uint32_t pvq_vqt_last_frames_per_launch(const pvq_vqt *v);
const char *pvq_vqt_kernel_name(uint32_t slot);

/* ---- the synth stage: SoundFont voices rendered for many streams ---------------------------------------------------
 * The first link of the trainer's chain (pitchvis_train/src/train.rs:252-351): MIDI-style events -> rustysynth_fork -> left / right
 * PCM and the active voices whose keys become the targets.  The work splits at the 64-sample block.  The CONTROL rate (once per
 * voice and block: both envelopes, both LFOs, pitch, filter coefficients, mix gains, and every decision about which voices exist)
 * runs on the host and emits a PLAN: per block the records of the voices that sound, in the reference's active-list order, which is
 * the order of the sum.  The AUDIO rate (oscillator.rs:112-176, bi_quad_filter.rs:77-99, synthesizer.rs:478-495) replays the plan,
 * on the host (pvq_synth_state_render) and on the device (pvq_synth_batch_render_device) with one copy of the arithmetic: integer
 * ops and unfused IEEE f32 in the written order, so both give the same bits.
 * The plain create entries give the reference with enable_reverb_and_chorus = false (the dry path).  train.rs:264 uses the
 * reference's default (on): the _ex entries with PVQ_SYNTH_EFFECTS add reverb and chorus (synthesizer.rs:393-475, reverb.rs,
 * chorus.rs), and the rows are then the trainer's exact PCM.  With effects the control rate also gives every record its chorus and
 * reverb gains (pvq_synth_sends), and the audio rate adds three more sums per block (chorus input left / right, reverb input), the
 * chorus (no feedback: a function of present and past inputs), the reverb (8 combs in parallel, whose filter_store is the one
 * recurrence from sample to sample, then 4 all-passes in series, per channel) and dry + 0.5 chorus + 0.5 reverb.  The effect state
 * of a stream (24 reverb buffers, 2 chorus rings: 51 KB at 22 050 Hz, 443 KB at 192 000) starts at zero and lives in the handle.
 * Left out: SF2 and MIDI file parsing (arrays in); play_loop; polyphony above 64; block sizes other than 64; the control rate on
 * the device. */
#define PVQ_SYNTH_GENERATORS 61 /* generator_type.rs:71 */
#define PVQ_SYNTH_BLOCK 64      /* SynthesizerSettings::DEFAULT_BLOCK_SIZE */
#define PVQ_SYNTH_EFFECTS 1u    /* flag of the _ex create entries: enable_reverb_and_chorus (synthesizer_settings.rs) */
/* One sounding voice in one block (64 bytes).  flags: 1 started since its last record (position := start, filter memory cleared),
 * 2 looping, 4 filter active, 8 a sample without a loop ends inside this block. */
typedef struct pvq_synth_record {
    uint32_t voice;              /* the voice object 0 .. maximum_polyphony - 1 */
    uint32_t flags;
    uint32_t ratio_lo, ratio_hi; /* pitch_ratio_fp, i64 (oscillator.rs:103) */
    float a[5];                  /* BiQuadFilter a0 .. a4 */
    float gain[4];               /* previous left, current left, previous right, current right, times master_volume */
    uint32_t desc;               /* the instrument region whose sample points a started voice reads */
    int32_t key;
    uint32_t stage;              /* volume envelope stage 0 delay 1 attack 2 hold 3 decay 4 release */
} pvq_synth_record;
/* The effect gains of one record (32 bytes), parallel to the records of a plan made with PVQ_SYNTH_EFFECTS.  The mix gains in them
 * are NOT times master_volume (synthesizer.rs:404-415, 449-454). */
typedef struct pvq_synth_sends {
    float chorus[4];             /* previous left, current left, previous right, current right: chorus send * mix gain */
    float reverb[2];             /* previous, current: (0.015 * reverb send) * (mix gain left + mix gain right) */
    uint32_t pad[2];
} pvq_synth_sends;
/* replaces SoundFont::new (soundfont.rs) after parsing.  wave_data [n_wave] int16; samples [n_samples][7] = start, end, start_loop,
 * end_loop, sample_rate, original_pitch, pitch_correction (sample_header.rs); instrument_gs [n_instrument_regions][61]: a region's
 * generators after the defaults and its zones (instrument_region.rs:39-66), instrument_sample [n_instrument_regions] its sample;
 * instruments [n_instruments][2] = first region, regions; preset_gs [n_preset_regions][61] (preset_region.rs:32-42),
 * preset_instrument its instrument; presets [n_presets][4] = bank, patch, first region, regions.  PVQ_ERR_INVALID_ARG names the
 * first bad index: a sample or instrument id out of range (the reference's InvalidSampleId / InvalidInstrumentId), a region range
 * past its array, a sample point (with the region's address offsets) outside 0 .. n_wave, a sample rate that is not positive, an original pitch
 * outside 0 .. 255 or a pitch correction outside -128 .. 127 (the file's u8 and i8). */
typedef struct pvq_synth_bank pvq_synth_bank;
pvq_status pvq_synth_bank_create(const int16_t *wave_data, size_t n_wave, const int32_t *samples, uint32_t n_samples,
                                 const int16_t *instrument_gs, const uint32_t *instrument_sample, uint32_t n_instrument_regions,
                                 const uint32_t *instruments, uint32_t n_instruments, const int16_t *preset_gs,
                                 const uint32_t *preset_instrument, uint32_t n_preset_regions, const int32_t *presets, uint32_t n_presets,
                                 pvq_synth_bank **out);
void pvq_synth_bank_destroy(pvq_synth_bank *b);   /* handles made from it keep their own reference */
/* out4: wave values, instrument regions, preset regions, presets */
pvq_status pvq_synth_bank_counts(const pvq_synth_bank *b, uint64_t *out4);
/* replaces Synthesizer::new + MidiFileSequencer (synthesizer.rs:58-174, midifile_sequencer.rs) for ONE stream on the host.
 * sample_rate 16 000 .. 192 000 and maximum_polyphony 8 .. 256 as synthesizer_settings.rs:35-57 (its texts); above 64:
 * PVQ_ERR_UNSUPPORTED. */
typedef struct pvq_synth_state pvq_synth_state;
pvq_status pvq_synth_state_create(const pvq_synth_bank *bank, int32_t sample_rate, uint32_t maximum_polyphony, pvq_synth_state **out);
/* the same with flags: 0 is exactly pvq_synth_state_create; PVQ_SYNTH_EFFECTS adds reverb and chorus; any other bit:
 * PVQ_ERR_INVALID_ARG */
pvq_status pvq_synth_state_create_ex(const pvq_synth_bank *bank, int32_t sample_rate, uint32_t maximum_polyphony, uint32_t flags,
                                     pvq_synth_state **out);
void pvq_synth_state_destroy(pvq_synth_state *s);
/* replaces MidiFileSequencer::render (midifile_sequencer.rs:52-104) over n_blocks blocks: left / right [n_blocks * 64].  The five
 * event arrays [n_events] are the stream's WHOLE list (times in seconds, ascending; channel, command, data1, data2 each 0 .. 255,
 * Synthesizer::process_midi_message's arguments, synthesizer.rs:176-213); the state keeps how many it has consumed, so calls
 * continue one another and a render in several calls equals one call.  Before each block every event with time <= current_time is
 * applied, and current_time grows by the repeated f64 addition of 64 / sample_rate.  snapshot_blocks [n_snapshots] (ascending
 * block numbers of this call, may be NULL with 0): the active voices after that block, for pvq_synth_state_get_snapshots.
 * Where the reference would panic on a read outside wave_data (a loop shorter than the pitch step: oscillator.rs:155-172), the call
 * ends with PVQ_ERR_INVALID_ARG naming stream, block and key before a sample is made; the state is then no longer usable. */
pvq_status pvq_synth_state_render(pvq_synth_state *s, const double *time_s, const int32_t *channel, const int32_t *command,
                                  const int32_t *data1, const int32_t *data2, size_t n_events, size_t n_blocks,
                                  const uint32_t *snapshot_blocks, size_t n_snapshots, float *left, float *right);
/* replaces Synthesizer::get_active_voices (synthesizer.rs:525; key, current_mix_gain_left, current_mix_gain_right of voice.rs:38-48)
 * after each snapshot block of the last render: out_counts [0] snapshots taken, [1] voices in all.  voice_ptr [ptr_capacity] (at
 * least snapshots + 1) indexes key / gain_left / gain_right [capacity]; any of them may be NULL to ask for the counts alone.
 * These are pvq_train_rows' voice arrays. */
pvq_status pvq_synth_state_get_snapshots(const pvq_synth_state *s, uint32_t *out_counts, uint32_t *voice_ptr, size_t ptr_capacity,
                                         int32_t *key, float *gain_left, float *gain_right, size_t capacity);
/* the plan of the last render: out_counts [0] blocks, [1] records.  block_ptr [ptr_capacity] (at least blocks + 1) indexes
 * records [capacity]; NULL to ask for the counts alone. */
pvq_status pvq_synth_state_get_plan(const pvq_synth_state *s, uint32_t *out_counts, uint32_t *block_ptr, size_t ptr_capacity,
                                    pvq_synth_record *records, size_t capacity);
/* the sends of the last render's plan, shaped like pvq_synth_state_get_plan: out_counts [0] blocks, [1] sends (one per record).
 * A state made without PVQ_SYNTH_EFFECTS has none: both counts are 0. */
pvq_status pvq_synth_state_get_sends(const pvq_synth_state *s, uint32_t *out_counts, uint32_t *block_ptr, size_t ptr_capacity,
                                     pvq_synth_sends *sends, size_t capacity);
uint32_t pvq_synth_state_active_voices(const pvq_synth_state *s);   /* VoiceCollection::active_voice_count */
/* The same for MANY streams: the planner on the host (at most 16 threads), the audio rate on the device, a wavefront per stream
 * and a lane per voice object.  device_id < 0: a host-only handle whose render returns PVQ_ERR_NO_DEVICE after its argument checks. */
typedef struct pvq_synth_batch pvq_synth_batch;
pvq_status pvq_synth_batch_create(int device_id, const pvq_synth_bank *bank, uint32_t n_streams, int32_t sample_rate,
                                  uint32_t maximum_polyphony, pvq_synth_batch **out);
/* the same with flags, as pvq_synth_state_create_ex.  With PVQ_SYNTH_EFFECTS the handle also owns every stream's effect state on
 * the device, zeroed here, and its render replays the plan with a second kernel. */
pvq_status pvq_synth_batch_create_ex(int device_id, const pvq_synth_bank *bank, uint32_t n_streams, int32_t sample_rate,
                                     uint32_t maximum_polyphony, uint32_t flags, pvq_synth_batch **out);
void pvq_synth_batch_destroy(pvq_synth_batch *b);
/* pvq_synth_state_render for every stream: event_ptr [n_streams + 1] indexes the five event arrays (stream s owns
 * [event_ptr[s], event_ptr[s + 1]), its whole list); n_blocks [n_streams]; d_left / d_right are HOST arrays of n_streams DEVICE
 * pointers to rows of n_blocks[s] * 64 floats (4-byte aligned; nothing past them is written; a stream without events gets zeros):
 * what pvq_agc_batch_condition_device takes.  snapshot_blocks is shared by the streams.  Every lane's position and filter memory
 * stay on the device and every stream's control state on the host between calls.  The planner runs before anything is launched:
 * its PVQ_ERR_INVALID_ARG (see pvq_synth_state_render) leaves the rows untouched and the handle unusable.  Asynchronous on
 * `stream`; the calls of one handle go to one stream. */
pvq_status pvq_synth_batch_render_device(pvq_synth_batch *b, const uint64_t *event_ptr, const double *time_s, const int32_t *channel,
                                         const int32_t *command, const int32_t *data1, const int32_t *data2, const size_t *n_blocks,
                                         float *const *d_left, float *const *d_right, const uint32_t *snapshot_blocks,
                                         size_t n_snapshots, void *stream);
/* What the last render cost, in ms: out_ms4 [0] the planner's host time, [1] the host time spent laying the plan out for the upload,
 * [2] the device time of the upload, [3] of the replay kernel (waits for the call's end); out_records (may be NULL): the
 * voice-blocks it replayed. */
pvq_status pvq_synth_batch_last_times(pvq_synth_batch *b, float *out_ms4, uint64_t *out_records);
/* pvq_synth_state_get_snapshots for stream `stream_index` of the last render (host data: does not synchronise) */
pvq_status pvq_synth_batch_get_snapshots(const pvq_synth_batch *b, uint32_t stream_index, uint32_t *out_counts, uint32_t *voice_ptr,
                                         size_t ptr_capacity, int32_t *key, float *gain_left, float *gain_right, size_t capacity);
/* Reverb + Chorus alone (Reverb::new, Chorus::new(sample_rate, 0.002, 0.0019, 0.4): synthesizer.rs:102-126) on the host, fed with
 * chosen inputs: the code the host face's effect path runs.  sample_rate as pvq_synth_state_create's. */
typedef struct pvq_synth_effects_s pvq_synth_effects;
pvq_status pvq_synth_effects_create(int32_t sample_rate, pvq_synth_effects **out);
void pvq_synth_effects_destroy(pvq_synth_effects *e);
/* Chorus::process and Reverb::process over n_blocks * 64 samples: the chorus inputs left / right and the (mono) reverb input in,
 * the chorus outputs left / right and the reverb outputs left / right out.  The state goes on from call to call. */
pvq_status pvq_synth_effects_process(pvq_synth_effects *e, size_t n_blocks, const float *chorus_in_left, const float *chorus_in_right,
                                     const float *reverb_in, float *chorus_out_left, float *chorus_out_right, float *reverb_out_left,
                                     float *reverb_out_right);
/* the chorus delay table (chorus.rs:24-29): returns its length, round(sample_rate / 0.4), and fills out [capacity] when it is
 * large enough (out may be NULL); 0 for a sample rate outside 16 000 .. 192 000 */
uint32_t pvq_synth_chorus_table(int32_t sample_rate, float *out, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* PVQ_H */
