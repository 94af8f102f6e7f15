// render_batch.hip — spectrogram rows, chroma and LED frames for many rows, a wavefront per row (render_batch.hpp).
//
// Every arithmetic step is spectrogram_row's / chroma_row's / led_frame's (consumers_host.cpp, itself the reference's f32 expressions,
// file:line cited there; the colour conversions are the very same source, color_math.hpp) with FMA contraction off, the correctly
// rounded fp32 division hipcc emits for a plain `/`, and fp32 subnormals kept — what differs from the host is the device's libm
// (powf, expf, cosf, sinf) alone.
//
// One 64-lane workgroup walks rows blockIdx.x, + gridDim.x, ...; lane l owns bins l, l + 64, ... of the row (NK of them: an
// instantiation knows its bin count's 64-chunk).  What depends on geometry and palette alone comes from the host once and sits in
// LDS: the colour of every bin's bucket (as u8 and as the finished texel), (L, C, h) of the twelve palette entries, and the bins of
// every pitch class in ascending order.
//
// The reference's two sequential-overwrite loops over peaks (update.rs:1017-1063: a later peak repaints what an earlier one painted;
// main.rs:131-140: x[lower], x[lower + 1]) are evaluated per bin: a lane per PEAK computes what the peak would write (its colour, its
// brightness, its two LED values) and enters its list index into every bin it covers with an LDS max; a lane per BIN then takes the
// entry that is left — the last peak in list order that covers it — and finishes its own pixel.  Peaks go through in chunks of 64 in
// list order (one chunk unless a row has more than 64), a later chunk overwriting an earlier one's bins, so any list gives what the
// sequential loop leaves.
//
// Chroma: all lanes take 10^(v / 10) of their bins into LDS, then twelve lanes each add up their class's bins in ascending order —
// per class the reference's order of additions (update.rs:1112-1123).
#include "render_batch.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "color_math.hpp"
#include "consumers_host.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
constexpr uint32_t MAX_BINS = 1024;

// built by the host at create, read-only afterwards
struct RenderTables {
    uint32_t bin_rgb[MAX_BINS];     // r | g << 8 | b << 16: calculate_color at (bin + bpo - 3 (bpo / 12)) % bpo, the u8 of lib.rs:108
    uint32_t bin_texel[MAX_BINS];   // the same through update.rs:998-1000: (c / 255 * 255 * 1.2).clamp(0, 255) as u8
    float lch[12][3];               // lib.rs:98 of every palette entry
    uint16_t class_bins[MAX_BINS];  // bins ordered by (pitch class, bin): update.rs:1115-1118
    uint16_t class_start[16];       // class k: class_bins[class_start[k] .. class_start[k + 1])
};

struct RenderArgs {
    const float* x;
    const float* center;
    const float* size;
    const uint32_t* peak_count;
    uint32_t max_peaks, n_rows;
    int n_bins;
    uint32_t bpo;
    float semitone_offset, gray_level, easing_pow;
    const RenderTables* tab;
    uint8_t* out_vqt;
    uint8_t* out_peaks;
    float* out_chroma;
    uint8_t* out_led;
};

// pitchvis_colors/src/lib.rs:19-36
const float DEFAULT_COLORS[12][3] = {
    {0.85f, 0.36f, 0.36f}, {0.01f, 0.52f, 0.71f}, {0.97f, 0.76f, 0.05f}, {0.45f, 0.34f, 0.63f}, {0.47f, 0.77f, 0.22f}, {0.78f, 0.32f, 0.52f},
    {0.00f, 0.64f, 0.56f}, {0.95f, 0.54f, 0.23f}, {0.30f, 0.37f, 0.64f}, {1.00f, 0.96f, 0.03f}, {0.57f, 0.30f, 0.55f}, {0.12f, 0.71f, 0.34f},
};

__device__ __forceinline__ float wave_max_ignoring_nan(float v) {   // f32::max over the wave: order-independent for non-NaN values
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

template <int NK>   // 64 (NK - 1) < n_bins <= 64 NK (the host's promise: the chunk tests fold away)
__global__ __launch_bounds__(64) void render_rows(RenderArgs a) {
#pragma clang fp contract(off)
    using namespace color;
    constexpr int NB = 64 * NK;
    __builtin_assume(a.n_bins > 64 * (NK - 1) && a.n_bins <= NB);
    __shared__ uint32_t s_rgb[NB];
    __shared__ uint32_t s_texel[NB];
    __shared__ float s_lch[36];
    __shared__ uint16_t s_cbins[NB];
    __shared__ uint16_t s_cstart[16];
    __shared__ float s_unit[256];        // k / 255.0f (lib.rs:110-114)
    __shared__ float s_pow[NB];          // update.rs:1121 of the row
    __shared__ uint32_t s_own[NB];       // spectrogram: 1 + the chunk's last peak whose footprint covers the bin, 0: none
    __shared__ uint32_t s_ownl[NB];      // LED: the same for x[lower] / x[lower + 1]
    __shared__ float s_pk_c[64], s_pk_b[64], s_led_lo[64], s_led_hi[64];
    __shared__ uint32_t s_pk_rgb[64];
    __shared__ int s_led_bin[64];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[3 * NB + 16];   // the LED frame, placed at the row's offset within a dword

    const int lane = threadIdx.x;
    const int n = a.n_bins;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int bin = lane + 64 * k;
        if (bin < n) {
            s_rgb[bin] = a.tab->bin_rgb[bin];
            s_texel[bin] = a.tab->bin_texel[bin];
            s_cbins[bin] = a.tab->class_bins[bin];
        }
    }
    if (lane < 36) s_lch[lane] = (&a.tab->lch[0][0])[lane];
    if (lane < 16) s_cstart[lane] = a.tab->class_start[lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) s_unit[lane + 64 * j] = static_cast<float>(lane + 64 * j) / 255.0f;
    __syncthreads();

    const bool do_x = a.out_vqt || a.out_chroma;
    const bool do_pk = a.out_peaks || a.out_led;
    const float bpo_f = static_cast<float>(a.bpo);
    const float width = static_cast<float>(n);

    for (uint32_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
        if (do_x) {
            const float* xr = a.x + static_cast<size_t>(row) * n;
            float v[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int bin = lane + 64 * k;
                v[k] = bin < n ? xr[bin] : 0.0f;
            }
            if (a.out_vqt) {   // update.rs:962-1004
                float m = 0.0f;
#pragma unroll
                for (int k = 0; k < NK; ++k) m = fmaxf(m, v[k]);   // update.rs:967 (a lane past the row holds 0, the fold's start)
                const float max_val = wave_max_ignoring_nan(m);
                uint32_t* o = reinterpret_cast<uint32_t*>(a.out_vqt) + static_cast<size_t>(row) * n;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int bin = lane + 64 * k;
                    if (bin < n) {
                        float brightness = 0.0f;
                        if (max_val > 0.0f) brightness = brightness_of(1.0f - v[k] / (max_val + 0.001f));   // update.rs:974-979
                        o[bin] = s_texel[bin] | (static_cast<uint32_t>(texel_u8(brightness)) << 24);        // update.rs:998-1001
                    }
                }
            }
            if (a.out_chroma) {   // update.rs:1102-1131
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int bin = lane + 64 * k;
                    if (bin < n) s_pow[bin] = powf(10.0f, v[k] / 10.0f);   // update.rs:1121
                }
                __syncthreads();
                float acc = 0.0f;
                if (lane < 12) {
                    const int e = s_cstart[lane + 1];
                    for (int i = s_cstart[lane]; i < e; ++i) acc = acc + s_pow[s_cbins[i]];   // update.rs:1122, ascending bins of the class
                }
                const float max_chroma = wave_max_ignoring_nan(lane < 12 ? acc : 0.0f);       // update.rs:1126
                if (lane < 12) a.out_chroma[static_cast<size_t>(row) * 12 + lane] = max_chroma > 0.0f ? acc / max_chroma : acc;
            }
        }
        if (do_pk) {
            const uint32_t cnt = min(a.peak_count[row], a.max_peaks);
            const float* c_row = a.center + static_cast<size_t>(row) * a.max_peaks;
            const float* z_row = a.size + static_cast<size_t>(row) * a.max_peaks;
            float max_size = 0.0f;
            if (a.out_peaks) {   // update.rs:1010-1014
                for (uint32_t p = lane; p < cnt; p += 64) max_size = fmaxf(max_size, z_row[p]);
                max_size = wave_max_ignoring_nan(max_size);
            }
            const bool paint = a.out_peaks && max_size > 0.0f;   // update.rs:1016
            uint32_t px[NK];
            float xl[NK];   // main.rs:130
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                px[k] = 0u;
                xl[k] = 0.0f;
            }
            for (uint32_t base = 0; base < cnt; base += 64) {
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    s_own[lane + 64 * k] = 0u;
                    s_ownl[lane + 64 * k] = 0u;
                }
                __syncthreads();
                const uint32_t p = base + lane;
                if (p < cnt) {
                    const float c = c_row[p], sz = z_row[p];
                    if (paint) {   // update.rs:1017-1039 for this lane's peak
                        uint32_t tone;
                        float inaccuracy;
                        tone_of_bucket(a.bpo, fmodf(c + a.semitone_offset, bpo_f), tone, inaccuracy);
                        uint8_t rgb[3];
                        lch_color_u8(s_lch[3 * tone], s_lch[3 * tone + 1], s_lch[3 * tone + 2], inaccuracy, a.gray_level, a.easing_pow, rgb);
                        s_pk_c[lane] = c;
                        s_pk_b[lane] = brightness_of(1.0f - sz / max_size);
                        s_pk_rgb[lane] = static_cast<uint32_t>(texel_u8(s_unit[rgb[0]])) | (static_cast<uint32_t>(texel_u8(s_unit[rgb[1]])) << 8) |
                                         (static_cast<uint32_t>(texel_u8(s_unit[rgb[2]])) << 16);
                        const float lo_f = fmaxf(floorf(c - 2.0f), 0.0f), hi_f = fminf(ceilf(c + 2.0f), width);
                        const int lo = lo_f >= width ? n : static_cast<int>(lo_f);
                        const int hi = hi_f > 0.0f ? static_cast<int>(hi_f) : 0;
#pragma unroll
                        for (int j = 0; j < 5; ++j) {   // floor(c - 2) .. ceil(c + 2) holds at most five bins; past them |bin - c| > 2
                            const int bin = lo + j;
                            if (bin < hi && fabsf(static_cast<float>(bin) - c) <= 2.0f) atomicMax(&s_own[bin], static_cast<uint32_t>(lane) + 1u);
                        }
                    }
                    if (a.out_led) {   // main.rs:131-140 for this lane's peak
                        const float fl = floorf(c);
                        if (fl >= 0.0f && fl < width) {
                            const int lower = static_cast<int>(fl);
                            const float pw = powf(c - truncf(c), 1.9f);
                            s_led_bin[lane] = lower;
                            s_led_lo[lane] = sz * (1.0f - pw);
                            s_led_hi[lane] = sz * pw;
                            atomicMax(&s_ownl[lower], static_cast<uint32_t>(lane) + 1u);
                            if (lower < n - 1) atomicMax(&s_ownl[lower + 1], static_cast<uint32_t>(lane) + 1u);
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int bin = lane + 64 * k;
                    if (bin < n) {
                        const uint32_t o = s_own[bin];
                        if (o) {   // update.rs:1042-1059
                            const float distance = fabsf(static_cast<float>(bin) - s_pk_c[o - 1]);
                            const float falloff = expf(-distance * distance / (2.0f * 2.0f * 0.5f));
                            px[k] = s_pk_rgb[o - 1] | (static_cast<uint32_t>(texel_u8(s_pk_b[o - 1] * falloff)) << 24);
                        }
                        const uint32_t ol = s_ownl[bin];
                        if (ol) xl[k] = s_led_bin[ol - 1] == bin ? s_led_lo[ol - 1] : s_led_hi[ol - 1];
                    }
                }
                __syncthreads();
            }
            if (a.out_peaks) {
                uint32_t* o = reinterpret_cast<uint32_t*>(a.out_peaks) + static_cast<size_t>(row) * n;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int bin = lane + 64 * k;
                    if (bin < n) o[bin] = px[k];
                }
            }
            if (a.out_led) {   // main.rs:142-170
                float best = -3.40282347e+38f;   // util::arg_max (util.rs:34-45): fold from f32::MIN with `>`; only the value is used
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    if (lane + 64 * k < n && xl[k] > best) best = xl[k];
                for (int o = 32; o; o >>= 1) {
                    const float other = __shfl_xor(best, o);
                    best = other > best ? other : best;
                }
                const size_t len = 3 + 3 * static_cast<size_t>(n);
                uint8_t* g = a.out_led + static_cast<size_t>(row) * len;
                const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(g) & 3);
                uint8_t* st = s_stage + mis;
                if (lane == 0) {
                    st[0] = 0xFF;                                        // main.rs:146
                    st[1] = static_cast<uint8_t>((n & 0xFFFF) / 256);    // main.rs:148-150
                    st[2] = static_cast<uint8_t>((n & 0xFFFF) % 256);
                }
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int bin = lane + 64 * k;
                    if (bin < n) {
                        const uint32_t rgb = s_rgb[bin];
                        const float coef = 1.0f - (1.0f - xl[k] / best);   // main.rs:162
                        st[3 + 3 * bin] = sat_u8((s_unit[rgb & 255u] * coef) * 254.0f);   // main.rs:163-167
                        st[4 + 3 * bin] = sat_u8((s_unit[(rgb >> 8) & 255u] * coef) * 254.0f);
                        st[5 + 3 * bin] = sat_u8((s_unit[(rgb >> 16) & 255u] * coef) * 254.0f);
                    }
                }
                __syncthreads();
                // s_stage and the row's first aligned dword in memory line up: whole dwords in between, single bytes at either end
                uint8_t* ga = g - mis;
                const int end = mis + static_cast<int>(len);
                const int fb = (mis + 3) & ~3, fe = end & ~3;
                for (int o = fb + 4 * lane; o < fe; o += 256) *reinterpret_cast<uint32_t*>(ga + o) = *reinterpret_cast<const uint32_t*>(s_stage + o);
                if (lane < fb - mis) ga[mis + lane] = s_stage[mis + lane];
                if (lane < end - fe) ga[fe + lane] = s_stage[fe + lane];
            }
        }
        __syncthreads();   // s_pow and s_stage are the next row's
    }
}

template <int NK>
void launch_nk(int nk, const RenderArgs& a, dim3 grid, hipStream_t stream) {
    if constexpr (NK > 16) {
        return;
    } else {
        if (nk == NK)
            hipLaunchKernelGGL(render_rows<NK>, grid, dim3(64), 0, stream, a);
        else
            launch_nk<NK + 1>(nk, a, grid, stream);
    }
}
}  // namespace

pvq_status RenderBatch::create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave, const float* colors,
                               float gray_level, float easing_pow, std::unique_ptr<RenderBatch>& out) {
    out.reset();
    if (!(min_freq > 0.0f) || octaves == 0 || buckets_per_octave == 0) {
        set_last_error("invalid VqtRange");
        return PVQ_ERR_INVALID_ARG;
    }
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (n < 3 || n > MAX_BINS) {
        set_last_error("unsupported: the batched render takes 3 .. 1024 bins");
        return PVQ_ERR_UNSUPPORTED;
    }
    const float(*pal)[3] = colors ? reinterpret_cast<const float(*)[3]>(colors) : DEFAULT_COLORS;
    std::unique_ptr<RenderBatch> b(new RenderBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_bins_ = static_cast<uint32_t>(n);
    b->bpo_ = buckets_per_octave;
    b->gray_level_ = gray_level;
    b->easing_pow_ = easing_pow;
    const uint32_t shift = buckets_per_octave - 3u * (buckets_per_octave / 12u);   // update.rs:982-984, main.rs:154
    b->semitone_offset_ = static_cast<float>(shift);
    if (device_id >= 0) {
        std::vector<RenderTables> host(1);
        RenderTables& t = host[0];
        std::fill(reinterpret_cast<char*>(&t), reinterpret_cast<char*>(&t + 1), 0);
        const uint16_t bpo16 = static_cast<uint16_t>(buckets_per_octave);
        for (uint32_t bin = 0; bin < n; ++bin) {
            uint8_t rgb[3];
            calculate_color_u8(bpo16, std::fmod(static_cast<float>(bin) + b->semitone_offset_, static_cast<float>(buckets_per_octave)), pal,
                               gray_level, easing_pow, rgb);   // update.rs:985-992 = main.rs:155-160
            t.bin_rgb[bin] = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
            uint32_t tx = 0;
            for (int i = 0; i < 3; ++i) tx |= static_cast<uint32_t>(color::texel_u8(static_cast<float>(rgb[i]) / 255.0f)) << (8 * i);
            t.bin_texel[bin] = tx;
        }
        palette_lch(pal, t.lch);
        const int bin_0 = chroma_bin_0_pitch_class(min_freq);
        uint32_t at = 0;
        for (uint32_t k = 0; k < 12; ++k) {
            t.class_start[k] = static_cast<uint16_t>(at);
            for (uint32_t bin = 0; bin < n; ++bin)
                if (chroma_pitch_class(bin, bpo16, bin_0) == k) t.class_bins[at++] = static_cast<uint16_t>(bin);
        }
        for (uint32_t k = 12; k < 16; ++k) t.class_start[k] = static_cast<uint16_t>(at);
        PVQ_HIP(hipSetDevice(device_id));
        if (pvq_status s = b->tab_.upload(&t, sizeof(RenderTables))) return s;
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status RenderBatch::rows_device(size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center, const float* d_size,
                                    const uint32_t* d_peak_count, uint32_t max_peaks, const pvq_render_outputs& outs, hipStream_t stream) {
    if ((outs.spectrogram_vqt || outs.chroma) && !d_x_vqt_smoothed) {
        set_last_error("render batch: spectrogram_vqt and chroma read x_vqt_smoothed, which is null");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((outs.spectrogram_peaks || outs.led) && (!d_center || !d_size || !d_peak_count || max_peaks == 0)) {
        set_last_error("render batch: spectrogram_peaks and led read center, size and peak_count, with max_peaks > 0");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(outs.spectrogram_vqt) | reinterpret_cast<uintptr_t>(outs.spectrogram_peaks)) & 3) {
        set_last_error("render batch: an RGBA output must be 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_rows > 0x7FFFFFFFull) {
        set_last_error("render batch: too many rows in one call");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched render runs on a GPU; this handle has none (pvq_spectrogram_row, pvq_chroma_row and pvq_led_frame are the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_rows == 0 || !(outs.spectrogram_vqt || outs.spectrogram_peaks || outs.chroma || outs.led)) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    RenderArgs a{};
    a.x = d_x_vqt_smoothed;
    a.center = d_center;
    a.size = d_size;
    a.peak_count = d_peak_count;
    a.max_peaks = max_peaks;
    a.n_rows = static_cast<uint32_t>(n_rows);
    a.n_bins = static_cast<int>(n_bins_);
    a.bpo = bpo_;
    a.semitone_offset = semitone_offset_;
    a.gray_level = gray_level_;
    a.easing_pow = easing_pow_;
    a.tab = tab_.as<RenderTables>();
    a.out_vqt = outs.spectrogram_vqt;
    a.out_peaks = outs.spectrogram_peaks;
    a.out_chroma = outs.chroma;
    a.out_led = outs.led;
    // a wave per row, rows strided over at most 32 resident waves per CU of a 256-CU chip: the tables reach LDS once per workgroup
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(n_rows, 256 * 32)));
    launch_nk<1>(static_cast<int>((n_bins_ + 63) / 64), a, grid, stream);
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

}  // namespace pvq
