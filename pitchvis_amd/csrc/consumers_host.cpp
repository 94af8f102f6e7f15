// consumers_host.cpp — see consumers_host.hpp.  Built with -ffp-contract=off: every expression below is the
// reference's f32 expression, operation for operation.
#include "consumers_host.hpp"

#include "color_math.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

namespace pvq {

// ---------------------------------------------------------------------------------------------------------
// dagc_fork/src/lib.rs
// ---------------------------------------------------------------------------------------------------------
bool MonoAgc::valid(float desired_output_rms, float distortion_factor, std::string* why) {
    if (!(desired_output_rms > 0.0f && std::isfinite(desired_output_rms))) {   // lib.rs:37-41
        if (why) *why = "`desired_output_rms` must be a finite positive number, but got " + std::to_string(desired_output_rms);
        return false;
    }
    if (!(distortion_factor >= 0.0f && distortion_factor <= 1.0f)) {           // lib.rs:42-46
        if (why) *why = "`distortion_factor` must be a number within `0.0 ..= 1.0`, but got " + std::to_string(distortion_factor);
        return false;
    }
    return true;
}

void MonoAgc::process(float* samples, size_t n) {   // lib.rs:76-86
    for (size_t i = 0; i < n; ++i) {
        float x = samples[i] * gain_;
        samples[i] = x;
        if (!frozen_) {
            const float y = (x * x) / desired_output_rms_;
            float g = 1.0f + (distortion_factor_ * (1.0f - y));
            g = std::fmax(g, distortion_factor_);   // f32::max (a NaN operand is ignored, like fmaxf)
            gain_ *= g;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// pitchvis_train/src/train.rs
// ---------------------------------------------------------------------------------------------------------
size_t train_chunk_samples(double delay_seconds, float sr) {
    // vqt.delay is Duration::from_secs_f32(..) (vqt.rs:756); as_millis() truncates
    const uint64_t delay_ms = static_cast<uint64_t>(delay_seconds * 1000.0);
    const size_t s = static_cast<size_t>(delay_ms) * static_cast<size_t>(sr) / 1000;   // train.rs:128 (SR is an integer constant)
    return (s / 64) * 64;                                                              // train.rs:129
}

void train_condition_stream(MonoAgc& agc, const float* left, const float* right, size_t n_chunks, size_t chunk, float* mono_out,
                            float* gain_out) {
    for (size_t c = 0; c < n_chunks; ++c) {
        float* dst = mono_out + c * chunk;
        const float* l = left + c * chunk;
        const float* r = right ? right + c * chunk : nullptr;
        float sq = 0.0f;
        for (size_t i = 0; i < chunk; ++i) {
            const float m = r ? (l[i] + r[i]) / 2.0f : l[i];   // train.rs:286-289
            dst[i] = m;
            sq += m * m;                                        // train.rs:292 (sequential f32 sum of powi(2))
        }
        agc.freeze_gain(sq < 1e-6f);                            // train.rs:293
        agc.process(dst, chunk);                                // train.rs:298-301 (the ring buffer's newest samples)
        if (gain_out) gain_out[c] = agc.gain();
    }
}

bool train_rows(const float* db, size_t n_frames, uint32_t n_bins, const uint32_t* voice_ptr, const int32_t* voice_key,
                const float* voice_gain_left, const float* voice_gain_right, const float* agc_gain, float* out_rows, std::string* why) {
    const size_t row_len = static_cast<size_t>(n_bins) + 128;
    std::map<int32_t, float> prev, cur;
    for (size_t f = 0; f < n_frames; ++f) {
        prev.swap(cur);   // train.rs:314
        cur.clear();
        for (uint32_t v = voice_ptr[f]; v < voice_ptr[f + 1]; ++v) {   // train.rs:317-337
            const float gain = (voice_gain_left[v] + voice_gain_right[v]) / 2.0f * agc_gain[f];
            auto it = cur.find(voice_key[v]);
            if (it != cur.end()) {
                if (gain > it->second) it->second = gain;
            } else {
                cur.emplace(voice_key[v], gain);
            }
        }
        float* row = out_rows + f * row_len;
        std::memcpy(row, db + f * static_cast<size_t>(n_bins), sizeof(float) * n_bins);   // train.rs:451
        float* targets = row + n_bins;
        for (int k = 0; k < 128; ++k) targets[k] = 0.0f;
        for (const auto& kv : prev) {                                                      // train.rs:456-458
            if (kv.first < 0 || kv.first >= 128) {
                if (why) *why = "midi key " + std::to_string(kv.first) + " outside 0..127";
                return false;
            }
            targets[kv.first] = (kv.second > 0.5f) ? 1.0f : 0.0f;
        }
    }
    return true;
}

bool npy_write_f32(const char* path, const float* data, uint64_t n, std::string* why) {
    // NumPy format 1.0: magic, version, u16 header length, ASCII dict padded with spaces to a multiple of 64, '\n'
    std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(n) + ",), }";
    size_t total = 10 + dict.size() + 1;
    const size_t pad = (64 - total % 64) % 64;
    dict.append(pad, ' ');
    dict.push_back('\n');
    FILE* fp = std::fopen(path, "wb");
    if (!fp) {
        if (why) *why = std::string("cannot open ") + path;
        return false;
    }
    const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    const uint16_t hl = static_cast<uint16_t>(dict.size());
    const unsigned char hlen[2] = {static_cast<unsigned char>(hl & 0xff), static_cast<unsigned char>(hl >> 8)};
    bool ok = std::fwrite(magic, 1, 8, fp) == 8 && std::fwrite(hlen, 1, 2, fp) == 2 &&
              std::fwrite(dict.data(), 1, dict.size(), fp) == dict.size() && (n == 0 || std::fwrite(data, sizeof(float), n, fp) == n);
    ok = (std::fclose(fp) == 0) && ok;
    if (!ok && why) *why = std::string("short write to ") + path;
    return ok;
}

// ---------------------------------------------------------------------------------------------------------
// pitchvis_colors/src/lib.rs; the conversions of the `lab` crate live in color_math.hpp (one copy for this unit and the
// render kernels).
// ---------------------------------------------------------------------------------------------------------
using color::sat_u8;

void palette_lch(const float colors[12][3], float out_lch[12][3]) {
    for (int t = 0; t < 12; ++t) {
        uint8_t base[3];
        for (int i = 0; i < 3; ++i) base[i] = sat_u8(colors[t][i] * 255.0f);                   // lib.rs:94-95
        color::rgb_to_lch(base, out_lch[t][0], out_lch[t][1], out_lch[t][2]);                  // lib.rs:98
    }
}

void calculate_color_u8(uint16_t buckets_per_octave, float bucket, const float colors[12][3], float gray_level, float easing_pow,
                        uint8_t rgb[3]) {
    uint32_t idx;
    float inaccuracy_cents;
    color::tone_of_bucket(buckets_per_octave, bucket, idx, inaccuracy_cents);                  // lib.rs:93-96
    uint8_t base[3];
    for (int i = 0; i < 3; ++i) base[i] = sat_u8(colors[idx][i] * 255.0f);                     // lib.rs:94-95
    float l, c, h;
    color::rgb_to_lch(base, l, c, h);                                                          // lib.rs:98
    color::lch_color_u8(l, c, h, inaccuracy_cents, gray_level, easing_pow, rgb);               // lib.rs:104-108
}

void calculate_color(uint16_t buckets_per_octave, float bucket, const float colors[12][3], float gray_level, float easing_pow,
                     float out_rgb[3]) {
    uint8_t rgb[3];
    calculate_color_u8(buckets_per_octave, bucket, colors, gray_level, easing_pow, rgb);
    for (int i = 0; i < 3; ++i) out_rgb[i] = static_cast<float>(rgb[i]) / 255.0f;
}

size_t led_frame(uint32_t n_buckets, uint16_t buckets_per_octave, const float* center, const float* size, uint32_t n_peaks,
                 const float colors[12][3], float gray_level, float easing_pow, uint8_t* out) {
    std::vector<float> x(n_buckets, 0.0f);                                      // main.rs:130
    for (uint32_t p = 0; p < n_peaks; ++p) {                                    // main.rs:131-140
        const float fl = std::floor(center[p]);
        if (!(fl >= 0.0f) || fl >= static_cast<float>(n_buckets)) continue;     // the reference would panic on an index out of range
        const size_t lower = static_cast<size_t>(fl);
        const float fract = center[p] - std::trunc(center[p]);                  // f32::fract
        x[lower] = size[p] * (1.0f - std::pow(fract, 1.9f));
        if (lower < n_buckets - 1) x[lower + 1] = size[p] * std::pow(fract, 1.9f);
    }
    // util::arg_max (util.rs:34-45): fold from f32::MIN, first maximum wins
    size_t k_max = 0;
    float best = -3.40282347e+38f;
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i] > best) {
            best = x[i];
            k_max = i;
        }
    const float max_size = x.empty() ? 0.0f : x[k_max];
    size_t o = 0;
    out[o++] = 0xFF;                                                            // main.rs:146
    const uint16_t num_triples = static_cast<uint16_t>(n_buckets);              // main.rs:148 (x_vqt_peakfiltered.len())
    out[o++] = static_cast<uint8_t>(num_triples / 256);
    out[o++] = static_cast<uint8_t>(num_triples % 256);
    const uint32_t shift = buckets_per_octave - 3u * (buckets_per_octave / 12u);   // main.rs:154
    for (uint32_t idx = 0; idx < n_buckets; ++idx) {
        float rgb[3];
        const float bucket = std::fmod(static_cast<float>(idx + shift), static_cast<float>(buckets_per_octave));
        calculate_color(buckets_per_octave, bucket, colors, gray_level, easing_pow, rgb);
        const float color_coefficient = 1.0f - (1.0f - x[idx] / max_size);       // main.rs:162
        for (int i = 0; i < 3; ++i) out[o++] = sat_u8((rgb[i] * color_coefficient) * 254.0f);   // main.rs:163-167
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------
// pitchvis_viewer/src/display_system/update.rs: the per-frame products that depend on AnalysisState alone
// ---------------------------------------------------------------------------------------------------------
void spectrogram_row(int mode, uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, const float* center,
                     const float* size, uint32_t n_peaks, const float colors[12][3], float gray_level, float easing_pow, uint8_t* out_rgba) {
    using color::brightness_of;
    using color::texel_u8;
    const float bpo = static_cast<float>(buckets_per_octave);
    const float semitone_offset = static_cast<float>(buckets_per_octave - 3u * (buckets_per_octave / 12u));   // update.rs:982-984
    if (mode == 0) {   // SpectrogramMode::VQT, update.rs:962-1004
        float max_val = 0.0f;
        for (uint32_t i = 0; i < n_buckets; ++i) max_val = std::fmax(max_val, x_vqt_smoothed[i]);   // update.rs:967 (f32::max ignores a NaN)
        for (uint32_t bin = 0; bin < n_buckets; ++bin) {
            const float value_db = x_vqt_smoothed[bin];
            float brightness = 0.0f;
            if (max_val > 0.0f) {                                                   // update.rs:974-979
                const float normalized = value_db / (max_val + 0.001f);
                brightness = brightness_of(1.0f - normalized);
            }
            uint8_t rgb[3];
            calculate_color_u8(buckets_per_octave, std::fmod(static_cast<float>(bin) + semitone_offset, bpo), colors, gray_level,
                               easing_pow, rgb);                                    // update.rs:985-992
            uint8_t* px = out_rgba + 4 * static_cast<size_t>(bin);
            for (int i = 0; i < 3; ++i) px[i] = texel_u8(static_cast<float>(rgb[i]) / 255.0f);   // update.rs:998-1000
            px[3] = texel_u8(brightness);                                           // update.rs:1001
        }
        return;
    }
    // SpectrogramMode::Peaks, update.rs:1005-1065
    std::memset(out_rgba, 0, 4 * static_cast<size_t>(n_buckets));                   // (the line was cleared a frame ago, update.rs:1068-1078)
    float max_size = 0.0f;
    for (uint32_t p = 0; p < n_peaks; ++p) max_size = std::fmax(max_size, size[p]); // update.rs:1010-1014
    if (!(max_size > 0.0f)) return;                                                 // update.rs:1016
    const float width = static_cast<float>(n_buckets);
    for (uint32_t p = 0; p < n_peaks; ++p) {
        const float c = center[p];
        const float brightness = brightness_of(1.0f - size[p] / max_size);          // update.rs:1022-1023
        uint8_t rgb[3];
        calculate_color_u8(buckets_per_octave, std::fmod(c + semitone_offset, bpo), colors, gray_level, easing_pow, rgb);   // update.rs:1029-1035
        // update.rs:1038-1039; `as usize` saturates and maps NaN to 0, f32::max / min ignore a NaN
        const float lo_f = std::fmax(std::floor(c - 2.0f), 0.0f), hi_f = std::fmin(std::ceil(c + 2.0f), width);
        const uint32_t lo = lo_f >= width ? n_buckets : static_cast<uint32_t>(lo_f);
        const uint32_t hi = hi_f > 0.0f ? static_cast<uint32_t>(hi_f) : 0u;
        for (uint32_t bin = lo; bin < hi; ++bin) {                                  // update.rs:1041-1062
            const float distance = std::fabs(static_cast<float>(bin) - c);
            if (distance <= 2.0f) {
                const float falloff = std::exp(-distance * distance / (2.0f * 2.0f * 0.5f));
                uint8_t* px = out_rgba + 4 * static_cast<size_t>(bin);
                for (int i = 0; i < 3; ++i) px[i] = texel_u8(static_cast<float>(rgb[i]) / 255.0f);
                px[3] = texel_u8(brightness * falloff);
            }
        }
    }
}

int chroma_bin_0_pitch_class(float min_freq) {   // update.rs:1108-1110
    const float semitones_from_c4 = 12.0f * std::log2(min_freq / 261.626f);
    const float r = std::round(semitones_from_c4);
    const int ri = !(r == r) ? 0 : (r >= 2147483648.0f ? 2147483647 : (r <= -2147483648.0f ? -2147483647 - 1 : static_cast<int>(r)));   // `as i32`
    return ((ri % 12) + 12) % 12;
}

uint32_t chroma_pitch_class(uint32_t bin, uint16_t buckets_per_octave, int bin_0_pitch_class) {   // update.rs:1115-1118
    const float semitone = std::round(static_cast<float>(bin * 12u) / static_cast<float>(buckets_per_octave));
    return static_cast<uint32_t>((static_cast<int>(semitone) + bin_0_pitch_class) % 12);
}

void chroma_row(float min_freq, uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, float out12[12]) {
    const int bin_0 = chroma_bin_0_pitch_class(min_freq);
    float chroma[12] = {0.0f};                                                      // update.rs:1103
    for (uint32_t bin = 0; bin < n_buckets; ++bin) {                                // update.rs:1112-1123
        const float power = std::pow(10.0f, x_vqt_smoothed[bin] / 10.0f);
        chroma[chroma_pitch_class(bin, buckets_per_octave, bin_0)] += power;
    }
    float max_chroma = 0.0f;
    for (int k = 0; k < 12; ++k) max_chroma = std::fmax(max_chroma, chroma[k]);     // update.rs:1126
    for (int k = 0; k < 12; ++k) out12[k] = max_chroma > 0.0f ? chroma[k] / max_chroma : chroma[k];   // update.rs:1127-1131
}

}  // namespace pvq
