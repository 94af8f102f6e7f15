// scene_math.hpp — the one copy of the pitch-ball scene's per-frame arithmetic, for the host object (scene_host.cpp, g++) and the
// device stage (scene_batch.hip): pitchvis_viewer/src/display_system/update.rs:136-426 with setup.rs:89-172 and util.rs:9-20.
//
// Every expression is the reference's f32 expression, operation for operation, FMA contraction off on both sides.  The libm calls
// of a frame (powf of the spiral radius, of the saturation easing and of the two sRGB curves; sin_cos of the spiral angle, cosf /
// sinf of the hue) go through SceneMath: the double-precision function, rounded once to f32.  That is the correctly rounded f32
// result but for arguments within ~1e-9 ulp of a rounding boundary, on the host's libm and on the device's alike, so a colour —
// which passes through a rounding to u8 (lib.rs:108) where one ulp can become 1 / 255 — carries the same bits on both sides.
#pragma once

#include "color_math.hpp"

#define PVQ_HD_FLAT PVQ_HD __attribute__((always_inline))   // a caller's small arrays stay in registers

namespace pvq {
namespace scene {

struct SceneMath {
    static PVQ_HD float pow(float x, float y) { return static_cast<float>(::pow(static_cast<double>(x), static_cast<double>(y))); }
    static PVQ_HD float cos(float x) { return static_cast<float>(::cos(static_cast<double>(x))); }
    static PVQ_HD float sin(float x) { return static_cast<float>(::sin(static_cast<double>(x))); }
};

constexpr float BALL_SCALE_FACTOR = 1.0f / 305.0f;   // update.rs:23 PITCH_BALL_SCALE_FACTOR
constexpr float VISIBILITY_CUTOFF = 0.019f;          // update.rs:147
constexpr uint32_t SEGMENTS_PER_SEMITONE = 6;        // update.rs:22
constexpr float PI_F = 3.14159274101257324219f;      // std::f32::consts::PI

enum Mode { FULL = 0, ZEN = 1, PERFORMANCE = 2, GALAXY = 3 };

// fixed at create
struct Settings {
    uint32_t n_bins, bpo, n_segments;
    int mode, enable_bloom;
    float gray_level, easing_pow;
    float semitone_offset;   // (bpo - 3 (bpo / 12)) as f32, update.rs:221
    float hide_radius;       // (bpo / 12) as f32 * 0.23, update.rs:310
    float lch[12][3];        // lib.rs:98 of every palette entry
};

// Rust `as usize` of an f32 that has been through round / trunc: saturating, NaN -> 0 (u32 range is enough: anything >= n_bins is out)
PVQ_HD uint32_t sat_u32(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967040.0f) return 4294967040u;
    return static_cast<uint32_t>(v);
}

// bevy_color: LinearRgba::from(Srgba), one channel (alpha is not converted)
PVQ_HD_FLAT float srgb_to_linear(float x) {
    PVQ_FP_STRICT
    if (x <= 0.04045f) return x / 12.92f;
    return SceneMath::pow((x + 0.055f) / 1.055f, 2.4f);
}

// util.rs:9-20 bin_to_spiral
PVQ_HD_FLAT void bin_to_spiral(uint32_t bpo, float x, float& out_x, float& out_y) {
    PVQ_FP_STRICT
    const float bpo_f = static_cast<float>(bpo);
    const float radius = 2.0f * (0.3f + SceneMath::pow(x / bpo_f, 0.75f));   // util.rs:12
    const float angle = (x + bpo_f) / bpo_f * 2.0f * PI_F;                   // util.rs:14-17 (0 * (bpo / 12) erased)
    out_x = -1.0f * SceneMath::cos(angle) * radius;                          // util.rs:19
    out_y = SceneMath::sin(angle) * radius;
}

// pitchvis_colors::calculate_color (lib.rs:86-117) from the palette's (L, C, h): r, g, b in 0..1 (u8 / 255)
PVQ_HD_FLAT void color_at(const Settings& s, float bucket, float rgb[3]) {
    PVQ_FP_STRICT
    uint32_t tone;
    float inaccuracy;
    color::tone_of_bucket(s.bpo, bucket, tone, inaccuracy);
    uint8_t u8[3];
    color::lch_color_u8<SceneMath>(s.lch[tone][0], s.lch[tone][1], s.lch[tone][2], inaccuracy, s.gray_level, s.easing_pow, u8);
    rgb[0] = static_cast<float>(u8[0]) / 255.0f;   // lib.rs:110-114
    rgb[1] = static_cast<float>(u8[1]) / 255.0f;
    rgb[2] = static_cast<float>(u8[2]) / 255.0f;
}

// util::arg_max (util.rs:48-57) folds from f32::MIN with `>`: the value of the first maximum; sizes[0] when nothing exceeds f32::MIN
constexpr float F32_MIN = -3.40282347e+38f;

// What one entry of peaks_continuous makes of the ball it is keyed to: update.rs:217-302, nothing of it depends on the scene's state.
struct PeakRecord {
    float x, y, z, scale;       // translation (update.rs:231-234) and the splat scale (update.rs:298-299)
    float r, g, b, a;           // LinearRgba (update.rs:245) after the clamp of update.rs:276-284
    float calmness, accuracy, deviation;   // update.rs:262-265
    uint32_t key;               // trunc(center) as usize (update.rs:211); >= n_bins: the entry is ignored
    uint32_t lo, hi;            // the hide range lo ..= hi (update.rs:312-315)
    uint32_t shows;             // scale >= 0.002 (update.rs:300)
    uint32_t pad;
};

// The MIDI pitch of a bin as the `ml` branch names it (update.rs:248, util.rs:23-31 bin_to_midi_pitch): round(bin / bpo * 12) + 33,
// the division and the product each rounded to f32, roundf half away from zero; 33 is FREQ_A1_MIDI_KEY_ID.  A pitch above 127 is
// the reference's None.
constexpr uint32_t FREQ_A1_MIDI_KEY_ID = 33;
constexpr uint32_t MIDI_PITCHES = 128;
constexpr float ML_THRESHOLD = 0.35f;   // update.rs:250
PVQ_HD uint32_t midi_pitch(uint32_t bpo, uint32_t bin) {
    PVQ_FP_STRICT
    const float q = static_cast<float>(bin) / static_cast<float>(bpo);
    return sat_u32(roundf(q * 12.0f)) + FREQ_A1_MIDI_KEY_ID;   // (sat_u32 stops at 4294967040: the sum does not wrap)
}

// calm / acc / dev: the frame's per-bin fields (only entry `key` is read).  ml_prob: the frame's ml_midi_base_pitches [128], or
// null: no `ml` branch.
PVQ_HD_FLAT void peak_record(const Settings& s, float center, float size, float max_size, const float* calm, const float* acc, const float* dev,
                        PeakRecord& o, const float* ml_prob = nullptr) {
    PVQ_FP_STRICT
    const uint32_t n = s.n_bins;
    o.key = sat_u32(truncf(center));
    o.pad = 0u;
    const bool ignored = o.key >= n;   // the reference would index out of range; the record is never applied
    const uint32_t at = ignored ? 0u : o.key;
    float rgb[3];
    color_at(s, fmodf(center + s.semitone_offset, static_cast<float>(s.bpo)), rgb);   // update.rs:219-226
    const float t = 1.0f - size / max_size;
    const float color_coefficient = 1.0f - (t * t);                                    // update.rs:229 (powf(2.0) is t * t rounded once)
    bin_to_spiral(s.bpo, center, o.x, o.y);                                            // update.rs:231
    o.z = (size / max_size - 1.01f) * 12.5f;                                           // update.rs:233
    o.r = color::clampf(srgb_to_linear(rgb[0]), 0.0f, 1.0f);                           // update.rs:245, :276-284
    o.g = color::clampf(srgb_to_linear(rgb[1]), 0.0f, 1.0f);
    o.b = color::clampf(srgb_to_linear(rgb[2]), 0.0f, 1.0f);
    o.a = color_coefficient;
    if (ml_prob && !ignored) {   // update.rs:247-255: an inferred pitch is opaque, any other nearly transparent
        const uint32_t m = midi_pitch(s.bpo, o.key);
        if (m < MIDI_PITCHES) o.a = ml_prob[m] > ML_THRESHOLD ? 1.0f : color_coefficient * 0.1f;   // (a NaN takes the dim side)
    }
    o.calmness = color::clampf(calm[at] - 0.27f, 0.0f, 1.0f);                       // update.rs:262-263
    o.accuracy = acc[at];
    o.deviation = dev[at];
    const float calmness_scale = 1.0f + 0.2f * o.calmness;                             // update.rs:273
    const float ball_scale_factor = s.mode == PERFORMANCE ? 0.7f : 1.0f;               // update.rs:291-295
    o.scale = size * ball_scale_factor * BALL_SCALE_FACTOR * calmness_scale;           // update.rs:298-299
    o.shows = !ignored && o.scale >= 0.002f ? 1u : 0u;                                             // update.rs:300
    // update.rs:312-315; f32::max / min ignore a NaN
    o.lo = ignored ? 1u : sat_u32(fmaxf(roundf(center - s.hide_radius), 0.0f));
    o.hi = ignored ? 0u : sat_u32(fminf(roundf(center + s.hide_radius), static_cast<float>(n - 1u)));
}

// fade_pitch_balls for one ball (update.rs:151-177); dropoff and z_step come from the host's table
PVQ_HD void fade_ball(float& scale, float& alpha, float& z, bool& visible, float dropoff, float z_step) {
    PVQ_FP_STRICT
    float size = scale / BALL_SCALE_FACTOR;                  // update.rs:151
    if (size * BALL_SCALE_FACTOR >= VISIBILITY_CUTOFF) {     // update.rs:153
        visible = true;
        size = size * dropoff;                               // update.rs:161
        scale = size * BALL_SCALE_FACTOR;                    // update.rs:162
        alpha = fmaxf(alpha * dropoff, 0.7f);                // update.rs:166-168
        z = z - z_step;                                      // update.rs:172
    }
    if (size * BALL_SCALE_FACTOR < VISIBILITY_CUTOFF) visible = false;   // update.rs:175-177
}

// update_bloom (update.rs:336-351)
PVQ_HD float bloom_of(const Settings& s, float scene_calmness) {
    PVQ_FP_STRICT
    if (!s.enable_bloom || s.mode == PERFORMANCE) return 0.0f;
    return color::clampf(scene_calmness * 1.3f, 0.0f, 1.0f);
}

// update_bass_spiral (update.rs:369-425) from the FIRST peak: the number of lit segments, and their one colour when any is lit
PVQ_HD_FLAT uint32_t bass_of(const Settings& s, float center, float size, float max_size, float rgba[4]) {
    PVQ_FP_STRICT
    if (s.mode == GALAXY) return 0u;                                                    // update.rs:374-376
    const float c = center / static_cast<float>(s.bpo) * 12.0f;                         // update.rs:381
    const float rc = roundf(c);
    if (static_cast<uint64_t>(sat_u32(rc)) * SEGMENTS_PER_SEMITONE >= s.n_segments) return 0u;   // update.rs:382-387
    const uint32_t lit = sat_u32(rc * static_cast<float>(SEGMENTS_PER_SEMITONE));       // update.rs:390
    if (lit == 0u) return 0u;
    const float color_map_ref = rc * static_cast<float>(s.bpo) / 12.0f;                 // update.rs:398
    color_at(s, fmodf(color_map_ref + s.semitone_offset, static_cast<float>(s.bpo)), rgba);   // update.rs:399-406
    const float t = 1.0f - size / max_size;
    rgba[3] = 1.0f - (t * t);                                                           // update.rs:416
    return lit;
}

}  // namespace scene
}  // namespace pvq
