// color_math.hpp — the one copy of the colour arithmetic, for the host unit (consumers_host.cpp, g++) and the render kernels
// (render_batch.hip, device code): pitchvis_colors/src/lib.rs:86-117 with the conversions of the `lab` crate (0.11.0,
// Cargo.lock:3985) restated: sRGB (u8) <-> CIE XYZ (D65) <-> L*a*b* <-> LCh.  Not vendored in the reference tree; parity with the
// crate's exact constants is unpinned.
//
// Every expression is the reference's f32 expression, operation for operation, with FMA contraction off on both sides (the host
// unit is built with -ffp-contract=off, device code takes the pragma below); what differs between host and device is libm alone
// (powf, cosf, sinf, expf).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PVQ_HD __host__ __device__ inline
#else
#define PVQ_HD inline
#endif
#if defined(__clang__)
#define PVQ_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define PVQ_FP_STRICT
#endif

namespace pvq {
namespace color {

constexpr float KAPPA = 24389.0f / 27.0f;
constexpr float EPSILON = 216.0f / 24389.0f;
constexpr float CBRT_EPSILON = 6.0f / 29.0f;
constexpr float S_0 = 0.003130668442500564f;
constexpr float E_0_255 = 3294.6f * S_0;
constexpr float WHITE_X = 0.9504492182750991f;
constexpr float WHITE_Z = 1.0889166484304715f;

// Which powf / cosf / sinf the conversions below call: the build's libm by default.  A caller that needs host and device to agree
// beyond libm (scene_math.hpp) passes its own.
struct LibmF32 {
    static PVQ_HD float pow(float x, float y) { return powf(x, y); }
    static PVQ_HD float cos(float x) { return cosf(x); }
    static PVQ_HD float sin(float x) { return sinf(x); }
};

PVQ_HD float srgb_expand(float c) {   // c in 0..255
    PVQ_FP_STRICT
    if (c > E_0_255) return powf((c + 0.055f * 255.0f) / (1.055f * 255.0f), 2.4f);
    return c / (12.92f * 255.0f);
}
template <class M = LibmF32>
PVQ_HD float srgb_compress(float c) {
    PVQ_FP_STRICT
    const float v = (c > S_0) ? 1.055f * M::pow(c, 1.0f / 2.4f) - 0.055f : 12.92f * c;
    return fmaxf(fminf(v, 1.0f), 0.0f);
}
PVQ_HD float lab_map(float c) {
    PVQ_FP_STRICT
    return (c > EPSILON) ? powf(c, 1.0f / 3.0f) : (KAPPA * c + 16.0f) / 116.0f;
}

PVQ_HD void rgb_to_lch(const uint8_t rgb[3], float& l, float& c, float& h) {
    PVQ_FP_STRICT
    const float r = srgb_expand(static_cast<float>(rgb[0])), g = srgb_expand(static_cast<float>(rgb[1])),
                b = srgb_expand(static_cast<float>(rgb[2]));
    const float x = r * 0.4124108464885388f + g * 0.3575845678529519f + b * 0.18045380393360833f;
    const float y = r * 0.21264934272065283f + g * 0.7151691357059038f + b * 0.07218152157344333f;
    const float z = r * 0.019331758429150258f + g * 0.11919485595098397f + b * 0.9503900340503373f;
    const float fx = lab_map(x / WHITE_X), fy = lab_map(y), fz = lab_map(z / WHITE_Z);
    l = (116.0f * fy) - 16.0f;
    const float a = 500.0f * (fx - fy), bb = 200.0f * (fy - fz);
    c = hypotf(a, bb);
    h = atan2f(bb, a);
}
template <class M = LibmF32>
PVQ_HD void lch_to_rgb(float l, float c, float h, uint8_t rgb[3]) {
    PVQ_FP_STRICT
    const float a = c * M::cos(h), bb = c * M::sin(h);
    const float fy = (l + 16.0f) / 116.0f;
    const float fx = (a / 500.0f) + fy;
    const float fz = fy - (bb / 200.0f);
    const float xr = (fx > CBRT_EPSILON) ? fx * fx * fx : ((fx * 116.0f) - 16.0f) / KAPPA;
    const float yr = (l > EPSILON * KAPPA) ? fy * fy * fy : l / KAPPA;
    const float zr = (fz > CBRT_EPSILON) ? fz * fz * fz : ((fz * 116.0f) - 16.0f) / KAPPA;
    const float x = xr * WHITE_X, y = yr, z = zr * WHITE_Z;
    const float r = x * 3.240812398895283f - y * 1.5373084456298136f - z * 0.4985865229069666f;
    const float g = x * -0.9692430170086407f + y * 1.8759663029085742f + z * 0.04155503085668564f;
    const float b = x * 0.055638398436112804f - y * 0.20400746093241362f + z * 1.0571295702861434f;
    rgb[0] = static_cast<uint8_t>(roundf(srgb_compress<M>(r) * 255.0f));
    rgb[1] = static_cast<uint8_t>(roundf(srgb_compress<M>(g) * 255.0f));
    rgb[2] = static_cast<uint8_t>(roundf(srgb_compress<M>(b) * 255.0f));
}
PVQ_HD uint8_t sat_u8(float v) {   // Rust `as u8`: saturating, NaN -> 0, truncation toward zero
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return static_cast<uint8_t>(v);
}
PVQ_HD float clampf(float v, float lo, float hi) {   // f32::clamp: a NaN passes through
    return v < lo ? lo : (v > hi ? hi : v);
}

// lib.rs:93-96: which palette entry a continuous bucket takes and how far off the tone it sits
PVQ_HD void tone_of_bucket(uint32_t buckets_per_octave, float bucket, uint32_t& tone, float& inaccuracy_cents) {
    PVQ_FP_STRICT
    const float pitch_continuous = 12.0f * bucket / static_cast<float>(buckets_per_octave);   // lib.rs:93
    const float rounded = roundf(pitch_continuous);
    // `as usize` saturates at 0 (and at the top: a float past 2^32 stays a defined conversion)
    tone = static_cast<uint32_t>(rounded < 0.0f ? 0.0f : fminf(rounded, 4294967040.0f)) % 12u;
    inaccuracy_cents = fabsf(pitch_continuous - rounded);                                      // lib.rs:96
}
// lib.rs:98-108 from the tone's (L, C, h) (lib.rs:98: rgb_to_lch of the palette entry as u8)
template <class M = LibmF32>
PVQ_HD void lch_color_u8(float l, float c, float h, float inaccuracy_cents, float gray_level, float easing_pow, uint8_t rgb[3]) {
    PVQ_FP_STRICT
    const float saturation = 1.0f - M::pow(2.0f * inaccuracy_cents, easing_pow);   // lib.rs:104
    c *= saturation;                                                              // lib.rs:105
    l = saturation * l + (1.0f - saturation) * gray_level;                        // lib.rs:106
    lch_to_rgb<M>(l, c, h, rgb);                                                  // lib.rs:108
}

// update.rs:998-1001 / :1053-1059: `(x * 255.0 * 1.2).clamp(0.0, 255.0) as u8`
PVQ_HD uint8_t texel_u8(float x) {
    PVQ_FP_STRICT
    return sat_u8(clampf((x * 255.0f) * 1.2f, 0.0f, 255.0f));
}
// update.rs:976 / :1023: `((1.0 - t.powf(2.0)) * 1.5).clamp(0.0, 1.0)`; powf(t, 2) is t * t correctly rounded
PVQ_HD float brightness_of(float t) {
    PVQ_FP_STRICT
    return clampf((1.0f - (t * t)) * 1.5f, 0.0f, 1.0f);
}

}  // namespace color
}  // namespace pvq
