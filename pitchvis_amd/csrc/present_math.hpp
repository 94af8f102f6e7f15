// present_math.hpp — the one copy of the present stage's arithmetic, for the host face (present_host.cpp, g++) and the device
// stage (present_batch.hip): bloom over a mip pyramid, the display transform and the sRGB encode that turn the linear HDR target
// [H][W][4] of the picture chain into bytes.  Bevy's bloom and tone-mapping shaders are not in the reference tree, so the rule is
// the one include/pvq.h states ("the present stage"), restated from Bevy's published behaviour; the assumed semantics are
// DESIGN.md 6h's table.  The reference pins the parameters (setup.rs:347-383) and the intensity (update.rs:346-347) only.
//
// All of it is f32, FMA contraction off on both sides, `/` the correctly rounded division, every sum in the order written.  The
// first pass's powf(g, 1 / 2.2) is taken in double arithmetic without libm and rounded once to f32 (present_root22): the correctly
// rounded f32 result but for arguments within 1e-7 ulp of a tie, with the same bits on host and device.  A difference of an ulp
// there would reach the bloomed picture multiplied by the sum of the blend factors (46 at the reference's settings and intensity
// 1), so the linear picture carries the same bits on both sides.  The blend factors' powf is
// taken on the host for both (Factors).  What differs between host and device is libm in the bytes alone: expf of the display
// transform and powf of the encode.
//
// A texture is read through a functor `tex(x, y, rgb)` with 0 <= x < w, 0 <= y < h, so the same code samples host arrays, device
// memory and a tile's footprint staged in LDS.
#pragma once

#include "raster_math.hpp"

#if defined(__clang__)
#define PVQ_UNROLL _Pragma("unroll")
#else
#define PVQ_UNROLL
#endif

namespace pvq {
namespace present {

constexpr uint32_t DEFAULT_MIP_DIMENSION = 512, MIN_MIP_DIMENSION = 4, MAX_MIP_DIMENSION = 4096;
constexpr uint32_t MAX_MIPS = 11;             // max(floor(log2 4096), 2) - 1
constexpr uint32_t MAX_MIP_SIDE = 16384;      // a mip 0 wider than this (a picture far wider than high) is refused
constexpr int ENERGY_CONSERVING = 0, ADDITIVE = 1;
constexpr int TONEMAP_NONE = 0, TONEMAP_SOMEWHAT_BORING = 1;
constexpr float TENT = 0.004f;                // the upsample tent's uv radius along y

struct Settings {   // pvq_present_settings with max_mip_dimension resolved
    float low_frequency_boost, low_frequency_boost_curvature, high_pass_frequency, threshold, threshold_softness;
    int composite_mode;
    uint32_t max_mip_dimension;
    int tonemapping;
};
// the reference camera's (setup.rs:347-383)
PVQ_HD Settings default_settings() { return Settings{1.0f, 1.0f, 0.52f, 0.17f, 0.82f, ADDITIVE, DEFAULT_MIP_DIMENSION, TONEMAP_SOMEWHAT_BORING}; }

// x^(1 / 2.2) for x >= 0 (never a NaN: the caller's fmaxf has seen to that), in double arithmetic and without libm, so that host
// and device carry the same bits: x = 2^e m with m in (sqrt(1/2), sqrt(2)], log2 m = 2 / ln 2 * atanh((m - 1) / (m + 1)) by its series
// to s^19 (|s| <= 0.1716: the first term left out is 2e-17 of the sum), y = (e + log2 m) * (1 / 2.2 as f32), 2^y = 2^n e^f with n = floor(y
// + 0.5) and e^f by its series to f^12 (|f| <= 0.3466: 2e-16), scaled through the exponent bits (n is -68 .. 59).  The double is within
// 1e-15 of the true power and is rounded once to f32: the correctly rounded f32 result but for arguments within 1e-7 ulp of a tie.
PVQ_HD float present_root22(float x) {
    PVQ_FP_STRICT
    if (!(x > 0.0f)) return 0.0f;
    if (x > 3.40282347e38f) return x;   // +inf
    const double d = static_cast<double>(x);   // a subnormal f32 is a normal double
    uint64_t bits;
    __builtin_memcpy(&bits, &d, 8);
    int e = static_cast<int>(bits >> 52) - 1023;
    bits = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    double m;
    __builtin_memcpy(&m, &bits, 8);   // [1, 2)
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e += 1;
    }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double p = 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0;
    p = p * s2 + 1.0 / 15.0;
    p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0;
    p = p * s2 + 1.0 / 9.0;
    p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;
    p = p * s2 + 1.0 / 3.0;
    p = p * s2 + 1.0;
    const double log2m = s * p * 2.8853900817779268;   // 2 / ln 2
    const double y = (static_cast<double>(e) + log2m) * static_cast<double>(1.0f / 2.2f);
    const double n = floor(y + 0.5);
    const double f = (y - n) * 0.6931471805599453;     // ln 2
    double q = 1.0 / 479001600.0;
    q = q * f + 1.0 / 39916800.0;
    q = q * f + 1.0 / 3628800.0;
    q = q * f + 1.0 / 362880.0;
    q = q * f + 1.0 / 40320.0;
    q = q * f + 1.0 / 5040.0;
    q = q * f + 1.0 / 720.0;
    q = q * f + 1.0 / 120.0;
    q = q * f + 1.0 / 24.0;
    q = q * f + 1.0 / 6.0;
    q = q * f + 0.5;
    q = q * f + 1.0;
    q = q * f + 1.0;
    uint64_t scale_bits = static_cast<uint64_t>(static_cast<int64_t>(n) + 1023) << 52;
    double scale;
    __builtin_memcpy(&scale, &scale_bits, 8);
    return static_cast<float>(q * scale);
}

struct Libm {
    static PVQ_HD float root22(float x) { return present_root22(x); }
    static PVQ_HD float pow(float x, float y) { return powf(x, y); }
    static PVQ_HD float exp(float x) { return expf(x); }
};

// ---- the mip chain ----
struct Mips {
    uint32_t n;
    uint32_t w[MAX_MIPS], h[MAX_MIPS];
};
// d: 4 .. 4096.  false where mip 0 would be wider than MAX_MIP_SIDE.
inline bool mip_chain(uint32_t W, uint32_t H, uint32_t d, Mips& m) {
    PVQ_FP_STRICT
    uint32_t log2d = 0;
    while ((d >> (log2d + 1u)) != 0u) ++log2d;
    m.n = (log2d > 2u ? log2d : 2u) - 1u;
    const float ratio = static_cast<float>(d) / static_cast<float>(H);
    const float fw = roundf(static_cast<float>(W) * ratio), fh = roundf(static_cast<float>(H) * ratio);
    if (!(fw <= static_cast<float>(MAX_MIP_SIDE) && fh <= static_cast<float>(MAX_MIP_SIDE))) return false;
    const uint32_t w0 = fw < 1.0f ? 1u : static_cast<uint32_t>(fw), h0 = fh < 1.0f ? 1u : static_cast<uint32_t>(fh);
    for (uint32_t k = 0; k < MAX_MIPS; ++k) {
        m.w[k] = k < m.n && (w0 >> k) > 1u ? w0 >> k : 1u;
        m.h[k] = k < m.n && (h0 >> k) > 1u ? h0 >> k : 1u;
    }
    return true;
}

// ---- the blend factors ----
// B_k = (intensity + lf[k] * (energy-conserving ? 1 - intensity : 1)) * hp[k]; lf and hp do not depend on the intensity
struct Factors {
    float lf[MAX_MIPS], hp[MAX_MIPS];
};
inline void blend_tables(const Settings& s, uint32_t n_mips, Factors& f) {
    PVQ_FP_STRICT
    for (uint32_t k = 0; k < MAX_MIPS; ++k) {
        const float r = n_mips > 1u ? static_cast<float>(k) / static_cast<float>(n_mips - 1u) : 0.0f;
        f.lf[k] = (1.0f - powf(1.0f - r, 1.0f / (1.0f - s.low_frequency_boost_curvature))) * s.low_frequency_boost;
        f.hp[k] = 1.0f - raster::w_clamp((r - s.high_pass_frequency) / s.high_pass_frequency, 0.0f, 1.0f);
    }
}
PVQ_HD float blend_factor(const Factors& f, uint32_t k, int composite_mode, float intensity) {
    PVQ_FP_STRICT
    float lf = f.lf[k];
    if (composite_mode == ENERGY_CONSERVING) lf *= 1.0f - intensity;
    return (intensity + lf) * f.hp[k];
}
// a row whose intensity is not finite or is <= 0 skips bloom
PVQ_HD bool blooms(float intensity) { return intensity > 0.0f && raster::finite_f(intensity); }

// ---- sampling ----
PVQ_HD uint32_t clamp_index(float f, uint32_t size) {   // f = floor of a coordinate within a few texels of the texture
    const int i = static_cast<int>(f);
    return i < 0 ? 0u : (static_cast<uint32_t>(i) >= size ? size - 1u : static_cast<uint32_t>(i));
}
template <class Tex>
PVQ_HD_FLAT void sample(const Tex& tex, uint32_t w, uint32_t h, float u, float v, float out[3]) {
    PVQ_FP_STRICT
    const float px = u * static_cast<float>(w) - 0.5f, py = v * static_cast<float>(h) - 0.5f;
    const float x0f = floorf(px), y0f = floorf(py);
    const float fx = px - x0f, fy = py - y0f;
    const uint32_t x0 = clamp_index(x0f, w), x1 = clamp_index(x0f + 1.0f, w), y0 = clamp_index(y0f, h), y1 = clamp_index(y0f + 1.0f, h);
    float a[3], b[3], c[3], d[3];
    tex(x0, y0, a);
    tex(x1, y0, b);
    tex(x0, y1, c);
    tex(x1, y1, d);
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        const float top = a[ch] + (b[ch] - a[ch]) * fx, bottom = c[ch] + (d[ch] - c[ch]) * fx;
        out[ch] = top + (bottom - top) * fy;
    }
}
PVQ_HD float pixel_uv(uint32_t i, uint32_t size) {
    PVQ_FP_STRICT
    return (static_cast<float>(i) + 0.5f) / static_cast<float>(size);
}

PVQ_HD float luma(const float v[3]) {
    PVQ_FP_STRICT
    return 0.2126f * v[0] + 0.7152f * v[1] + 0.0722f * v[2];
}

// ---- downsample: 13 taps a .. m around (u, v), offsets in source texels ----
// The taps are taken in the order a .. m and added to the sums they belong to as they come, which is the order the rule writes
// every sum in; no more than one tap and the sums are alive at a time.
template <class Tex>
PVQ_HD_FLAT void tap(const Tex& tex, uint32_t ws, uint32_t hs, float u, float v, float ox, float oy, float out[3]) {
    PVQ_FP_STRICT
    sample(tex, ws, hs, u + ox / static_cast<float>(ws), v + oy / static_cast<float>(hs), out);
}
PVQ_HD void set3(float acc[3], const float t[3]) {
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) acc[ch] = t[ch];
}
PVQ_HD void add3(float acc[3], const float t[3]) {
    PVQ_FP_STRICT
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + t[ch];
}
// mip k -> k + 1: (a + c + g + i) * 0.03125 + (b + d + f + h) * 0.0625 + (e + j + k + l + m) * 0.125
template <class Tex>
PVQ_HD_FLAT void down_plain(const Tex& tex, uint32_t ws, uint32_t hs, float u, float v, float out[3]) {
    PVQ_FP_STRICT
    float t[3], corners[3], edges[3], inner[3];
    tap(tex, ws, hs, u, v, -2.0f, 2.0f, t), set3(corners, t);    // a
    tap(tex, ws, hs, u, v, 0.0f, 2.0f, t), set3(edges, t);       // b
    tap(tex, ws, hs, u, v, 2.0f, 2.0f, t), add3(corners, t);     // c
    tap(tex, ws, hs, u, v, -2.0f, 0.0f, t), add3(edges, t);      // d
    tap(tex, ws, hs, u, v, 0.0f, 0.0f, t), set3(inner, t);       // e
    tap(tex, ws, hs, u, v, 2.0f, 0.0f, t), add3(edges, t);       // f
    tap(tex, ws, hs, u, v, -2.0f, -2.0f, t), add3(corners, t);   // g
    tap(tex, ws, hs, u, v, 0.0f, -2.0f, t), add3(edges, t);      // h
    tap(tex, ws, hs, u, v, 2.0f, -2.0f, t), add3(corners, t);    // i
    tap(tex, ws, hs, u, v, -1.0f, 1.0f, t), add3(inner, t);      // j
    tap(tex, ws, hs, u, v, 1.0f, 1.0f, t), add3(inner, t);       // k
    tap(tex, ws, hs, u, v, -1.0f, -1.0f, t), add3(inner, t);     // l
    tap(tex, ws, hs, u, v, 1.0f, -1.0f, t), add3(inner, t);      // m
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) out[ch] = corners[ch] * 0.03125f + edges[ch] * 0.0625f + inner[ch] * 0.125f;
}
// picture -> mip 0: the groups (a + b + d + e), (b + c + e + f), (d + e + g + h), (e + f + h + i) at 0.03125 and (j + k + l + m) at
// 0.125, each weighted by its luma, summed in order; the clamp; the soft threshold
template <class Tex, class Lm = Libm>
PVQ_HD_FLAT void down_first(const Tex& tex, uint32_t ws, uint32_t hs, float u, float v, float threshold, float softness, float out[3]) {
    PVQ_FP_STRICT
    float t[3], g[5][3];
    tap(tex, ws, hs, u, v, -2.0f, 2.0f, t), set3(g[0], t);                                             // a
    tap(tex, ws, hs, u, v, 0.0f, 2.0f, t), add3(g[0], t), set3(g[1], t);                               // b
    tap(tex, ws, hs, u, v, 2.0f, 2.0f, t), add3(g[1], t);                                              // c
    tap(tex, ws, hs, u, v, -2.0f, 0.0f, t), add3(g[0], t), set3(g[2], t);                              // d
    tap(tex, ws, hs, u, v, 0.0f, 0.0f, t), add3(g[0], t), add3(g[1], t), add3(g[2], t), set3(g[3], t);   // e
    tap(tex, ws, hs, u, v, 2.0f, 0.0f, t), add3(g[1], t), add3(g[3], t);                               // f
    tap(tex, ws, hs, u, v, -2.0f, -2.0f, t), add3(g[2], t);                                            // g
    tap(tex, ws, hs, u, v, 0.0f, -2.0f, t), add3(g[2], t), add3(g[3], t);                              // h
    tap(tex, ws, hs, u, v, 2.0f, -2.0f, t), add3(g[3], t);                                             // i
    tap(tex, ws, hs, u, v, -1.0f, 1.0f, t), set3(g[4], t);                                             // j
    tap(tex, ws, hs, u, v, 1.0f, 1.0f, t), add3(g[4], t);                                              // k
    tap(tex, ws, hs, u, v, -1.0f, -1.0f, t), add3(g[4], t);                                            // l
    tap(tex, ws, hs, u, v, 1.0f, -1.0f, t), add3(g[4], t);                                             // m
    float sum[3] = {0.0f, 0.0f, 0.0f};
    PVQ_UNROLL
    for (int k = 0; k < 5; ++k) {
        float c[3], p[3];
        PVQ_UNROLL
        for (int ch = 0; ch < 3; ++ch) {
            c[ch] = g[k][ch] * (k < 4 ? 0.03125f : 0.125f);
            p[ch] = Lm::root22(fmaxf(c[ch], 0.0f));
        }
        const float weight = 1.0f / (1.0f + luma(p) / 4.0f);
        PVQ_UNROLL
        for (int ch = 0; ch < 3; ++ch) sum[ch] = k == 0 ? c[ch] * weight : sum[ch] + c[ch] * weight;
    }
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) out[ch] = fminf(fmaxf(sum[ch], 1e-4f), 3.40282347e37f);   // a NaN becomes 1e-4
    if (threshold == 0.0f) return;
    const float knee = threshold * softness;
    const float br = fmaxf(fmaxf(out[0], out[1]), out[2]);
    float s = raster::w_clamp(br - (threshold - knee), 0.0f, 2.0f * knee);
    s = s * s * (0.25f / (knee + 1e-5f));
    const float contribution = fmaxf(br - threshold, s) / fmaxf(br, 1e-5f);
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) out[ch] *= contribution;
}

// ---- upsample: the 3 x 3 tent of a mip around (u, v); x = TENT / (W / H) of the picture, y = TENT ----
PVQ_HD float tent_x(uint32_t W, uint32_t H) {
    PVQ_FP_STRICT
    return TENT / (static_cast<float>(W) / static_cast<float>(H));
}
template <class Tex>
PVQ_HD_FLAT void tent(const Tex& tex, uint32_t w, uint32_t h, float u, float v, float x, float y, float out[3]) {
    PVQ_FP_STRICT
    enum { TA, TB, TC, TD, TE, TF, TG, TH, TI };
    float t[9][3];
    sample(tex, w, h, u - x, v + y, t[TA]);
    sample(tex, w, h, u, v + y, t[TB]);
    sample(tex, w, h, u + x, v + y, t[TC]);
    sample(tex, w, h, u - x, v, t[TD]);
    sample(tex, w, h, u, v, t[TE]);
    sample(tex, w, h, u + x, v, t[TF]);
    sample(tex, w, h, u - x, v - y, t[TG]);
    sample(tex, w, h, u, v - y, t[TH]);
    sample(tex, w, h, u + x, v - y, t[TI]);
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch)
        out[ch] = t[TE][ch] * 0.25f + (t[TB][ch] + t[TD][ch] + t[TF][ch] + t[TH][ch]) * 0.125f + (t[TA][ch] + t[TC][ch] + t[TG][ch] + t[TI][ch]) * 0.0625f;
}
PVQ_HD void composite(int composite_mode, float b, const float tent_rgb[3], float dst[3]) {
    PVQ_FP_STRICT
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch)
        dst[ch] = composite_mode == ADDITIVE ? dst[ch] + b * tent_rgb[ch] : dst[ch] * (1.0f - b) + b * tent_rgb[ch];
}

// ---- the display transform and the encode ----
template <class Lm = Libm>
PVQ_HD_FLAT void display(int tonemapping, const float in[3], float out[3]) {
    PVQ_FP_STRICT
    const float c[3] = {fmaxf(in[0], 0.0f), fmaxf(in[1], 0.0f), fmaxf(in[2], 0.0f)};
    if (tonemapping == TONEMAP_NONE) {
        PVQ_UNROLL
        for (int ch = 0; ch < 3; ++ch) out[ch] = c[ch];
        return;
    }
    const float y = luma(c);
    const float cb = c[0] * -0.1146f + c[1] * -0.3854f + c[2] * 0.5f;
    const float cr = c[0] * 0.5f + c[1] * -0.4542f + c[2] * -0.0458f;
    const float bt = 1.0f - Lm::exp(-(sqrtf(cb * cb + cr * cr) * 2.4f));
    float desat = fmaxf((bt - 0.7f) * 0.8f, 0.0f);
    desat *= desat;
    const float scale = fmaxf(0.0f, (1.0f - Lm::exp(-y)) / fmaxf(1e-5f, y));
    const float mix = bt * bt;
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        const float desat_col = c[ch] + (y - c[ch]) * desat;
        const float tm0 = c[ch] * scale, tm1 = 1.0f - Lm::exp(-desat_col);
        out[ch] = (tm0 + (tm1 - tm0) * mix) * 0.97f;
    }
}
PVQ_HD uint32_t unorm8(float v) {   // v in [0, 1]
    PVQ_FP_STRICT
    return static_cast<uint32_t>(floorf(v * 255.0f + 0.5f));
}
// r | g << 8 | b << 16 | a << 24: the bytes in memory order
template <class Lm = Libm>
PVQ_HD_FLAT uint32_t encode(const float rgb[3], float alpha) {
    PVQ_FP_STRICT
    uint32_t px = 0u;
    PVQ_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        const float v = raster::w_clamp(rgb[ch], 0.0f, 1.0f);
        const float e = v <= 0.0031308f ? 12.92f * v : 1.055f * Lm::pow(v, 1.0f / 2.4f) - 0.055f;
        px |= unorm8(raster::w_clamp(e, 0.0f, 1.0f)) << (8 * ch);
    }
    return px | unorm8(raster::w_clamp(alpha, 0.0f, 1.0f)) << 24;
}

// ---- a tile's footprint ----
// The source texels along one axis that outputs i0 .. i0 + n of a wt-texel target can sample in a ws-texel source, with taps
// up to `margin` source texels either side: lo .. lo + count.  Two texels of slack beyond the bilinear pair cover the rounding of
// the coordinates, and every sampled index is clamped into 0 .. ws - 1 as the footprint is.
PVQ_HD void footprint(uint32_t i0, uint32_t n, uint32_t wt, uint32_t ws, float margin, uint32_t& lo, uint32_t& count) {
    PVQ_FP_STRICT
    const uint32_t last = (i0 + n < wt ? i0 + n : wt) - 1u;
    const float a = pixel_uv(i0, wt) * static_cast<float>(ws), b = pixel_uv(last, wt) * static_cast<float>(ws);
    const int l = static_cast<int>(floorf(a - margin)) - 2, h = static_cast<int>(floorf(b + margin)) + 2;
    lo = l < 0 ? 0u : (static_cast<uint32_t>(l) >= ws ? ws - 1u : static_cast<uint32_t>(l));
    const uint32_t hi = h < 0 ? 0u : (static_cast<uint32_t>(h) >= ws ? ws - 1u : static_cast<uint32_t>(h));
    count = hi - lo + 1u;
}

}  // namespace present
}  // namespace pvq
