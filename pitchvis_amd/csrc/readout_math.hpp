// readout_math.hpp — the one copy of the readout stage's rule, for the host object (readout_host.cpp, g++) and the device stage
// (readout_batch.hip): the text of a value (Rust's format!("{:>3.0}") of the rounded value), the colour of that text
// (pitchvis_viewer/src/app/common.rs:404-413), the pen fold, the node's box and where a glyph's origin lands.  include/pvq.h, "the
// readout", states the rule; what it assumes of the viewer's UI text pipeline is DESIGN.md 6k's table.  The glyph coverage itself
// is text_math.hpp's, unchanged.
//
// All of it is f32, FMA contraction off on both sides; the decimal digits are integer arithmetic on a uint32 (no libm, no
// snprintf), so the host face and the device carry the same bits.
#pragma once

#include "text_math.hpp"

namespace pvq {
namespace readout {

constexpr uint32_t N_PREFIX = 14;                              // "Tuning drift: "
constexpr uint32_t MAX_VALUE_CHARS = 11;                       // "-2147483520"
constexpr uint32_t MAX_SLOTS = N_PREFIX + MAX_VALUE_CHARS;     // glyph slots of a row
constexpr uint32_t N_GLYPHS = 24;                              // codepoints the stage can emit, ascending: the atlas's order
constexpr float FONT_PX = 16.0f;                               // common.rs:350
constexpr float MAX_ABS = 2147483520.0f;                       // the largest f32 below 2^31: a larger finite |r| is formatted as this
constexpr float BOX_ALPHA = 0.5f;                              // common.rs:369, Color::BLACK.with_alpha(0.5)
constexpr float EDGE = 0.01f;                                  // common.rs:361-362, Val::Percent(1.)

// atlas index -> codepoint: ' ' '-' '0'..'9' ':' 'N' 'T' 'a' 'd' 'f' 'g' 'i' 'n' 'r' 't' 'u'
PVQ_HD uint32_t codepoint_of(uint32_t g) {
    if (g >= 2u && g <= 11u) return 0x30u + (g - 2u);
    switch (g) {
        case 0: return 0x20u;
        case 1: return 0x2Du;
        case 12: return 0x3Au;
        case 13: return 0x4Eu;
        case 14: return 0x54u;
        case 15: return 0x61u;
        case 16: return 0x64u;
        case 17: return 0x66u;
        case 18: return 0x67u;
        case 19: return 0x69u;
        case 20: return 0x6Eu;
        case 21: return 0x72u;
        case 22: return 0x74u;
        default: return 0x75u;
    }
}
// codepoint -> atlas index, N_GLYPHS for one the stage never emits
PVQ_HD uint32_t glyph_of(uint32_t cp) {
    for (uint32_t g = 0; g < N_GLYPHS; ++g)
        if (codepoint_of(g) == cp) return g;
    return N_GLYPHS;
}
// "Tuning drift: " as atlas indices
PVQ_HD uint32_t prefix_glyph(uint32_t i) {
    switch (i) {
        case 0: return 14u;    // T
        case 1: return 23u;    // u
        case 2: return 20u;    // n
        case 3: return 19u;    // i
        case 4: return 20u;    // n
        case 5: return 18u;    // g
        case 6: return 0u;     // ' '
        case 7: return 16u;    // d
        case 8: return 21u;    // r
        case 9: return 19u;    // i
        case 10: return 17u;   // f
        case 11: return 22u;   // t
        case 12: return 12u;   // :
        default: return 0u;    // ' '
    }
}

PVQ_HD uint32_t bits_of(float v) {
    uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(v);
#else
    memcpy(&bits, &v, 4);
#endif
    return bits;
}

// The value text of v as atlas indices, five bits a character: character k of the n (3 .. MAX_VALUE_CHARS) in bits 5 k .. 5 k + 4 of
// `packed` (a register, not an array: the device indexes it by a shift).  r is roundf(v) (half away from zero, f32::round), which
// the colour takes.  The text is format!("{r:>3.0}"): digits, '-' for a negative r (-0 included), spaces on the left up to three
// characters; "NaN", "inf", "-inf".
PVQ_HD uint32_t value_glyphs(float v, uint64_t& packed, float& r) {
    r = roundf(v);
    const uint32_t bits = bits_of(r);
    const bool negative = (bits >> 31) != 0u;
    const uint32_t magnitude = bits & 0x7FFFFFFFu;
    if (magnitude > 0x7F800000u) {   // NaN: no sign
        packed = 13u | 15u << 5 | 13u << 10;
        return 3;
    }
    if (magnitude == 0x7F800000u) {
        packed = 19u | 20u << 5 | 17u << 10;   // inf
        if (negative) packed = packed << 5 | 1u;
        return negative ? 4u : 3u;
    }
    const float a = fabsf(r);
    uint32_t u = a > MAX_ABS ? 2147483520u : static_cast<uint32_t>(a);   // a is an integer below 2^31: the cast is exact
    uint32_t n = 0;
    packed = 0;
    do {   // from the last digit: each new character goes in front of those there
        packed = packed << 5 | (2u + u % 10u);
        u /= 10u;
        ++n;
    } while (u != 0u);
    if (negative) packed = packed << 5 | 1u, ++n;
    for (; n < 3u; ++n) packed = packed << 5;   // a space is index 0
    return n;
}

// the value text's sRGB colour, common.rs:404-413 in its expression order; a NaN fails every comparison: red
PVQ_HD void value_srgb(float r, float srgb[3]) {
    PVQ_FP_STRICT
    const float a = fabsf(r);
    srgb[2] = 0.0f;
    if (a <= 10.0f) srgb[0] = 0.0f, srgb[1] = 1.0f;
    else if (a <= 20.0f) srgb[0] = (a - 10.0f) / (20.0f - 10.0f), srgb[1] = 1.0f;
    else if (a <= 30.0f) srgb[0] = 1.0f, srgb[1] = 1.0f - (a - 20.0f) / (30.0f - 20.0f);
    else srgb[0] = 1.0f, srgb[1] = 0.0f;
}

// glyph slot i of a row's string: the prefix, then the value text
PVQ_HD uint32_t slot_glyph(uint64_t value, uint32_t i) {
    return i < N_PREFIX ? prefix_glyph(i) : static_cast<uint32_t>(value >> (5u * (i - N_PREFIX))) & 31u;
}

// The pen: the sequential left fold p_0 = 0, p_{i + 1} = p_i + advance[glyph_i] over the n slots of the string.  Returns p_n, the
// text's width; p_at is p_slot (slot <= n).
PVQ_HD float pen_fold(const float advance[N_GLYPHS], uint64_t value, uint32_t n, uint32_t slot, float& p_at) {
    PVQ_FP_STRICT
    float p = 0.0f;
    p_at = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {
        p = p + advance[slot_glyph(value, i)];
        if (i + 1u == slot) p_at = p;
    }
    return p;
}

// the node's box for a text of width text_w at font size F on a W x H image (pixel coordinates from the top left)
struct Box {
    float xl, xr, yt, yb;
};
PVQ_HD Box box_of(uint32_t W, uint32_t H, float text_w, float F) {
    PVQ_FP_STRICT
    const float Wf = static_cast<float>(W), Hf = static_cast<float>(H);
    Box b;
    b.xr = Wf - EDGE * Wf;
    b.yb = Hf - EDGE * Hf;
    b.xl = b.xr - text_w;
    b.yt = b.yb - text::LINE_HEIGHT * F;
    return b;
}
// a glyph's origin column for the pen p, and the baseline row for the handle's baseline offset: no sub-pixel positions
PVQ_HD float origin_column(const Box& b, float p) {
    PVQ_FP_STRICT
    return floorf(b.xl + p + 0.5f);
}
PVQ_HD float baseline_row(const Box& b, float baseline) {
    PVQ_FP_STRICT
    return floorf(b.yt + baseline + 0.5f);
}
// the box covers the pixels whose centre lies in [xl, xr) x [yt, yb)
PVQ_HD bool in_box(const Box& b, uint32_t i, uint32_t j) {
    PVQ_FP_STRICT
    const float cx = static_cast<float>(i) + 0.5f, cy = static_cast<float>(j) + 0.5f;
    return cx >= b.xl && cx < b.xr && cy >= b.yt && cy < b.yb;
}

// a glyph's cell in the atlas: the pixel box its outline's bounding box meets, relative to (origin column, baseline row)
struct Cell {
    int32_t x0, y0;      // first column and row; a left bearing makes x0 negative, y0 is negative above the baseline
    uint32_t w, h;       // 0 x 0: no outline (the space)
    uint32_t offset;     // of its [h][w] coverages in the atlas
    float advance;       // (float)(advance * k)
};
static_assert(sizeof(Cell) == 24, "three 8-byte loads");

// the box, then a glyph at `coverage`: what a pixel becomes
PVQ_HD void blend_box(float dst[4]) {
    const float src[4] = {0.0f, 0.0f, 0.0f, BOX_ALPHA};
    raster::blend(src, dst);
}

}  // namespace readout
}  // namespace pvq
