// overlay_math.hpp — the one copy of the overlay's picture, for the host object (overlay_host.cpp, g++) and the device stage
// (overlay_batch.hip): the scrolling spectrogram quad (pitchvis_viewer/src/display_system/setup.rs:418-517, update.rs:929-1087,
// material.rs:42-71 with assets/shaders/spectrogram_scroll.wgsl) and the twelve chroma boxes (setup.rs:519-541,
// update.rs:1132-1143), restated from their behaviour as include/pvq.h states the rule (its layers 8 and 9).  The assumed
// semantics are DESIGN.md 6g's table.
//
// All of it is f32, FMA contraction off on both sides; `/` and floor are IEEE f32.  The sRGB decode of a texel byte and the
// division of an alpha byte by 255 go through one table built on the host (Tables), for host and device alike, so the model
// (tests/overlay_model.py), the host face and the device carry the same bits.
#pragma once

#include "raster_math.hpp"

namespace pvq {
namespace overlay {

constexpr uint32_t HISTORY_ROWS = 200;                        // setup.rs:430, the texture's height
constexpr uint32_t MIN_HISTORY = 2, MAX_HISTORY = 4096;
constexpr uint32_t MIN_BINS = 3, MAX_BINS = 1024;
constexpr uint32_t BOXES = 12;
constexpr float BOX_LEFT = 400.0f, BOX_PITCH = 45.0f, BOX_SIDE = 40.0f, BOX_BOTTOM = 10.0f, BOX_RADIUS = 4.0f;   // setup.rs:528-532, px

// what a pixel's colour goes through, built once on the host (overlay_host.cpp: overlay_tables)
struct Tables {
    float linear[256];      // scene::srgb_to_linear(byte / 255): an Rgba8UnormSrgb texel's colour channel
    float alpha[256];       // byte / 255
    float box[BOXES][3];    // scene::srgb_to_linear(COLORS[pitch class])
};

// the reference's quad (cx, cy, ex, ey): Rectangle(12 * (h / n_bins), 12) at (-7, 6), turned a quarter
PVQ_HD void reference_quad(uint32_t n_bins, uint32_t history_rows, float q[4]) {
    PVQ_FP_STRICT
    q[0] = -7.0f;
    q[1] = 6.0f;
    q[2] = 12.0f;
    q[3] = 12.0f * (static_cast<float>(history_rows) / static_cast<float>(n_bins));
}

// the material's scroll_offset once the frame's row is written: next = (write_index + 1) % h
PVQ_HD float scroll_of(uint32_t next, uint32_t history_rows) {
    PVQ_FP_STRICT
    return static_cast<float>(next) / static_cast<float>(history_rows);
}

// The quad: the texel (tx, ty) of the texture that the quad shows at the world position (wx, wy); false where the quad does not
// cover it (a NaN covers nothing).
PVQ_HD bool quad_texel(const float q[4], uint32_t n_bins, uint32_t history_rows, float scroll, float wx, float wy, uint32_t& tx,
                       uint32_t& ty) {
    PVQ_FP_STRICT
    const float u = (wy - q[1]) / q[3] + 0.5f;
    const float v = 0.5f - (wx - q[0]) / q[2];
    if (!(u >= 0.0f && u < 1.0f && v >= 0.0f && v < 1.0f)) return false;
    const float t = v + (1.0f - scroll);
    const float v2 = t - floorf(t);                                            // fract: 0 <= v2 < 1
    const uint32_t y = static_cast<uint32_t>(floorf(v2 * static_cast<float>(history_rows)));   // 0 .. h: the product may round up
    const uint32_t x = static_cast<uint32_t>(floorf(u * static_cast<float>(n_bins)));
    ty = y < history_rows - 1u ? y : history_rows - 1u;
    tx = x < n_bins - 1u ? x : n_bins - 1u;
    return true;
}

// Texture row ty holds the ring's row h - 1 - ty, which the frame `age` frames before the one being drawn wrote: with next =
// (write_index + 1) % h, age = (next + ty) % h.  Age h - 1 is the row zeroed for the next frame.
PVQ_HD uint32_t age_of(uint32_t ty, uint32_t next, uint32_t history_rows) {
    const uint32_t a = next + ty;   // < 2 h
    return a >= history_rows ? a - history_rows : a;
}

// a texel (r | g << 8 | b << 16 | a << 24, the bytes in memory order) over the pixel; alpha byte 0 leaves the pixel as it is
PVQ_HD bool texel_draws(uint32_t texel) { return (texel >> 24) != 0u; }
PVQ_HD void blend_texel(const float* linear, const float* alpha, uint32_t texel, float dst[4]) {
    const float src[4] = {linear[texel & 0xFFu], linear[(texel >> 8) & 0xFFu], linear[(texel >> 16) & 0xFFu], alpha[texel >> 24]};
    raster::blend(src, dst);
}

// The boxes: the chroma box whose rounded rectangle holds the centre of pixel (i, j) of an image H rows high, or BOXES.  Box pc
// spans x from (400 + 45 pc) s, 40 s wide, and y from H - 50 s to H - 10 s, both half-open; in the four 4 s corner squares the
// centre lies within 4 s of the corner circle's centre.
PVQ_HD uint32_t box_at(uint32_t i, uint32_t j, uint32_t H, float s) {
    PVQ_FP_STRICT
    const float px = static_cast<float>(i) + 0.5f, py = static_cast<float>(j) + 0.5f;
    const float y0 = static_cast<float>(H) - (BOX_BOTTOM + BOX_SIDE) * s, y1 = static_cast<float>(H) - BOX_BOTTOM * s;
    if (!(py >= y0 && py < y1)) return BOXES;
    const float r = BOX_RADIUS * s;
    for (uint32_t pc = 0; pc < BOXES; ++pc) {
        const float x0 = (BOX_LEFT + BOX_PITCH * static_cast<float>(pc)) * s, x1 = x0 + BOX_SIDE * s;
        if (!(px >= x0 && px < x1)) continue;
        const float lx = x0 + r, hx = x1 - r, ly = y0 + r, hy = y1 - r;
        const float dx = px < lx ? px - lx : (px > hx ? px - hx : 0.0f);
        const float dy = py < ly ? py - ly : (py > hy ? py - hy : 0.0f);
        if (dx != 0.0f && dy != 0.0f && !(dx * dx + dy * dy <= r * r)) return BOXES;   // a corner square, outside its circle
        return pc;                                                                    // the boxes do not overlap
    }
    return BOXES;
}
// a strength that is not finite or is <= 0 draws nothing
PVQ_HD bool strength_draws(float strength) { return raster::finite_f(strength) && strength > 0.0f; }
PVQ_HD void blend_box(const float rgb[3], float strength, float dst[4]) {
    const float src[4] = {rgb[0], rgb[1], rgb[2], strength};
    raster::blend(src, dst);
}

}  // namespace overlay
}  // namespace pvq
