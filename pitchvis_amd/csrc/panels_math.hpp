// panels_math.hpp — the one copy of the debug panels' per-frame arithmetic, for the host face (panels_host.cpp, g++) and the device
// stage (panels_batch.hip): the three meshes of DisplayMode::Debugging, pitchvis_viewer/src/display_system/update.rs
//   * update_spectrum             :474-638  the smoothed spectrum as a thick line with a 12-segment disc on every continuous peak
//   * update_scene_calmness_graph :640-742  the last `capacity` values of smoothed_scene_calmness as a thick line
//   * update_calmness_histogram   :744-869  the per-bin calmness as a thick line
// with calmness_to_color (:27-35) and CircleGeometry::new (:435-471).
//
// Every expression is the reference's f32 expression, operation for operation, FMA contraction off on both sides, `/` the correctly
// rounded division.  Two calls are not the four IEEE operations: f32::hypot, taken as the double-precision function rounded once to
// f32 — (float)sqrt((double)dx * dx + (double)dy * dy), both products exact in double — and powf(t, 0.5), taken as the correctly
// rounded f32 square root.  Neither face evaluates anything else of libm per frame: the colour of a bucket and the twelve angles of
// a disc are tables the host builds once (panels_host.hpp).
//
// The histogram's `l < 0.0001` skip (update.rs:818-820) never fires: l >= |dx|, and |dx| = |i * 0.011 - (i + 1) * 0.011| is 0.011 to
// within a few ulp for every bin count the project admits (at most 1024), so the panel always has n_bins - 1 quads.
#pragma once

#include "scene_math.hpp"

namespace pvq {
namespace panels {

constexpr float X_STEP = 0.011f;               // update.rs:520, :583, :801-802
constexpr float SPECTRUM_THICKNESS = 0.02f;    // update.rs:523
constexpr float CALMNESS_THICKNESS = 0.01f;    // update.rs:673, :793
constexpr float HEIGHT_SCALE = 0.5f;           // update.rs:794
constexpr float DISC_RADIUS = 0.08f;           // update.rs:605
constexpr float DISC_ALPHA = 0.9f;             // update.rs:600
constexpr uint32_t DISC_SEGMENTS = 12;         // update.rs:607
constexpr uint32_t DISC_VERTICES = 13;         // the centre, then the perimeter
constexpr float TAU_F = 6.28318548202514648438f;   // std::f32::consts::TAU
constexpr uint32_t DEFAULT_GRAPH_CAPACITY = 300;   // app/common.rs:2037
constexpr float SPECTRUM_EASING = 10.0f;       // update.rs:568, :596: the literal, not EASING_POW

// Rust `as usize` of an f32: saturating, NaN -> 0
PVQ_HD uint64_t sat_u64(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 18446744073709551616.0f) return 0xFFFFFFFFFFFFFFFFull;
    return static_cast<uint64_t>(v);
}

// update.rs:531-541 = :691-700 = :815-827: the quad of segment (p, q) with thickness t; out: v0, v1, v2, v3 as x, y, z
PVQ_HD_FLAT void thick_quad(float px, float py, float qx, float qy, float t, float out[12]) {
    PVQ_FP_STRICT
    const float dx = px - qx;
    const float dy = py - qy;
    const float l = static_cast<float>(::sqrt(static_cast<double>(dx) * dx + static_cast<double>(dy) * dy));   // dx.hypot(dy)
    const float u = dx * t * 0.5f / l;
    const float v = dy * t * 0.5f / l;
    out[0] = px + v; out[1] = py - u; out[2] = 0.0f;
    out[3] = px - v; out[4] = py + u; out[5] = 0.0f;
    out[6] = qx - v; out[7] = qy + u; out[8] = 0.0f;
    out[9] = qx + v; out[10] = qy - u; out[11] = 0.0f;
}

// update.rs:516-524 with :531-541: segment i of the spectrum line from x[i], x[i + 1]
PVQ_HD_FLAT void spectrum_quad(uint32_t i, float x0, float x1, float out[12]) {
    PVQ_FP_STRICT
    thick_quad(static_cast<float>(i) * X_STEP, x0 / 10.0f, static_cast<float>(i + 1u) * X_STEP, x1 / 10.0f, SPECTRUM_THICKNESS, out);
}
// update.rs:570: powf(0.5) as the correctly rounded square root
PVQ_HD float spectrum_alpha(float x, float max_size) {
    PVQ_FP_STRICT
    return 1.0f - sqrtf(0.5f - x / max_size / 2.0f);
}

// update.rs:798-802 with :815-827: segment i of the calmness histogram from calmness[i], calmness[i + 1]
PVQ_HD_FLAT void histogram_quad(uint32_t i, float c0, float c1, float out[12]) {
    PVQ_FP_STRICT
    thick_quad(static_cast<float>(i) * X_STEP, c0 * HEIGHT_SCALE, static_cast<float>(i + 1u) * X_STEP, c1 * HEIGHT_SCALE, CALMNESS_THICKNESS, out);
}
PVQ_HD float histogram_class_value(float c0, float c1) {   // update.rs:805
    PVQ_FP_STRICT
    return (c0 + c1) / 2.0f;
}

// update.rs:662-667 with :691-700: segment i of the graph from the window's values h[i], h[i + 1]
PVQ_HD_FLAT void graph_quad(uint32_t i, uint32_t capacity, float h0, float h1, float out[12]) {
    PVQ_FP_STRICT
    const float c = static_cast<float>(capacity);
    thick_quad(static_cast<float>(i) / c - 0.5f, h0, static_cast<float>(i + 1u) / c - 0.5f, h1, CALMNESS_THICKNESS, out);
}

// update.rs:27-35; Color::srgb(..).to_srgba() gives its arguments back with alpha 1.0
PVQ_HD void calmness_to_color(float calmness, float& r, float& g, float& b) {
    if (calmness > 0.7f) {
        r = 0.5f; g = 0.8f; b = 1.0f;
    } else if (calmness > 0.3f) {
        r = 1.0f; g = 1.0f; b = 0.5f;
    } else {
        r = 1.0f; g = 0.5f; b = 0.5f;
    }
}

// update.rs:583-587: the disc of a peak: its centre and its entry of the bucket colour table
PVQ_HD void disc_of_peak(uint32_t bpo, float center, float size, float& cx, float& cy, uint32_t& color_at) {
    PVQ_FP_STRICT
    cx = center * X_STEP;
    cy = size / 10.0f;
    color_at = static_cast<uint32_t>(sat_u64(roundf(center)) % bpo);
}
// update.rs:442, :446-455: coordinate `comp` (0: x, 1: y, 2: z) of vertex `vtx` (0: the centre, 1 + i: perimeter point i);
// cs: the twelve (cos a_i, sin a_i)
PVQ_HD float disc_coordinate(float cx, float cy, const float* cs, uint32_t vtx, uint32_t comp) {
    PVQ_FP_STRICT
    if (comp == 2u) return 0.0f;
    const float c = comp == 0u ? cx : cy;
    if (vtx == 0u) return c;
    return c + DISC_RADIUS * cs[2u * (vtx - 1u) + comp];
}

}  // namespace panels
}  // namespace pvq
