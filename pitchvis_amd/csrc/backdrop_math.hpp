// backdrop_math.hpp — the one copy of the picture behind the pitch balls, for the host face (backdrop_host.cpp, g++) and the device
// stage (backdrop_batch.hip): the spider net, the lit bass spiral and the three debug panels are lists of flat-coloured triangles
// in world units, blended in a fixed order (pvq.h has the table of layers).  What is here: the static geometry
// (pitchvis_viewer/src/display_system/setup.rs:127-222 with mod.rs:277-306), the coverage rule, and a triangle made ready to be
// drawn.  Camera and blend are raster_math.hpp's.
//
// All of it is f32, FMA contraction off on both sides.  The libm calls of the static geometry go through scene_math.hpp and
// panels_math.hpp: double-precision functions rounded once to f32.
//
// The coverage rule.  One sample per pixel, at its centre p.  An edge between two vertices is evaluated from its canonically ordered
// endpoints — lo is the endpoint with the smaller x, then the smaller y — as
//     e = (hi.x - lo.x) * (p.y - lo.y) - (hi.y - lo.y) * (p.x - lo.x)
// so two triangles that share an edge compute the same number for it.  A triangle's sign for an edge is the sign of e at its third
// vertex.  p is inside when, for all three edges, e has the triangle's sign, or e == 0 and the triangle's sign is positive: an edge
// through a pixel centre goes to exactly one of the two triangles beside it.  Both windings are drawn.  A triangle with a zero or
// non-finite sign, a non-finite vertex or a non-finite colour draws nothing.
//
// Multisampling (samples = 4; the reference's desktop and wasm builds, Msaa::Sample4).  A pixel has four samples at the standard
// positions (sample_fraction below), each with a destination of its own that starts from the clear colour or the background's
// pixel.  Every sample runs the rule above unchanged at its own position — a tie e == 0 still goes to the triangle whose sign is
// positive, and two triangles that share an edge still compute the same number for it at every sample — and a covered sample is
// blended with the triangle's flat colour, in list order.  At the end of the backdrop the pixel is the unweighted mean of its
// samples (resolve4).  samples = 1 is the rule above: one sample at (0.5, 0.5).
#pragma once

#include <cstddef>

#include "panels_math.hpp"
#include "raster_math.hpp"

namespace pvq {
namespace backdrop {

constexpr float NET_THICKNESS = 0.05f;            // setup.rs:197, :215
constexpr float NET_GRAY = 0.3f;                  // setup.rs:200, :220 (sRGB)
constexpr float RAY_RADIUS_PER_OCTAVE = 2.2f;     // setup.rs:184
constexpr uint32_t RAYS = 12;                     // setup.rs:182
constexpr uint32_t POINTS_PER_OCTAVE = 72;        // 12 * SPIRAL_SEGMENTS_PER_SEMITONE, setup.rs:48
constexpr uint32_t BASS_POINTS = 168;             // HIGHEST_BASSNOTE * SPIRAL_SEGMENTS_PER_SEMITONE, setup.rs:136
constexpr float BASS_WIDTH = 0.05f;               // setup.rs:159
constexpr float BASS_EXTRA_LENGTH = 0.01f;        // setup.rs:159
constexpr float GRAPH_TX = -5.0f, GRAPH_TY = -6.5f, GRAPH_SX = 3.0f, GRAPH_SY = 1.0f;   // setup.rs:284-288
constexpr float PANEL_MARGIN_X = 0.2f, PANEL_DROP_Y = 4.2f;                             // update.rs:496-500, :776-781

enum What { NET_SPIRAL = 0, NET_RAYS = 1, BASS = 2 };

PVQ_HD uint32_t spiral_points(uint32_t octaves) { return POINTS_PER_OCTAVE * octaves; }
PVQ_HD uint32_t geometry_count(uint32_t octaves, int what) {
    if (what == NET_RAYS) return RAYS;
    const uint32_t pts = spiral_points(octaves);
    if (what == NET_SPIRAL) return pts - 1u;
    return (pts < BASS_POINTS ? pts : BASS_POINTS) - 1u;
}

// quad i of `what`: v0 .. v3 as (x, y); the triangles are the panels' (2, 1, 0) and (2, 0, 3)
PVQ_HD_FLAT void geometry_quad(uint32_t octaves, int what, uint32_t i, float out[8]) {
    PVQ_FP_STRICT
    float q12[12];
    if (what == NET_RAYS) {   // setup.rs:182-191
        const float radius = static_cast<float>(octaves) * RAY_RADIUS_PER_OCTAVE;
        const float angle = static_cast<float>(i) / 12.0f * 2.0f * scene::PI_F;
        const float px = scene::SceneMath::cos(angle), py = scene::SceneMath::sin(angle);
        panels::thick_quad(0.0f, 0.0f, radius * px, radius * py, NET_THICKNESS, q12);
        for (int v = 0; v < 4; ++v) {
            out[2 * v] = q12[3 * v];
            out[2 * v + 1] = q12[3 * v + 1];
        }
        return;
    }
    float px, py, qx, qy;
    scene::bin_to_spiral(POINTS_PER_OCTAVE, static_cast<float>(i), px, py);
    scene::bin_to_spiral(POINTS_PER_OCTAVE, static_cast<float>(i + 1u), qx, qy);
    if (what == NET_SPIRAL) {   // setup.rs:209-216
        panels::thick_quad(px, py, qx, qy, NET_THICKNESS, q12);
        for (int v = 0; v < 4; ++v) {
            out[2 * v] = q12[3 * v];
            out[2 * v + 1] = q12[3 * v + 1];
        }
        return;
    }
    // setup.rs:141-159, restated: a rectangle 0.05 wide and h + 0.01 long, centred on the midpoint, its long axis along p - q
    const float dx = px - qx, dy = py - qy;
    const float h = static_cast<float>(::sqrt(static_cast<double>(dx) * dx + static_cast<double>(dy) * dy));
    const float mx = (px + qx) * 0.5f, my = (py + qy) * 0.5f;
    const float ux = dx / h, uy = dy / h;                      // the long axis
    const float hw = BASS_WIDTH * 0.5f, hl = (h + BASS_EXTRA_LENGTH) * 0.5f;
    const float ax = hw * uy, ay = hw * -ux;                   // half the width, along the normal
    const float bx = hl * ux, by = hl * uy;                    // half the length
    out[0] = mx + ax + bx; out[1] = my + ay + by;
    out[2] = mx - ax + bx; out[3] = my - ay + by;
    out[4] = mx - ax - bx; out[5] = my - ay - by;
    out[6] = mx + ax - bx; out[7] = my + ay - by;
}

// the reference's placement of the three panels: out[0] spectrum, out[1] histogram, out[2] graph, each (tx, ty, sx, sy)
PVQ_HD void panel_transforms(uint32_t n_bins, uint32_t W, uint32_t H, float vh, float out[12]) {
    PVQ_FP_STRICT
    const float max_y = vh / 2.0f;
    const float max_x = max_y * (static_cast<float>(W) / static_cast<float>(H));
    const float tx = max_x - static_cast<float>(n_bins) * panels::X_STEP - PANEL_MARGIN_X, ty = max_y - PANEL_DROP_Y;
    out[0] = tx; out[1] = ty; out[2] = 1.0f; out[3] = 1.0f;
    out[4] = tx; out[5] = ty; out[6] = 1.0f; out[7] = -1.0f;
    out[8] = GRAPH_TX; out[9] = GRAPH_TY; out[10] = GRAPH_SX; out[11] = GRAPH_SY;
}

// ---- a triangle, ready to be drawn: 80 bytes, five 16-byte words; the first holds what the box test reads ----
struct Tri {
    uint32_t box_x, box_y;      // first | last << 16 of the pixel columns / rows that can be covered
    uint32_t positive;          // bit k: the triangle's sign for edge k is positive
    uint32_t pad;
    float edge[3][4];           // lo.x, lo.y, hi.x - lo.x, hi.y - lo.y
    float rgba[4];              // linear
};
static_assert(sizeof(Tri) == 80 && offsetof(Tri, edge) == 16 && offsetof(Tri, rgba) == 64, "workspace layout");

PVQ_HD float edge_value(const float e[4], float px, float py) {
    PVQ_FP_STRICT
    return e[2] * (py - e[1]) - e[3] * (px - e[0]);
}

// edge (a, b) with third vertex c -> its canonical data and the triangle's sign for it: 1, -1, or 0 (draws nothing)
PVQ_HD int make_edge(float ax, float ay, float bx, float by, float cx, float cy, float e[4]) {
    PVQ_FP_STRICT
    const bool a_lo = ax < bx || (ax == bx && ay <= by);
    const float lx = a_lo ? ax : bx, ly = a_lo ? ay : by, hx = a_lo ? bx : ax, hy = a_lo ? by : ay;
    e[0] = lx; e[1] = ly; e[2] = hx - lx; e[3] = hy - ly;
    const float s = edge_value(e, cx, cy);
    if (!raster::finite_f(s) || s == 0.0f) return 0;
    return s > 0.0f ? 1 : -1;
}

// The pixel columns and rows outside of which the rule covers nothing: an acceleration only, so it errs outwards.  A pixel passes
// the three f32 tests only if it lies within d of the exact triangle's three half planes, d = (rounding error of e) / (edge
// length) <= 8 * 2^-24 * R with R the largest |p - lo| that can occur; the three half planes moved out by d meet within
// d / sin(smallest angle / 2) <= 2 d Lmax^2 / (2 area) of the vertices.  The box is the vertices' box widened by twice that and a
// pixel.  false: nothing of the triangle is on the image.  The arithmetic is double precision and not held to one evaluation order
// (the device may contract it): the host's and the device's box of a triangle need not be equal, and nothing may rely on that —
// both contain every pixel the rule covers, which is all the pictures depend on.
//
// With four samples the same box holds every pixel that has a covered sample.  For the left side: a covered sample lies at
// x >= xmin - slack (the argument above is about a position, not about a centre), and the sample of column i lies at
// (i + fx - 0.5 W) s with fx <= 0.875, so i >= A + 0.5 - fx >= A - 0.375 with A = (xmin - slack) / s + 0.5 W - 0.5, and since i is
// a whole number i >= floor(A) > floor(A) - 1, the box's first column.  No sample is further than 0.375 pixel from its centre and
// the box is widened by a whole pixel on every side, so the other three sides go the same way.  The multisampled parity tests,
// whose model uses no boxes, are the check.
PVQ_HD bool tri_box(const float v[6], uint32_t W, uint32_t H, float vh, uint32_t& box_x, uint32_t& box_y) {
    const double s = static_cast<double>(vh / static_cast<float>(H));
    const double x0 = v[0], y0 = v[1], x1 = v[2], y1 = v[3], x2 = v[4], y2 = v[5];
    const double xmin = fmin(x0, fmin(x1, x2)), xmax = fmax(x0, fmax(x1, x2));
    const double ymin = fmin(y0, fmin(y1, y2)), ymax = fmax(y0, fmax(y1, y2));
    const double area2 = fabs((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0));
    const double l01 = (x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0), l12 = (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1),
                 l20 = (x0 - x2) * (x0 - x2) + (y0 - y2) * (y0 - y2);
    const double lmax2 = fmax(l01, fmax(l12, l20));
    const double reach = fabs(xmin) + fabs(xmax) + fabs(ymin) + fabs(ymax) + s * (static_cast<double>(W) + H);
    const double slack = 2.0e-6 * reach * lmax2 / area2 + 2.4e-7 * reach;   // (area2 == 0: inf or NaN, the whole image)
    double c0 = floor((xmin - slack) / s + 0.5 * W - 0.5) - 1.0, c1 = ceil((xmax + slack) / s + 0.5 * W - 0.5) + 1.0;
    double r0 = floor(0.5 * H - 0.5 - (ymax + slack) / s) - 1.0, r1 = ceil(0.5 * H - 0.5 - (ymin - slack) / s) + 1.0;
    if (!(c0 <= c1) || !(r0 <= r1)) {   // NaN: the whole image
        c0 = r0 = 0.0;
        c1 = W - 1.0;
        r1 = H - 1.0;
    }
    if (c1 < 0.0 || r1 < 0.0 || c0 > W - 1.0 || r0 > H - 1.0) return false;
    c0 = c0 < 0.0 ? 0.0 : c0;
    r0 = r0 < 0.0 ? 0.0 : r0;
    c1 = c1 > W - 1.0 ? W - 1.0 : c1;
    r1 = r1 > H - 1.0 ? H - 1.0 : r1;
    box_x = static_cast<uint32_t>(c0) | static_cast<uint32_t>(c1) << 16;
    box_y = static_cast<uint32_t>(r0) | static_cast<uint32_t>(r1) << 16;
    return true;
}

// x * sx + tx, y * sy + ty; t null: as it is
PVQ_HD void place(const float* t, float x, float y, float& ox, float& oy) {
    PVQ_FP_STRICT
    ox = t ? x * t[2] + t[0] : x;
    oy = t ? y * t[3] + t[1] : y;
}

// v: the three vertices in world units (placed), rgba: the linear colour.  false: the triangle draws nothing on this image.
PVQ_HD_FLAT bool make_tri(const float v[6], const float rgba[4], uint32_t W, uint32_t H, float vh, Tri& o) {
    bool ok = true;
    for (int i = 0; i < 6; ++i) ok = ok && raster::finite_f(v[i]);
    for (int i = 0; i < 4; ++i) ok = ok && raster::finite_f(rgba[i]);
    if (!ok) return false;
    const int s0 = make_edge(v[0], v[1], v[2], v[3], v[4], v[5], o.edge[0]);
    const int s1 = make_edge(v[2], v[3], v[4], v[5], v[0], v[1], o.edge[1]);
    const int s2 = make_edge(v[4], v[5], v[0], v[1], v[2], v[3], o.edge[2]);
    if (s0 == 0 || s1 == 0 || s2 == 0) return false;
    o.positive = (s0 > 0 ? 1u : 0u) | (s1 > 0 ? 2u : 0u) | (s2 > 0 ? 4u : 0u);
    o.pad = 0u;
    for (int i = 0; i < 4; ++i) o.rgba[i] = rgba[i];
    return tri_box(v, W, H, vh, o.box_x, o.box_y);
}

// the rule at the pixel centre (px, py)
PVQ_HD bool covers(const Tri& t, float px, float py) {
    bool in = true;
    for (int k = 0; k < 3; ++k) {
        const float e = edge_value(t.edge[k], px, py);
        in = in && (((t.positive >> k) & 1u) ? e >= 0.0f : e < 0.0f);
    }
    return in;
}

// ---- multisampling: the sample positions, a sample's world position, the resolve ----
constexpr uint32_t MAX_SAMPLES = 4;
PVQ_HD bool samples_ok(uint32_t samples) { return samples == 1u || samples == 4u; }

// sample k of `samples` (1 or 4), in pixel units from the pixel's top-left corner: the standard four-sample pattern that Vulkan's
// standard sample locations, D3D and Metal share, in their order; one sample sits at the centre
PVQ_HD void sample_fraction(uint32_t samples, uint32_t k, float& fx, float& fy) {
    if (samples == 1u) {
        fx = 0.5f;
        fy = 0.5f;
        return;
    }
    fx = k == 0u ? 0.375f : (k == 1u ? 0.875f : (k == 2u ? 0.125f : 0.625f));
    fy = k == 0u ? 0.125f : (k == 1u ? 0.375f : (k == 2u ? 0.625f : 0.875f));
}

// The world position of the point (fx, fy) of pixel (i, j): raster::pixel_world with 0.5 replaced by the fractions, and with
// (0.5, 0.5) that function bit for bit (the same expressions in the same order).  i + fx and j + fy are exact for every admitted
// image: the sides are <= 4096 = 2^12 and the fractions are eighths, so the sum needs 15 of f32's 24 bits.
PVQ_HD void sample_world(uint32_t i, uint32_t j, uint32_t W, uint32_t H, float vh, float fx, float fy, float& wx, float& wy) {
    PVQ_FP_STRICT
    const float s = vh / static_cast<float>(H);
    wx = (static_cast<float>(i) + fx - 0.5f * static_cast<float>(W)) * s;
    wy = (0.5f * static_cast<float>(H) - (static_cast<float>(j) + fy)) * s;
}

// The resolve of one channel: the unweighted mean, in this order.  Four equal finite samples x with |x| < 2^126 resolve to
// exactly x: x + x = 2x and 2x + 2x = 4x are exact below the overflow threshold (|4x| < 2^128), and * 0.25 is exact for a normal
// result and for a subnormal x too (4x / 4 is x again, representable).  Pictures with channels at or beyond 2^126 are not promised.
PVQ_HD float resolve4(float s0, float s1, float s2, float s3) {
    PVQ_FP_STRICT
    return ((s0 + s1) + (s2 + s3)) * 0.25f;
}

// the vertex numbers of triangle t of a mesh of quads (4 vertices each) or of discs (13 each)
PVQ_HD void quad_triangle(uint32_t t, uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& base) {
    base = (t >> 1) * 4u;
    a = base + 2u;
    b = base + ((t & 1u) ? 0u : 1u);
    c = base + ((t & 1u) ? 3u : 0u);
}
PVQ_HD void disc_triangle(uint32_t t, uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& base) {
    const uint32_t d = t / panels::DISC_SEGMENTS, i = t - d * panels::DISC_SEGMENTS;
    base = d * panels::DISC_VERTICES;
    a = base;
    b = base + 1u + i;
    c = base + 1u + (i + 1u) % panels::DISC_SEGMENTS;
}

// the material colours: LinearRgba::from(Color::srgb(0.3, 0.3, 0.3)), and the lit bass segments' LinearRgba::from(srgba(bass_rgba))
PVQ_HD_FLAT void net_color(float out[4]) {
    out[0] = out[1] = out[2] = scene::srgb_to_linear(NET_GRAY);
    out[3] = 1.0f;
}
PVQ_HD_FLAT void bass_color(const float srgba[4], float out[4]) {
    for (int c = 0; c < 3; ++c) out[c] = scene::srgb_to_linear(srgba[c]);
    out[3] = srgba[3];
}

}  // namespace backdrop
}  // namespace pvq
