// text_math.hpp — the one copy of the text stage's coverage rule, for the host object (text_host.cpp, g++) and the device stage
// (text_batch.hip): how much of a pixel square a label's outline covers, from the label's list of directed line segments in output
// pixel coordinates (text_host.cpp lays the label out, maps it through raster::pixel_world's camera and flattens its curves), and
// the blend of the label's colour over what is there.  include/pvq.h, "the text", states the rule; what it assumes of the
// viewer's text pipeline is DESIGN.md 6i's table.
//
// All of it is f32, FMA contraction off on both sides; `/` is IEEE f32.  A pixel's sum runs over the segments in list order, so
// the host face and the device carry the same bits.
#pragma once

#include "raster_math.hpp"

namespace pvq {
namespace text {

constexpr uint32_t MAX_LABELS = 64;
constexpr uint32_t MAX_CODEPOINTS = 8;          // of a label
constexpr float MAX_EM_PIXELS = 1024.0f;        // font_px * scale in output pixels
constexpr double FLATTEN_TOL = 1.0 / 64.0;      // a chord stays within this many output pixels of its curve
constexpr float LINE_HEIGHT = 1.2f;             // of font_px
constexpr uint32_t MAX_SEGMENTS = 1u << 16;     // of a label
constexpr uint32_t CHUNK = 256;                 // segments a workgroup of text_coverage stages in LDS at a time

// a directed chord of the outline, output pixel coordinates: pixel (i, j) is the square [i, i + 1] x [j, j + 1], y downwards
struct Segment {
    float x0, y0, x1, y1;
};
static_assert(sizeof(Segment) == 16, "one 16-byte load");

// The signed area between the segment and the line x = X, inside the pixel square at (X, Y): the integral over the pixel's y
// range of clamp(x(y) - X, 0, 1), positive where the segment runs towards larger y.  Piecewise linear after the cuts at x = X
// and x = X + 1, so each piece's mean is that of its ends.  A horizontal segment gives 0.
PVQ_HD float segment_area(const Segment& s, float X, float Y) {
    PVQ_FP_STRICT
    if (s.y0 == s.y1) return 0.0f;
    const bool down = s.y1 > s.y0;
    const float xa = down ? s.x0 : s.x1, ya = down ? s.y0 : s.y1;   // the end with the smaller y
    const float xb = down ? s.x1 : s.x0, yb = down ? s.y1 : s.y0;
    const float top = Y + 1.0f;
    const float ylo = ya > Y ? ya : Y, yhi = yb < top ? yb : top;
    if (!(ylo < yhi)) return 0.0f;
    const float slope = (xb - xa) / (yb - ya);
    const float xlo = ya >= Y ? xa : xa + (Y - ya) * slope;         // an end inside the rows keeps its own x
    const float xhi = yb <= top ? xb : xa + (top - ya) * slope;
    const float h = yhi - ylo;
    float ua = xlo - X, ub = xhi - X;
    if (ua > ub) {
        const float t = ua;
        ua = ub;
        ub = t;
    }
    float mean;                                                      // of clamp(u, 0, 1) along the piece
    if (ub <= 0.0f) return 0.0f;
    if (ua >= 1.0f) mean = 1.0f;
    else if (ua >= 0.0f && ub <= 1.0f) mean = 0.5f * (ua + ub);
    else {
        const float d = ub - ua;                                     // > 0: the piece crosses x = X or x = X + 1
        const float t0 = ua < 0.0f ? (0.0f - ua) / d : 0.0f;         // where it enters the column
        const float t1 = ub > 1.0f ? (1.0f - ua) / d : 1.0f;         // where it leaves it
        const float c0 = ua < 0.0f ? 0.0f : ua, c1 = ub > 1.0f ? 1.0f : ub;
        mean = (t1 - t0) * (0.5f * (c0 + c1)) + (1.0f - t1);
    }
    const float area = h * mean;
    return down ? area : -area;
}

// what the sum over a label's segments becomes: 0 .. 1 (a NaN, which finite segments cannot give, would become 0)
PVQ_HD float coverage_of(float sum) {
    const float a = fabsf(sum);
    return a < 1.0f ? (a > 0.0f ? a : 0.0f) : 1.0f;
}

// a label's colour (linear) at `coverage` over what is there; coverage exactly 0 leaves the pixel as it is
PVQ_HD void blend_label(const float linear_rgb[3], float coverage, float dst[4]) {
    const float src[4] = {linear_rgb[0], linear_rgb[1], linear_rgb[2], coverage};
    raster::blend(src, dst);
}

}  // namespace text
}  // namespace pvq
