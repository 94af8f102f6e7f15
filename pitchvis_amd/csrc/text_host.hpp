// text_host.hpp — the pitch-name labels (setup.rs:386-416) on the host: a font as TrueType outlines and advances, the layout of a
// label, its outline as directed line segments in output pixels, and the one-frame face and second reference of TextBatch
// (text_batch.hpp).  The coverage arithmetic is text_math.hpp's on both.  The product embeds no font: the caller brings one, as
// TrueType bytes or as outline arrays.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pvq.h"
#include "text_math.hpp"

namespace pvq {

// A glyph as TrueType keeps it: contours of on- and off-curve points in font units, y upwards; an implied on-curve point lies
// between two consecutive off-curve points.
struct TextGlyph {
    float advance = 0.0f;
    std::vector<uint32_t> contour_ends;   // index of each contour's last point, ascending
    std::vector<float> points;            // [n][2]
    std::vector<uint8_t> on_curve;        // [n]
};

class TextFont {
   public:
    // head, maxp, hhea, hmtx and cmap (format 12, else format 4) are read and checked here; loca and glyf when a glyph is asked
    // for.  Bad bytes: PVQ_ERR_INVALID_ARG and a text that names the table.  kern and GPOS are ignored, hinting is never run.
    static pvq_status from_ttf(const uint8_t* bytes, size_t n_bytes, std::unique_ptr<TextFont>& out, std::string& err);
    // contour_ends holds, glyph after glyph, n_contours[g] indices into the glyph's own n_points[g] points
    static pvq_status from_outlines(uint32_t n_glyphs, const uint32_t* codepoints, const float* advances, const uint32_t* n_contours,
                                    const uint32_t* contour_ends, const uint32_t* n_points, const float* points, const uint8_t* on_curve,
                                    uint32_t units_per_em, float ascent, float descent, std::unique_ptr<TextFont>& out, std::string& err);
    // PVQ_ERR_INVALID_ARG: the font lacks the codepoint, or its bytes are bad; PVQ_ERR_UNSUPPORTED: a composite glyph, or a font
    // without glyf outlines (CFF)
    pvq_status glyph(uint32_t codepoint, const TextGlyph*& out, std::string& err);
    uint32_t units_per_em() const { return upem_; }
    float ascent() const { return ascent_; }
    float descent() const { return descent_; }

   private:
    TextFont() = default;
    pvq_status read_glyph(uint32_t codepoint, TextGlyph& g, std::string& err) const;
    bool glyph_index(uint32_t codepoint, uint32_t& gid) const;
    uint32_t upem_ = 0;
    float ascent_ = 0.0f, descent_ = 0.0f;
    std::map<uint32_t, TextGlyph> glyphs_;   // from_outlines: all of them; from_ttf: those asked for so far
    // from_ttf only: a copy of the file and where its tables lie, every range checked against the copy
    std::vector<uint8_t> bytes_;
    struct Table {
        size_t at = 0, len = 0;
    };
    Table hmtx_, cmap_sub_, loca_, glyf_;
    uint32_t n_glyphs_ = 0, n_hmetrics_ = 0, cmap_format_ = 0;
    bool long_loca_ = false, from_bytes_ = false;
};

// One contour of a glyph (its points first .. last) as a closed polygon in output pixels: every point through `map` (font units, y
// upwards, to output pixels, doubles), implied on-curve points added, lines kept and each quadratic cut into chords within
// text::FLATTEN_TOL of it.  The readout stage (readout_host.cpp) flattens its atlas glyphs with it.  false: more chords than a
// label may have.
struct TextPoint {
    double x, y;
};
using TextMap = std::function<TextPoint(double gx, double gy)>;
bool text_contour_chords(const TextGlyph& g, uint32_t first, uint32_t last, const TextMap& map, std::vector<TextPoint>& poly);

// A label laid out and flattened for a W x H image.
struct TextLabelPlan {
    std::vector<text::Segment> segments;   // list order is the order of the sum; horizontal ones and those no pixel can see dropped
    bool on_image = false;                 // false: nothing of the label lies on the image, the box is not set
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;   // first and last pixel column and row the outline can touch
    float origin_x = 0.0f, baseline_y = 0.0f;  // the first glyph's origin, output pixels
    float linear_rgb[3] = {0.0f, 0.0f, 0.0f};
    uint32_t n_tiles() const { return on_image ? (x1 / 16 - x0 / 16 + 1) * (y1 / 16 - y0 / 16 + 1) : 0; }
};

// The checks on the labels (1 .. 64 of them; UTF-8 of 1 .. 8 codepoints the font has; finite numbers; positive font_px and scale;
// rgb in 0 .. 1; an em of at most 1024 output pixels), then the plans.  viewport_height > 0.  The status is the failing check's.
pvq_status text_plan(const char* who, TextFont& font, const pvq_text_label* labels, uint32_t n, uint32_t W, uint32_t H, float viewport_height,
                     std::vector<TextLabelPlan>& out, std::string& err);

// a label's coverage of pixel (i, j), which lies in its box
inline float text_coverage_at(const TextLabelPlan& p, uint32_t i, uint32_t j) {
    float sum = 0.0f;
    const float X = static_cast<float>(i), Y = static_cast<float>(j);
    for (const text::Segment& s : p.segments) sum += text::segment_area(s, X, Y);
    return text::coverage_of(sum);
}

// The labels over image_inout [H][W][4] in label order, and / or their coverages to coverage_out [n][H][W]; either may be null.
void text_frame(const std::vector<TextLabelPlan>& plans, uint32_t W, uint32_t H, float* image_inout, float* coverage_out);

// the reference's twelve labels (setup.rs:386-416); colors 12 RGB triples or null (pitchvis_colors::COLORS)
void text_pitch_labels(uint32_t octaves, const float* colors, pvq_text_label* out12);

}  // namespace pvq
