// readout_host.hpp — the tuning-drift readout (pitchvis_viewer/src/app/common.rs:348-432) on the host: the glyph atlas of a font at a
// UI scale, the layout of a row's string, and the one-frame face and second reference of ReadoutBatch (readout_batch.hpp).  The
// arithmetic is readout_math.hpp's and text_math.hpp's on both; the outlines are mapped and flattened by text_host's
// text_contour_chords.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pvq.h"
#include "readout_math.hpp"
#include "text_host.hpp"

namespace pvq {

// What create makes of a font: the cells, the chords of every glyph (origin at column 0, baseline on row 0) and the per-handle
// constants.  `coverage` is filled by readout_cover (the host face) or left empty (the device computes its own).
struct ReadoutPlan {
    uint32_t width = 0, height = 0;
    float font_px = 0.0f;                          // F = 16 ui_scale
    float baseline = 0.0f;                         // b: the baseline's offset inside a line of 1.2 F
    readout::Cell cells[readout::N_GLYPHS] = {};
    float advance[readout::N_GLYPHS] = {};         // the cells' advances, for readout::pen_fold
    uint32_t first_segment[readout::N_GLYPHS] = {}, n_segments[readout::N_GLYPHS] = {};
    std::vector<text::Segment> segments;           // glyph after glyph, list order is the order of the sum; horizontal ones dropped
    std::vector<float> coverage;                   // the atlas: every cell's [h][w]
    size_t atlas_floats = 0;
    // the tiles (stage::TILE) that the widest admissible box and its glyph cells can meet: columns tx0 .. tx1, rows ty0 .. ty1;
    // any == false: nothing of any row's readout lies on the image
    bool any = false;
    uint32_t tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0;
};

// The checks (width and height 1 .. 4096; ui_scale 0, meaning 1, or positive and finite with F at most 1024; every codepoint in the
// font; an atlas of at most 256 MiB), then the plan.  The status is the failing check's.
pvq_status readout_plan(const char* who, TextFont& font, uint32_t W, uint32_t H, float ui_scale, ReadoutPlan& out, std::string& err);
// the atlas by the host face's sum: text::segment_area over a glyph's chords in list order, text::coverage_of
void readout_cover(ReadoutPlan& plan);

// a row's string laid out: the box, the slots' glyphs and placed cells, the value's colour
struct ReadoutRow {
    readout::Box box;
    float text_width = 0.0f, r = 0.0f;
    int32_t baseline_row = 0;
    uint32_t n_slots = 0;
    uint8_t glyph[readout::MAX_SLOTS] = {};
    int32_t origin_x[readout::MAX_SLOTS] = {};
    float value_srgb[3] = {}, value_linear[3] = {};
};
void readout_row(const ReadoutPlan& plan, float value, ReadoutRow& out);
// one picture [H][W][4] in place; the plan's atlas must have been covered
void readout_frame(const ReadoutPlan& plan, float value, float* image_inout);

}  // namespace pvq
