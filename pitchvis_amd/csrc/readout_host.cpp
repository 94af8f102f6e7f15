// readout_host.cpp — see readout_host.hpp.  Built with -ffp-contract=off.
#include "readout_host.hpp"

#include <algorithm>
#include <cmath>

namespace pvq {

namespace {
constexpr size_t MAX_ATLAS_FLOATS = size_t{1} << 26;   // 256 MiB
constexpr int TILE = 16;                                // stage::TILE (stage_device.hpp is the device's)
}  // namespace

pvq_status readout_plan(const char* who, TextFont& font, uint32_t W, uint32_t H, float ui_scale, ReadoutPlan& out, std::string& err) {
    out = ReadoutPlan();
    const std::string tag(who);
    if (W == 0 || H == 0 || W > raster::MAX_IMAGE || H > raster::MAX_IMAGE) {
        err = tag + ": width and height are 1 .. 4096";
        return PVQ_ERR_INVALID_ARG;
    }
    const float scale = ui_scale == 0.0f ? 1.0f : ui_scale;
    const float F = readout::FONT_PX * scale;
    if (!raster::finite_f(scale) || !(scale > 0.0f) || !(F > 0.0f) || !(F <= text::MAX_EM_PIXELS)) {
        err = tag + ": ui_scale is 0 (meaning 1) or positive and finite, and the font size 16 ui_scale at most 1024 output pixels";
        return PVQ_ERR_INVALID_ARG;
    }
    out.width = W;
    out.height = H;
    out.font_px = F;
    const double k = static_cast<double>(F) / font.units_per_em();
    {   // the text stage's baseline inside a line of 1.2 F (text_host.cpp: text_plan)
        const double line = static_cast<double>(text::LINE_HEIGHT) * F, asc = font.ascent() * k, desc = font.descent() * k;
        out.baseline = static_cast<float>(0.5 * (line - (asc - desc)) + asc);
    }
    const TextMap map = [&](double gx, double gy) { return TextPoint{gx * k, -(gy * k)}; };   // origin at column 0, baseline on row 0
    std::vector<TextPoint> poly;
    double min_x0 = 0.0, max_x1 = 0.0, min_y0 = 0.0, max_y1 = 0.0, max_advance = 0.0;
    for (uint32_t g = 0; g < readout::N_GLYPHS; ++g) {
        const TextGlyph* glyph = nullptr;
        if (pvq_status st = font.glyph(readout::codepoint_of(g), glyph, err)) {
            err = tag + ": " + err;
            return st;
        }
        readout::Cell& cell = out.cells[g];
        cell.advance = static_cast<float>(glyph->advance * k);
        out.advance[g] = cell.advance;
        max_advance = std::max(max_advance, static_cast<double>(cell.advance));
        out.first_segment[g] = static_cast<uint32_t>(out.segments.size());
        double lo_x = 1e300, lo_y = 1e300, hi_x = -1e300, hi_y = -1e300;
        uint32_t first = 0, kept = 0;
        for (uint32_t e : glyph->contour_ends) {
            const bool fits = text_contour_chords(*glyph, first, e, map, poly);
            first = e + 1;
            if (!fits || kept + poly.size() > text::MAX_SEGMENTS + 1u) {
                err = tag + ": the outline of U+00" + "0123456789ABCDEF"[readout::codepoint_of(g) >> 4] + "0123456789ABCDEF"[readout::codepoint_of(g) & 15u] +
                      " takes more than 65536 line segments";
                return PVQ_ERR_INVALID_ARG;
            }
            for (size_t q = 0; q + 1 < poly.size(); ++q) {
                const text::Segment sg{static_cast<float>(poly[q].x), static_cast<float>(poly[q].y), static_cast<float>(poly[q + 1].x),
                                       static_cast<float>(poly[q + 1].y)};
                lo_x = std::min({lo_x, static_cast<double>(sg.x0), static_cast<double>(sg.x1)});
                hi_x = std::max({hi_x, static_cast<double>(sg.x0), static_cast<double>(sg.x1)});
                lo_y = std::min({lo_y, static_cast<double>(sg.y0), static_cast<double>(sg.y1)});
                hi_y = std::max({hi_y, static_cast<double>(sg.y0), static_cast<double>(sg.y1)});
                if (sg.y0 == sg.y1) continue;   // contributes nothing
                out.segments.push_back(sg);
                ++kept;
            }
        }
        out.n_segments[g] = kept;
        cell.offset = static_cast<uint32_t>(out.atlas_floats);
        if (!(lo_x < hi_x && lo_y < hi_y) || kept == 0) {   // no outline, or one without area: an empty cell
            out.segments.resize(out.first_segment[g]);
            out.n_segments[g] = 0;
            continue;
        }
        // the pixel box: every pixel square that the outline's bounding box meets with positive area
        const double x0 = std::floor(lo_x), y0 = std::floor(lo_y), w = std::ceil(hi_x) - x0, h = std::ceil(hi_y) - y0;
        if (w * h > static_cast<double>(MAX_ATLAS_FLOATS - out.atlas_floats)) {
            err = "unsupported: the glyph cells take more than an atlas of 256 MiB holds";
            return PVQ_ERR_UNSUPPORTED;
        }
        cell.x0 = static_cast<int32_t>(x0);
        cell.y0 = static_cast<int32_t>(y0);
        cell.w = static_cast<uint32_t>(w);
        cell.h = static_cast<uint32_t>(h);
        out.atlas_floats += static_cast<size_t>(cell.w) * cell.h;
        min_x0 = std::min(min_x0, x0);
        min_y0 = std::min(min_y0, y0);
        max_x1 = std::max(max_x1, x0 + w);
        max_y1 = std::max(max_y1, y0 + h);
    }
    // What any row can touch, with a pixel to spare on every side: the widest text is the prefix and eleven times the widest glyph.
    const readout::Box narrow = readout::box_of(W, H, 0.0f, F);
    const double widest = static_cast<double>(readout::MAX_SLOTS) * max_advance + 1.0;
    const double by = readout::baseline_row(narrow, out.baseline);
    const double slack = 2.0 + 4e-6 * widest;   // the f32 fold and xr - Wt + p_i round: 26 operations of relative error 2^-24 each
    const double lo_x = std::floor(narrow.xr - widest) + min_x0 - slack, hi_x = std::ceil(static_cast<double>(narrow.xr)) + max_x1 + slack;
    const double lo_y = std::min(std::floor(static_cast<double>(narrow.yt)), by + min_y0) - 1.0;
    const double hi_y = std::max(std::ceil(static_cast<double>(narrow.yb)), by + max_y1) + 1.0;
    if (hi_x > 0.0 && hi_y > 0.0 && lo_x < W && lo_y < H) {
        out.any = true;
        out.tx0 = static_cast<uint32_t>(std::max(lo_x, 0.0)) / TILE;
        out.ty0 = static_cast<uint32_t>(std::max(lo_y, 0.0)) / TILE;
        out.tx1 = static_cast<uint32_t>(std::min(hi_x, static_cast<double>(W)) - 1.0) / TILE;
        out.ty1 = static_cast<uint32_t>(std::min(hi_y, static_cast<double>(H)) - 1.0) / TILE;
    }
    return PVQ_OK;
}

void readout_cover(ReadoutPlan& plan) {
    plan.coverage.assign(plan.atlas_floats, 0.0f);
    for (uint32_t g = 0; g < readout::N_GLYPHS; ++g) {
        const readout::Cell& c = plan.cells[g];
        const text::Segment* segs = plan.segments.data() + plan.first_segment[g];
        for (uint32_t j = 0; j < c.h; ++j)
            for (uint32_t i = 0; i < c.w; ++i) {
                const float X = static_cast<float>(c.x0 + static_cast<int32_t>(i)), Y = static_cast<float>(c.y0 + static_cast<int32_t>(j));
                float sum = 0.0f;
                for (uint32_t s = 0; s < plan.n_segments[g]; ++s) sum += text::segment_area(segs[s], X, Y);
                plan.coverage[c.offset + static_cast<size_t>(j) * c.w + i] = text::coverage_of(sum);
            }
    }
}

void readout_row(const ReadoutPlan& plan, float value, ReadoutRow& out) {
    out = ReadoutRow();
    uint64_t text = 0;
    const uint32_t n = readout::N_PREFIX + readout::value_glyphs(value, text, out.r);
    out.n_slots = n;
    float p0;
    out.text_width = readout::pen_fold(plan.advance, text, n, 0, p0);
    out.box = readout::box_of(plan.width, plan.height, out.text_width, plan.font_px);
    out.baseline_row = static_cast<int32_t>(readout::baseline_row(out.box, plan.baseline));
    for (uint32_t i = 0; i < n; ++i) {
        float p;
        readout::pen_fold(plan.advance, text, n, i, p);
        out.glyph[i] = static_cast<uint8_t>(readout::slot_glyph(text, i));
        out.origin_x[i] = static_cast<int32_t>(readout::origin_column(out.box, p));
    }
    readout::value_srgb(out.r, out.value_srgb);
    for (int c = 0; c < 3; ++c) out.value_linear[c] = scene::srgb_to_linear(out.value_srgb[c]);
}

void readout_frame(const ReadoutPlan& plan, float value, float* image) {
    ReadoutRow row;
    readout_row(plan, value, row);
    const int64_t W = plan.width, H = plan.height;
    const auto clip = [](double v, int64_t hi) { return static_cast<int64_t>(std::min(std::max(v, 0.0), static_cast<double>(hi))); };
    // the box: every pixel whose centre lies in it, the candidates a pixel wider than it
    for (int64_t j = clip(std::floor(row.box.yt) - 1.0, H); j < clip(std::ceil(row.box.yb) + 1.0, H); ++j)
        for (int64_t i = clip(std::floor(row.box.xl) - 1.0, W); i < clip(std::ceil(row.box.xr) + 1.0, W); ++i)
            if (readout::in_box(row.box, static_cast<uint32_t>(i), static_cast<uint32_t>(j))) readout::blend_box(image + 4 * (j * W + i));
    const float white[3] = {1.0f, 1.0f, 1.0f};
    for (uint32_t s = 0; s < row.n_slots; ++s) {
        const readout::Cell& c = plan.cells[row.glyph[s]];
        const float* rgb = s < readout::N_PREFIX ? white : row.value_linear;
        const int64_t x0 = static_cast<int64_t>(row.origin_x[s]) + c.x0, y0 = static_cast<int64_t>(row.baseline_row) + c.y0;
        for (int64_t j = std::max<int64_t>(y0, 0); j < std::min<int64_t>(y0 + c.h, H); ++j)
            for (int64_t i = std::max<int64_t>(x0, 0); i < std::min<int64_t>(x0 + c.w, W); ++i) {
                const float cov = plan.coverage[c.offset + static_cast<size_t>(j - y0) * c.w + static_cast<size_t>(i - x0)];
                if (cov == 0.0f) continue;
                text::blend_label(rgb, cov, image + 4 * (j * W + i));
            }
    }
}

}  // namespace pvq
