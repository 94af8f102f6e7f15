// ASan / UBSan driver for the readout stage's host face (test infrastructure; built and run by tests/test_sanitize_readout.py, CPU
// only).  It makes a font of the stage's 24 codepoints from outline arrays (rectangles with left bearings and a descender, and one
// contour of off-curve points only, so that the flattening runs), then for a set of image sizes and UI scales lays the atlas out,
// covers it and draws every value of a list — the colour edges, -0, the clamp, values far beyond it, NaN and the infinities — into
// exactly sized pictures.  Every changed pixel must lie in a 16 x 16 tile of the grid the device stage would launch
// (ReadoutPlan::tx0 .. ty1), so a draw outside that grid, a read outside the atlas or the picture, or an out-of-range
// float-to-integer conversion aborts the run.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "readout_host.hpp"

using namespace pvq;

static std::unique_ptr<TextFont> make_font(float advance_scale, uint32_t upem) {
    std::vector<uint32_t> cps, n_contours, ends, n_points;
    std::vector<float> advances, points;
    std::vector<uint8_t> on;
    for (uint32_t g = 0; g < readout::N_GLYPHS; ++g) {
        const uint32_t cp = readout::codepoint_of(g);
        cps.push_back(cp);
        advances.push_back((6.0f + 0.5f * g) * advance_scale);
        if (cp == ' ') {
            n_contours.push_back(0);
            n_points.push_back(0);
            continue;
        }
        const float x0 = g % 4 == 0 ? -1.5f : 0.25f * (g % 4), y0 = cp == 'g' ? -2.5f : 0.5f * (g % 2), w = 1.0f + 0.75f * (g % 3), h = 3.75f + g % 7;
        n_contours.push_back(1);
        n_points.push_back(4);
        ends.push_back(3);
        const float quad[8] = {x0, y0, x0, y0 + h, x0 + w, y0 + h, x0 + w, y0};
        points.insert(points.end(), quad, quad + 8);
        const bool curved = g % 5 == 0;   // off-curve points only: every on-curve point is implied
        for (int k = 0; k < 4; ++k) on.push_back(curved ? 0 : 1);
    }
    std::unique_ptr<TextFont> font;
    std::string err;
    if (TextFont::from_outlines(readout::N_GLYPHS, cps.data(), advances.data(), n_contours.data(), ends.data(), n_points.data(), points.data(),
                                on.data(), upem, 48.0f, -16.0f, font, err) != PVQ_OK) {
        std::printf("font: %s\n", err.c_str());
        return nullptr;
    }
    return font;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const float values[] = {0.0f, -0.4f, 0.5f, 9.5f, 10.5f, 20.5f, 30.5f, -99.5f, 999.0f, -1000.0f, 1e7f, 2147483520.0f, 3e9f, -3e9f, 3.4e38f, -3.4e38f,
                            std::numeric_limits<float>::denorm_min(), std::nanf(""), -std::nanf(""), inf, -inf};
    struct Case {
        uint32_t W, H;
        float scale, advance_scale;
        uint32_t upem;
    };
    const Case cases[] = {{301, 173, 4.0f, 1.0f, 64},  {64, 64, 4.0f, 1.0f, 64},  {160, 90, 0.5f, 1.0f, 64}, {1, 1, 0.0f, 1.0f, 64},   {4096, 1, 1.0f, 1.0f, 64},
                          {1, 257, 2.0f, 1.0f, 64},    {50, 50, 0.0f, 1.0f, 64},  {24, 8, 0.25f, 1.0f, 64},  {33, 17, 64.0f, 1.0f, 64}, {45, 29, 1.3f, 1.0f, 1000},
                          {45, 29, 1.0f, 900.0f, 16},  {45, 29, 1e-3f, 1.0f, 64}};
    size_t drawn_total = 0;
    for (const Case& c : cases) {
        std::unique_ptr<TextFont> font = make_font(c.advance_scale, c.upem);
        if (!font) return 1;
        ReadoutPlan plan;
        std::string err;
        const pvq_status st = readout_plan("sanitize", *font, c.W, c.H, c.scale, plan, err);
        if (st != PVQ_OK) {
            std::printf("plan %u x %u at %g: %s\n", c.W, c.H, c.scale, err.c_str());
            return 1;
        }
        readout_cover(plan);
        const size_t n = static_cast<size_t>(c.W) * c.H * 4;
        for (float v : values) {
            std::unique_ptr<float[]> img(new float[n]), before(new float[n]);   // exactly sized: no slack behind the last pixel
            for (size_t k = 0; k < n; ++k) before[k] = img[k] = 0.25f + 0.5f * static_cast<float>(k % 7) / 7.0f;
            ReadoutRow row;
            readout_row(plan, v, row);
            if (row.n_slots < readout::N_PREFIX + 3 || row.n_slots > readout::MAX_SLOTS) {
                std::printf("slots %u for %g\n", row.n_slots, v);
                return 1;
            }
            readout_frame(plan, v, img.get());
            for (uint32_t j = 0; j < c.H; ++j)
                for (uint32_t i = 0; i < c.W; ++i) {
                    const size_t at = (static_cast<size_t>(j) * c.W + i) * 4;
                    if (std::memcmp(&img[at], &before[at], 16) == 0) continue;
                    ++drawn_total;
                    const uint32_t tx = i / 16, ty = j / 16;
                    if (!plan.any || tx < plan.tx0 || tx > plan.tx1 || ty < plan.ty0 || ty > plan.ty1) {
                        std::printf("%u x %u at %g, value %g: pixel (%u, %u) is drawn outside the device's grid\n", c.W, c.H, c.scale, v, i, j);
                        return 1;
                    }
                }
        }
    }
    // the checks refuse, and leave a text
    std::unique_ptr<TextFont> font = make_font(1.0f, 64);
    ReadoutPlan plan;
    std::string err;
    const float bad_scales[] = {-1.0f, std::nanf(""), inf, 64.5f};
    for (float s : bad_scales)
        if (readout_plan("sanitize", *font, 8, 8, s, plan, err) != PVQ_ERR_INVALID_ARG || err.empty()) return 1;
    if (readout_plan("sanitize", *font, 0, 8, 0.0f, plan, err) != PVQ_ERR_INVALID_ARG || readout_plan("sanitize", *font, 8, 4097, 0.0f, plan, err) != PVQ_ERR_INVALID_ARG) return 1;
    if (drawn_total == 0) return 1;
    std::printf("SANITIZE_READOUT_OK %zu pixels drawn\n", drawn_total);
    return 0;
}
