// overlay_host.cpp — see overlay_host.hpp.  Built with -ffp-contract=off.
#include "overlay_host.hpp"

#include <algorithm>
#include <cmath>

namespace pvq {

namespace {
// pitchvis_colors/src/lib.rs:19-36
const float DEFAULT_COLORS[12][3] = {
    {0.85f, 0.36f, 0.36f}, {0.01f, 0.52f, 0.71f}, {0.97f, 0.76f, 0.05f}, {0.45f, 0.34f, 0.63f}, {0.47f, 0.77f, 0.22f}, {0.78f, 0.32f, 0.52f},
    {0.00f, 0.64f, 0.56f}, {0.95f, 0.54f, 0.23f}, {0.30f, 0.37f, 0.64f}, {1.00f, 0.96f, 0.03f}, {0.57f, 0.30f, 0.55f}, {0.12f, 0.71f, 0.34f},
};

// first and last of the W columns (or H rows) that the span lo .. hi of pixel coordinates can touch, widened by a pixel and the
// slack; false: none.  A span that is not a number takes every column.
bool span(double lo, double hi, uint32_t n, uint32_t& first, uint32_t& last) {
    double a = std::floor(lo) - 1.0, b = std::ceil(hi) + 1.0;
    if (!(a <= b)) {
        a = 0.0;
        b = n - 1.0;
    }
    if (b < 0.0 || a > n - 1.0) return false;
    first = static_cast<uint32_t>(std::max(a, 0.0));
    last = static_cast<uint32_t>(std::min(b, n - 1.0));
    return true;
}
}  // namespace

bool overlay_args_ok(const char* who, uint32_t history_rows, float ui_scale, const float* quad, std::string& err) {
    if (history_rows != 0 && (history_rows < overlay::MIN_HISTORY || history_rows > overlay::MAX_HISTORY)) {
        err = std::string(who) + ": history_rows is 0 (the viewer's 200) or 2 .. 4096";
        return false;
    }
    if (!(ui_scale >= 0.0f) || !raster::finite_f(ui_scale)) {
        err = std::string(who) + ": ui_scale is 0 (meaning 1) or positive and finite";
        return false;
    }
    if (quad && !(raster::finite_f(quad[0]) && raster::finite_f(quad[1]) && raster::finite_f(quad[2]) && raster::finite_f(quad[3]) && quad[2] > 0.0f &&
                  quad[3] > 0.0f)) {
        err = std::string(who) + ": the quad is (cx, cy, ex, ey), finite, with positive extents";
        return false;
    }
    return true;
}

void overlay_tables(const float* colors, overlay::Tables& out) {
    const float(*pal)[3] = colors ? reinterpret_cast<const float(*)[3]>(colors) : DEFAULT_COLORS;
    for (uint32_t b = 0; b < 256; ++b) {
        out.alpha[b] = static_cast<float>(b) / 255.0f;
        out.linear[b] = scene::srgb_to_linear(out.alpha[b]);
    }
    for (uint32_t pc = 0; pc < overlay::BOXES; ++pc)
        for (int c = 0; c < 3; ++c) out.box[pc][c] = scene::srgb_to_linear(pal[pc][c]);
}

void OverlayState::push(const uint8_t* row_rgba) {
    const size_t row = static_cast<size_t>(n_bins_) * 4;
    std::copy(row_rgba, row_rgba + row, texture_.begin() + (h_ - 1u - write_index_) * row);
    const uint32_t next = (write_index_ + 1u) % h_;
    std::fill_n(texture_.begin() + (h_ - 1u - next) * row, row, uint8_t{0});
    write_index_ = next;
}

void overlay_frame(const OverlayState* state, uint32_t W, uint32_t H, float vh, float ui_scale, const float* quad, const float* chroma12,
                   const overlay::Tables& tables, float* image) {
    float q[4] = {0.0f, 0.0f, 1.0f, 1.0f};
    uint32_t n = 0, h = 0;
    float scroll = 0.0f;
    if (state) {
        n = state->n_bins();
        h = state->history_rows();
        scroll = overlay::scroll_of(state->write_index(), h);
        if (quad) std::copy(quad, quad + 4, q);
        else overlay::reference_quad(n, h, q);
    }
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            float* dst = image + 4 * (static_cast<size_t>(j) * W + i);
            if (state) {
                float wx, wy;
                raster::pixel_world(i, j, W, H, vh, wx, wy);
                uint32_t tx, ty;
                if (overlay::quad_texel(q, n, h, scroll, wx, wy, tx, ty)) {
                    const uint8_t* t = state->texture() + 4 * (static_cast<size_t>(ty) * n + tx);
                    const uint32_t texel = t[0] | static_cast<uint32_t>(t[1]) << 8 | static_cast<uint32_t>(t[2]) << 16 | static_cast<uint32_t>(t[3]) << 24;
                    if (overlay::texel_draws(texel)) overlay::blend_texel(tables.linear, tables.alpha, texel, dst);
                }
            }
            if (chroma12) {
                const uint32_t pc = overlay::box_at(i, j, H, ui_scale);
                if (pc < overlay::BOXES && overlay::strength_draws(chroma12[pc])) overlay::blend_box(tables.box[pc], chroma12[pc], dst);
            }
        }
}

std::vector<uint32_t> overlay_tiles(uint32_t W, uint32_t H, float vh, float ui_scale, const float quad[4]) {
    constexpr uint32_t TILE = 16;
    const uint32_t tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
    std::vector<uint32_t> flags(static_cast<size_t>(tiles_x) * tiles_y, 0u);
    const auto mark = [&](uint32_t c0, uint32_t c1, uint32_t r0, uint32_t r1, uint32_t flag) {
        for (uint32_t ty = r0 / TILE; ty <= r1 / TILE; ++ty)
            for (uint32_t tx = c0 / TILE; tx <= c1 / TILE; ++tx) flags[static_cast<size_t>(ty) * tiles_x + tx] |= flag;
    };
    uint32_t c0, c1, r0, r1;
    if (quad) {
        // pixel_world's column of a world x is x / s + W / 2 - 1 / 2, its row H / 2 - 1 / 2 - y / s; the slack covers the rounding of
        // wx - cx, wy - cy and the two divisions (2^-22 relative, as raster::pixel_box)
        const double s = static_cast<double>(vh / static_cast<float>(H));
        const double cx = quad[0], cy = quad[1];
        const double slack = 2.4e-7 * (std::fabs(cx) + std::fabs(cy) + s * (W + H));
        const double hx = 0.5 * quad[2] * (1.0 + 1e-6) + slack, hy = 0.5 * quad[3] * (1.0 + 1e-6) + slack;
        if (span((cx - hx) / s + 0.5 * W - 0.5, (cx + hx) / s + 0.5 * W - 0.5, W, c0, c1) &&
            span(0.5 * H - 0.5 - (cy + hy) / s, 0.5 * H - 0.5 - (cy - hy) / s, H, r0, r1))
            mark(c0, c1, r0, r1, QUAD_TILE);
    }
    {
        const double s = ui_scale;
        const double left = overlay::BOX_LEFT * s, right = (overlay::BOX_LEFT + overlay::BOX_PITCH * (overlay::BOXES - 1) + overlay::BOX_SIDE) * s;
        const double top = H - (overlay::BOX_BOTTOM + overlay::BOX_SIDE) * s, bottom = H - overlay::BOX_BOTTOM * s;
        if (span(left - 0.5, right - 0.5, W, c0, c1) && span(top - 0.5, bottom - 0.5, H, r0, r1)) mark(c0, c1, r0, r1, BOX_TILE);
    }
    std::vector<uint32_t> out;
    for (size_t t = 0; t < flags.size(); ++t)
        if (flags[t]) out.push_back(static_cast<uint32_t>(t) | flags[t]);
    return out;
}

}  // namespace pvq
