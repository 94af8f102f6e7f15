// ASan / UBSan driver for the present stage's host face and host planning (test infrastructure; built and run by
// tests/test_sanitize_present.py, CPU only).  Calls present_frame of present_host.cpp on the edge sizes of tests/present_cases.py —
// one pixel, images that are no multiple of anything, mips one texel wide, 1 to 8 mips, a magnified picture — with exactly sized
// buffers, so a texel index past a mip, a mip past the chain or a float-to-integer conversion out of range aborts the run; pixels
// that are NaN, infinite, negative and huge and every kind of intensity go through.  It checks the planning the device stage
// shares: a chain's offsets, the cut of a call's rows into pieces (every row in exactly one piece, a piece within the limit
// wherever one row is), and that every texel a tile's taps can sample lies in the footprint the device would stage for it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "present_host.hpp"

using namespace pvq;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned next_u32() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (unsigned)((rng_state * 2685821657736338717ull) >> 32);
}
static float frand() { return (float)(next_u32() >> 8) / 16777216.0f; }

// a texture functor that records the range of indices sampled
struct Probe {
    mutable uint32_t x0 = ~0u, x1 = 0, y0 = ~0u, y1 = 0;
    uint32_t w, h;
    Probe(uint32_t w_, uint32_t h_) : w(w_), h(h_) {}
    void operator()(uint32_t x, uint32_t y, float rgb[3]) const {
        if (x >= w || y >= h) {
            std::printf("texel (%u, %u) outside a %u x %u texture\n", x, y, w, h);
            std::exit(1);
        }
        x0 = x < x0 ? x : x0;
        x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0;
        y1 = y > y1 ? y : y1;
        rgb[0] = rgb[1] = rgb[2] = 1.0f;
    }
};

// every tile of a pass: what its texels sample lies within present::footprint
static bool footprints_hold(uint32_t wt, uint32_t ht, uint32_t ws, uint32_t hs, bool down, float x, float y) {
    const float mx = down ? 2.0f : x * (float)ws, my = down ? 2.0f : y * (float)hs;
    for (uint32_t j0 = 0; j0 < ht; j0 += 16)
        for (uint32_t i0 = 0; i0 < wt; i0 += 16) {
            if (wt * ht > 4096 && (next_u32() & 7u)) continue;   // a sample of the tiles of a large level
            Probe p(ws, hs);
            for (uint32_t j = j0; j < j0 + 16 && j < ht; ++j)
                for (uint32_t i = i0; i < i0 + 16 && i < wt; ++i) {
                    float o[3];
                    if (down) present::down_plain(p, ws, hs, present::pixel_uv(i, wt), present::pixel_uv(j, ht), o);
                    else present::tent(p, ws, hs, present::pixel_uv(i, wt), present::pixel_uv(j, ht), x, y, o);
                }
            uint32_t lx, fw, ly, fh;
            present::footprint(i0, 16, wt, ws, mx, lx, fw);
            present::footprint(j0, 16, ht, hs, my, ly, fh);
            if (p.x0 < lx || p.x1 >= lx + fw || p.y0 < ly || p.y1 >= ly + fh || lx + fw > ws || ly + fh > hs) {
                std::printf("tile (%u, %u) of %u x %u over %u x %u samples %u..%u x %u..%u outside its footprint %u+%u x %u+%u\n", i0, j0, wt, ht,
                            ws, hs, p.x0, p.x1, p.y0, p.y1, lx, fw, ly, fh);
                return false;
            }
        }
    return true;
}

int main() {
    const uint32_t sizes[][3] = {{1, 1, 16},   {2, 3, 4},    {5, 4, 8},     {17, 9, 16},   {129, 33, 64}, {129, 33, 4},   {4, 130, 64},
                                 {64, 64, 64}, {64, 64, 8},  {33, 17, 512}, {1, 64, 4096}, {300, 7, 4},   {1280, 720, 512}, {16, 4096, 4096}};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float intensities[] = {0.5f, 1.0f, 0.0f, nan, inf, -1.0f, 1e-30f, 3.0e38f};
    size_t channels = 0, pieces_seen = 0;
    for (const auto& whd : sizes) {
        const uint32_t W = whd[0], H = whd[1], d = whd[2];
        PresentPlan plan;
        std::string err;
        if (!present_plan("sanitize", W, H, d, plan, err)) return 1;
        // the chain's layout
        size_t at = 0;
        for (uint32_t k = 0; k < plan.mips.n; ++k) {
            if (plan.offset[k] != at || plan.mips.w[k] == 0 || plan.mips.h[k] == 0) return 1;
            at += static_cast<size_t>(plan.mips.w[k]) * plan.mips.h[k];
        }
        if (at != plan.texels || plan.mips.n == 0 || plan.mips.n > present::MAX_MIPS) return 1;
        // the cut into pieces
        const size_t per_row = plan.texels * 16;
        const size_t limits[] = {1, per_row - 1, per_row, per_row + 1, 3 * per_row + per_row / 2, 7 * per_row, 1000 * per_row, ~size_t{0} / 2};
        for (size_t n_rows : {size_t{1}, size_t{7}, size_t{32}, size_t{0x7FFFFFFF}})
            for (size_t limit : limits) {
                const size_t piece = present_piece_rows(n_rows, plan, limit);
                if (piece < 1 || piece > n_rows) return 1;
                if (per_row <= limit && piece * per_row > limit) return 1;                        // a piece fits wherever one row does
                if (piece < n_rows && (piece + 1) * per_row <= limit) return 1;                   // and is as long as fits
                if (n_rows == 7 && limit == 3 * per_row + per_row / 2 && piece != 3) return 1;    // 3, 3 and 1
                if (limit < 2 * per_row && piece != 1) return 1;
                ++pieces_seen;
            }
        // the footprints the device stage would size
        const float x = present::tent_x(W, H);
        for (uint32_t k = 0; k < plan.mips.n; ++k) {
            const uint32_t ws = k == 0 ? W : plan.mips.w[k - 1], hs = k == 0 ? H : plan.mips.h[k - 1];
            if (!footprints_hold(plan.mips.w[k], plan.mips.h[k], ws, hs, true, 0.0f, 0.0f)) return 1;
            if (!footprints_hold(ws, hs, plan.mips.w[k], plan.mips.h[k], false, x, present::TENT)) return 1;
        }
        if (static_cast<size_t>(W) * H > 100000) continue;   // the planning alone for the large sizes
        std::vector<float> image(static_cast<size_t>(W) * H * 4), hdr(image.size());
        std::vector<uint8_t> bytes(image.size());
        unsigned trial = 0;
        for (float intensity : intensities) {
            for (float& v : image) {
                const unsigned pick = next_u32() % 64u;
                v = pick == 0 ? nan : pick == 1 ? inf : pick == 2 ? -inf : pick == 3 ? -5.0f : pick == 4 ? 3.0e38f : frand() * 8.0f;
            }
            present::Settings s = present::default_settings();
            s.max_mip_dimension = d;
            s.composite_mode = trial & 1 ? present::ENERGY_CONSERVING : present::ADDITIVE;
            s.tonemapping = trial & 2 ? present::TONEMAP_NONE : present::TONEMAP_SOMEWHAT_BORING;
            s.threshold = trial % 3 == 2 ? 0.0f : 0.17f;
            s.low_frequency_boost_curvature = trial & 4 ? 0.5f : 1.0f;
            if (!present_settings_ok("sanitize", s, err)) return 1;
            present_frame(s, plan, W, H, image.data(), intensity, bytes.data(), trial & 1 ? hdr.data() : nullptr);
            float factors[present::MAX_MIPS];
            present_blend_factors(s, intensity, plan.mips.n, factors);
            channels += image.size();
            ++trial;
            if (d == 512 && trial == 2) break;   // the magnified picture is the slow one
        }
    }
    std::printf("SANITIZE_PRESENT_OK %zu channels, %zu cuts\n", channels, pieces_seen);
    return 0;
}
