// ASan / UBSan driver for the overlay stage's host face (test infrastructure; built and run by tests/test_sanitize_overlay.py, CPU
// only).  Calls OverlayState, overlay_frame and overlay_tiles of overlay_host.cpp on the edge sizes of tests/test_overlay.py — one
// pixel, images that are no multiple of anything, 3 and 1024 bins, rings of 2 and 200 rows — with exactly sized buffers, so a texel
// index past the texture, a ring row past the ring or a float-to-integer conversion out of range aborts the run.  Quads far off,
// far larger and far smaller than the image, strengths that are NaN or infinite and every ui_scale a handle takes go through; and
// every pixel a frame changes must lie in a tile that overlay_tiles lists for its layer: the device stage launches over that list.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "overlay_host.hpp"

using namespace pvq;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned next_u32() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (unsigned)((rng_state * 2685821657736338717ull) >> 32);
}
static float frand() { return (float)(next_u32() >> 8) / 16777216.0f; }

int main() {
    overlay::Tables tables;
    overlay_tables(nullptr, tables);
    const uint32_t sizes[][2] = {{1, 1}, {7, 5}, {33, 17}, {129, 33}, {16, 16}, {240, 14}, {960, 56}};
    const uint32_t shapes[][2] = {{3, 2}, {24, 5}, {1024, 3}, {252, 200}};   // bins, ring rows
    const float scales[] = {1.0f, 0.25f, 1e-30f, 3.0e38f, 7.3f};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    size_t channels = 0, changed_pixels = 0;
    for (const auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const float vh = 3.0f;
        const float hx = 0.5f * vh * W / H;
        const float quads[][4] = {{0.0f, 0.0f, 2.0f * hx, vh},       {-7.0f, 6.0f, 12.0f, 9.5f},   {0.3f * hx, -0.4f, 0.7f * hx, 0.9f},
                                  {1e30f, -1e30f, 1.0f, 1.0f},       {0.0f, 0.0f, 3.0e38f, 3.0e38f}, {0.0f, 0.0f, 1e-30f, 1e-30f},
                                  {-hx, 0.5f * vh, 1e-3f, 1e-3f},    {3.0e38f, 3.0e38f, 3.0e38f, 1e-38f}};
        for (const auto& nh : shapes) {
            const uint32_t n = nh[0], h = nh[1];
            OverlayState st(n, h);
            std::vector<uint8_t> row(static_cast<size_t>(n) * 4);
            for (uint32_t f = 0; f < 2 * h + 3; f += (h > 50 && f > 3 && f + 4 < 2 * h ? 37 : 1)) {
                for (uint8_t& b : row) b = (uint8_t)(next_u32() >> 24);
                for (uint32_t k = 0; k < n; k += 5) row[4 * k + 3] = 0;
                st.push(row.data());
                if (st.write_index() >= h) return 1;
                const float chroma[12] = {frand(), 0.0f, 1.0f, nan, inf, -inf, -0.5f, frand(), 2.0f, 1e-30f, frand(), frand()};
                const auto& q = quads[f % 8];
                const float s = scales[f % 5];
                std::vector<float> img(static_cast<size_t>(W) * H * 4), before;
                for (float& v : img) v = frand();
                before = img;
                overlay_frame(&st, W, H, vh, s, f % 3 == 2 ? nullptr : q, f % 4 == 3 ? nullptr : chroma, tables, img.data());
                overlay_frame(nullptr, W, H, vh, s, nullptr, chroma, tables, img.data());
                float ref[4];
                overlay::reference_quad(n, h, ref);
                const std::vector<uint32_t> tiles = overlay_tiles(W, H, vh, s, f % 3 == 2 ? ref : q);
                const uint32_t tiles_x = (W + 15) / 16;
                std::vector<uint32_t> flags(static_cast<size_t>(tiles_x) * ((H + 15) / 16), 0u);
                for (uint32_t t : tiles) {
                    if ((t & TILE_MASK) >= flags.size() || !(t & (QUAD_TILE | BOX_TILE))) return 1;
                    flags[t & TILE_MASK] = t;
                }
                for (uint32_t j = 0; j < H; ++j)
                    for (uint32_t i = 0; i < W; ++i) {
                        const size_t at = 4 * (static_cast<size_t>(j) * W + i);
                        if (!std::memcmp(&img[at], &before[at], 16)) continue;
                        ++changed_pixels;
                        if (!flags[(j / 16) * tiles_x + i / 16]) {
                            std::printf("pixel (%u, %u) of %u x %u was drawn on outside the tile list\n", i, j, W, H);
                            return 1;
                        }
                    }
                channels += img.size();
            }
        }
    }
    if (changed_pixels == 0) return 1;
    std::printf("SANITIZE_OVERLAY_OK %zu channels, %zu pixels drawn on\n", channels, changed_pixels);
    return 0;
}
