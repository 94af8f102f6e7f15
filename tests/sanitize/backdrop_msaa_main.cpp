// ASan / UBSan driver for the multisampled host face of the backdrop stage (test infrastructure; built and run by
// tests/test_sanitize_backdrop_msaa.py, CPU only).  Calls backdrop_draw_mesh and backdrop_frame of backdrop_host.cpp with samples = 4 and
// exactly sized buffers — the image, and inside the call the four sample planes — so a pixel box that reaches past the image, a sample
// plane indexed past its end or a float-to-integer conversion out of range aborts the run: a mesh whose boxes leave the image on
// every side, a 1 x 1 image, and a 4096-wide image of one row.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "backdrop_host.hpp"

using namespace pvq;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float frand() {   // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (float)((rng_state * 2685821657736338717ull) >> 40) / 16777216.0f;
}

static const float SPECIALS[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                                 -std::numeric_limits<float>::infinity(), 1e30f, -1e30f, 3.0e38f, 1e-30f, -0.0f, 0.0f};

// n values in [-span, span], every 17th a special
static std::vector<float> values(size_t n, float span) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = i % 17 == 16 ? SPECIALS[(i / 17) % 9] : (frand() * 2.0f - 1.0f) * span;
    return v;
}

static size_t check_image(const std::vector<float>& img, const char* what) {
    size_t odd = 0;
    for (float v : img) odd += std::isfinite(v) ? 0 : 1;
    if (odd) {
        std::printf("%s: %zu channels are not finite\n", what, odd);
        std::exit(1);
    }
    return img.size();
}

int main() {
    const uint32_t sizes[][2] = {{1, 1}, {4096, 1}, {33, 17}, {7, 5}};
    size_t channels = 0, moved = 0;
    for (const auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        for (float vh : {0.6f, 3.0f, 400.0f}) {
            const float hx = 0.5f * vh * static_cast<float>(W) / static_cast<float>(H), hy = 0.5f * vh;
            // triangles that straddle each side and each corner of the image, and one that holds it whole: their boxes leave the image
            std::vector<float> pos;
            for (int sx = -1; sx <= 1; ++sx)
                for (int sy = -1; sy <= 1; ++sy) {
                    const float cx = sx * hx, cy = sy * hy, r = 0.7f * (hx < hy ? hx : hy) + 0.4f * vh / static_cast<float>(H);
                    const float t[6] = {cx - r, cy - 0.8f * r, cx + r, cy - 0.6f * r, cx + 0.1f * r, cy + r};
                    pos.insert(pos.end(), t, t + 6);
                }
            const float whole[6] = {-5.0f * hx, -3.0f * hy, 5.0f * hx, -3.0f * hy, 0.0f, 7.0f * hy};
            pos.insert(pos.end(), whole, whole + 6);
            const std::vector<float> wild = values(150 * 6, vh * 2.0f);   // and random ones with NaN, infinities, 1e30
            pos.insert(pos.end(), wild.begin(), wild.end());
            const size_t n_tri = pos.size() / 6;
            std::vector<float> rgba(n_tri * 4);
            for (size_t i = 0; i < rgba.size(); ++i) rgba[i] = i % 41 == 40 ? SPECIALS[(i / 41) % 3] : frand();
            std::vector<float> img(static_cast<size_t>(W) * H * 4, 0.25f);
            const float t[4] = {0.1f * vh, -0.2f * vh, 1.5f, -0.75f};
            backdrop_draw_mesh(W, H, vh, n_tri, pos.data(), rgba.data(), nullptr, img.data(), 4);
            backdrop_draw_mesh(W, H, vh, n_tri, pos.data(), rgba.data(), t, img.data(), 4);
            backdrop_draw_mesh(W, H, vh, 0, nullptr, nullptr, nullptr, img.data(), 4);
            channels += check_image(img, "draw_mesh, four samples");
            for (float v : img) moved += v != 0.25f;
            // whole frames
            for (uint32_t octaves : {1u, 7u}) {
                const uint32_t bpo = 12, n = octaves * bpo, n_peaks = 5, capacity = 9;
                const std::vector<float> line_pos = values(4 * (n - 1) * 3, vh), hist_pos = values(4 * (n - 1) * 3, vh);
                const std::vector<float> disc_pos = values(n_peaks * 13 * 3, vh), graph_pos = values(4 * (capacity - 1) * 3, vh);
                std::vector<float> line_rgba(4 * (n - 1) * 4), hist_rgba(4 * (n - 1) * 4), disc_rgba(n_peaks * 13 * 4), graph_rgba(4 * (capacity - 1) * 4);
                for (auto* c : {&line_rgba, &hist_rgba, &disc_rgba, &graph_rgba})
                    for (float& v : *c) v = frand();
                pvq_backdrop_panels p{};
                p.line_pos = line_pos.data(); p.line_rgba = line_rgba.data();
                p.disc_pos = disc_pos.data(); p.disc_rgba = disc_rgba.data(); p.n_peaks = n_peaks;
                p.hist_pos = hist_pos.data(); p.hist_rgba = hist_rgba.data();
                p.graph_pos = graph_pos.data(); p.graph_rgba = graph_rgba.data(); p.graph_capacity = capacity;
                for (int i = 0; i < 4; ++i) {
                    p.spectrum_transform[i] = i < 2 ? 0.0f : 1.0f;
                    p.histogram_transform[i] = i == 3 ? -1.0f : (i == 2 ? 1.0f : 0.1f);
                    p.graph_transform[i] = i < 2 ? -0.3f * vh : 3.0f;
                }
                const float bass[4] = {0.9f, 0.4f, 0.2f, 0.8f};
                std::vector<float> bg(static_cast<size_t>(W) * H * 4, 0.5f), out(bg.size());
                for (int mode : {0, 3})
                    for (uint32_t lit : {0u, 100000u}) {
                        backdrop_frame(octaves, bpo, W, H, vh, mode, lit, bass, &p, nullptr, out.data(), 4);
                        channels += check_image(out, "frame, four samples");
                        backdrop_frame(octaves, bpo, W, H, vh, mode, lit, bass, nullptr, bg.data(), out.data(), 4);
                        channels += check_image(out, "frame over a background, four samples");
                    }
            }
        }
    }
    if (moved == 0) {
        std::printf("no mesh changed a pixel\n");
        return 1;
    }
    std::printf("SANITIZE_BACKDROP_MSAA_OK %zu channels, %zu moved\n", channels, moved);
    return 0;
}
