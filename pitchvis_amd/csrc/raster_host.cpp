// raster_host.cpp — see raster_host.hpp.  Built with -ffp-contract=off.
#include "raster_host.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace pvq {

void raster_shade(const float rgba[4], const float params[4], float u, float v, float out[4]) {
    const float xyzs[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    const float p3[3] = {params[0], params[2], params[3]};
    raster::Ball q;
    raster::make_ball(xyzs, rgba, p3, params[1], q);
    float px, py;
    const float r = raster::radius_of(u, v, px, py);
    raster::shade(q, u, v, px, py, r, out);
}

void raster_touch(uint32_t n_bins, const float* center, uint32_t n_peaks, float elapsed, float* time_inout) {
    for (uint32_t p = 0; p < n_peaks; ++p) {
        const uint32_t key = scene::sat_u32(truncf(center[p]));   // as scene::peak_record takes it
        if (key < n_bins) time_inout[key] = elapsed;
    }
}

void raster_frame(uint32_t n_bins, uint32_t W, uint32_t H, float viewport_height, int visuals_mode, const float* ball_xyzs,
                  const float* ball_rgba, const float* ball_params, const uint32_t* ball_visible, const float* ball_time,
                  const float* background, float* image_out) {
    const size_t px_count = static_cast<size_t>(W) * H;
    if (background) {
        std::copy(background, background + 4 * px_count, image_out);
    } else {
        float clear[4];
        raster::clear_color(visuals_mode, clear);
        for (size_t i = 0; i < px_count; ++i) std::copy(clear, clear + 4, image_out + 4 * i);
    }
    std::vector<std::pair<uint64_t, raster::Ball>> list;
    for (uint32_t bin = 0; bin < n_bins; ++bin) {
        const float* xyzs = ball_xyzs + 4 * bin;
        const bool vis = (ball_visible[bin / 32] >> (bin % 32)) & 1u;
        if (!raster::drawable(xyzs, ball_rgba + 4 * bin, ball_params + 3 * bin, ball_time[bin], vis)) continue;
        raster::Ball q;
        raster::make_ball(xyzs, ball_rgba + 4 * bin, ball_params + 3 * bin, ball_time[bin], q);
        if (!raster::pixel_box(q.x, q.y, q.side, W, H, viewport_height, q.box_x, q.box_y)) continue;
        list.emplace_back(raster::order_key(xyzs[2], bin), q);
    }
    std::sort(list.begin(), list.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (const auto& e : list) {
        const raster::Ball& q = e.second;
        for (uint32_t j = q.box_y & 0xFFFFu; j <= q.box_y >> 16; ++j)
            for (uint32_t i = q.box_x & 0xFFFFu; i <= q.box_x >> 16; ++i) {
                float wx, wy;
                raster::pixel_world(i, j, W, H, viewport_height, wx, wy);
                raster::compose_ball(q, wx, wy, image_out + 4 * (static_cast<size_t>(j) * W + i));
            }
    }
}

}  // namespace pvq
