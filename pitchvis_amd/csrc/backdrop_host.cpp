// backdrop_host.cpp — see backdrop_host.hpp.  Built with -ffp-contract=off.
#include "backdrop_host.hpp"

#include <algorithm>

namespace pvq {

namespace {
// one triangle of placed vertices over the image; samples == 4: over the four sample planes image [4][H][W][4]
void draw(const float v[6], const float rgba[4], uint32_t W, uint32_t H, float vh, float* image, uint32_t samples) {
    backdrop::Tri t;
    if (!backdrop::make_tri(v, rgba, W, H, vh, t)) return;
    if (samples == 1u) {
        for (uint32_t j = t.box_y & 0xFFFFu; j <= t.box_y >> 16; ++j)
            for (uint32_t i = t.box_x & 0xFFFFu; i <= t.box_x >> 16; ++i) {
                float wx, wy;
                raster::pixel_world(i, j, W, H, vh, wx, wy);
                if (backdrop::covers(t, wx, wy)) raster::blend(t.rgba, image + 4 * (static_cast<size_t>(j) * W + i));
            }
        return;
    }
    const size_t plane = 4 * static_cast<size_t>(W) * H;
    for (uint32_t j = t.box_y & 0xFFFFu; j <= t.box_y >> 16; ++j)
        for (uint32_t i = t.box_x & 0xFFFFu; i <= t.box_x >> 16; ++i)
            for (uint32_t k = 0; k < samples; ++k) {
                float fx, fy, wx, wy;
                backdrop::sample_fraction(samples, k, fx, fy);
                backdrop::sample_world(i, j, W, H, vh, fx, fy, wx, wy);
                if (backdrop::covers(t, wx, wy)) raster::blend(t.rgba, image + k * plane + 4 * (static_cast<size_t>(j) * W + i));
            }
}

// The picture a multisampled draw works on.  samples == 1: the caller's image itself.  samples == 4: four planes, every sample
// starting from its pixel of `image`; finish() resolves them back into it.
struct Target {
    Target(float* image, uint32_t W, uint32_t H, uint32_t samples) : image_(image), px_(static_cast<size_t>(W) * H), samples_(samples) {
        if (samples_ == 1u) return;
        planes_.resize(samples_ * 4 * px_);
        for (uint32_t k = 0; k < samples_; ++k) std::copy(image_, image_ + 4 * px_, planes_.data() + k * 4 * px_);
    }
    float* data() { return samples_ == 1u ? image_ : planes_.data(); }
    void finish() {
        if (samples_ == 1u) return;
        const float *s0 = planes_.data(), *s1 = s0 + 4 * px_, *s2 = s1 + 4 * px_, *s3 = s2 + 4 * px_;
        for (size_t c = 0; c < 4 * px_; ++c) image_[c] = backdrop::resolve4(s0[c], s1[c], s2[c], s3[c]);
    }
    float* image_;
    size_t px_;
    uint32_t samples_;
    std::vector<float> planes_;
};

// a mesh of quads or discs as the panels stage leaves it: pos [vertices][3], rgba [vertices][4]; a triangle takes the colour of
// its quad's first vertex or its disc's centre
void draw_panel(bool discs, uint32_t n_triangles, const float* pos, const float* rgba, const float* transform, uint32_t W, uint32_t H,
                float vh, float* image, uint32_t samples) {
    for (uint32_t t = 0; t < n_triangles; ++t) {
        uint32_t a, b, c, base;
        if (discs) backdrop::disc_triangle(t, a, b, c, base);
        else backdrop::quad_triangle(t, a, b, c, base);
        float v[6];
        backdrop::place(transform, pos[3 * a], pos[3 * a + 1], v[0], v[1]);
        backdrop::place(transform, pos[3 * b], pos[3 * b + 1], v[2], v[3]);
        backdrop::place(transform, pos[3 * c], pos[3 * c + 1], v[4], v[5]);
        draw(v, rgba + 4 * base, W, H, vh, image, samples);
    }
}

// static quads [n][4][2], the first n_quads of them, in one colour
void draw_static(const std::vector<float>& quads, uint32_t n_quads, const float rgba[4], uint32_t W, uint32_t H, float vh, float* image,
                 uint32_t samples) {
    for (uint32_t t = 0; t < 2u * n_quads; ++t) {
        uint32_t a, b, c, base;
        backdrop::quad_triangle(t, a, b, c, base);
        const float v[6] = {quads[2 * a], quads[2 * a + 1], quads[2 * b], quads[2 * b + 1], quads[2 * c], quads[2 * c + 1]};
        draw(v, rgba, W, H, vh, image, samples);
    }
}
}  // namespace

std::vector<float> backdrop_geometry(uint32_t octaves, int what) {
    const uint32_t n = backdrop::geometry_count(octaves, what);
    std::vector<float> out(static_cast<size_t>(n) * 8);
    for (uint32_t i = 0; i < n; ++i) backdrop::geometry_quad(octaves, what, i, out.data() + 8 * static_cast<size_t>(i));
    return out;
}

void backdrop_draw_mesh(uint32_t W, uint32_t H, float viewport_height, size_t n_triangles, const float* pos, const float* rgba,
                        const float* transform, float* image_inout, uint32_t samples) {
    Target target(image_inout, W, H, samples);
    for (size_t t = 0; t < n_triangles; ++t) {
        float v[6];
        for (int k = 0; k < 3; ++k) backdrop::place(transform, pos[6 * t + 2 * k], pos[6 * t + 2 * k + 1], v[2 * k], v[2 * k + 1]);
        draw(v, rgba + 4 * t, W, H, viewport_height, target.data(), samples);
    }
    target.finish();
}

void backdrop_frame(uint32_t octaves, uint32_t buckets_per_octave, uint32_t W, uint32_t H, float viewport_height, int visuals_mode,
                    uint32_t bass_lit, const float* bass_rgba, const pvq_backdrop_panels* panels, const float* background,
                    float* image_out, uint32_t samples) {
    const size_t px_count = static_cast<size_t>(W) * H;
    const float vh = viewport_height;
    if (background) {
        std::copy(background, background + 4 * px_count, image_out);
    } else {
        float clear[4];
        raster::clear_color(visuals_mode, clear);
        for (size_t i = 0; i < px_count; ++i) std::copy(clear, clear + 4, image_out + 4 * i);
    }
    Target target(image_out, W, H, samples);   // every sample starts from layer 0's pixel
    float* const image = target.data();
    const bool galaxy = visuals_mode == scene::GALAXY;
    if (!galaxy) {   // update.rs:888-895
        float gray[4];
        backdrop::net_color(gray);
        for (int what : {backdrop::NET_SPIRAL, backdrop::NET_RAYS})
            draw_static(backdrop_geometry(octaves, what), backdrop::geometry_count(octaves, what), gray, W, H, vh, image, samples);
    }
    if (panels) {
        const uint32_t quads = octaves * buckets_per_octave - 1u;
        if (panels->line_pos) draw_panel(false, 2u * quads, panels->line_pos, panels->line_rgba, panels->spectrum_transform, W, H, vh, image, samples);
        if (panels->disc_pos)
            draw_panel(true, panels::DISC_SEGMENTS * panels->n_peaks, panels->disc_pos, panels->disc_rgba, panels->spectrum_transform, W, H, vh,
                       image, samples);
        if (panels->graph_pos)
            draw_panel(false, 2u * (panels->graph_capacity - 1u), panels->graph_pos, panels->graph_rgba, panels->graph_transform, W, H, vh,
                       image, samples);
        if (panels->hist_pos) draw_panel(false, 2u * quads, panels->hist_pos, panels->hist_rgba, panels->histogram_transform, W, H, vh, image, samples);
    }
    if (!galaxy && bass_lit && bass_rgba) {
        const uint32_t n = backdrop::geometry_count(octaves, backdrop::BASS);
        float color[4];
        backdrop::bass_color(bass_rgba, color);
        draw_static(backdrop_geometry(octaves, backdrop::BASS), std::min(bass_lit, n), color, W, H, vh, image, samples);
    }
    target.finish();
}

}  // namespace pvq
