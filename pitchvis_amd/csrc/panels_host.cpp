// panels_host.cpp — see panels_host.hpp.  Built with -ffp-contract=off.
#include "panels_host.hpp"

#include <cmath>

#include "consumers_host.hpp"

namespace pvq {

namespace {
// pitchvis_colors/src/lib.rs:19-36
const float DEFAULT_COLORS[12][3] = {
    {0.85f, 0.36f, 0.36f}, {0.01f, 0.52f, 0.71f}, {0.97f, 0.76f, 0.05f}, {0.45f, 0.34f, 0.63f}, {0.47f, 0.77f, 0.22f}, {0.78f, 0.32f, 0.52f},
    {0.00f, 0.64f, 0.56f}, {0.95f, 0.54f, 0.23f}, {0.30f, 0.37f, 0.64f}, {1.00f, 0.96f, 0.03f}, {0.57f, 0.30f, 0.55f}, {0.12f, 0.71f, 0.34f},
};

void put_quad(const float q[12], float* pos) {
    for (int j = 0; j < 12; ++j) pos[j] = q[j];
}
void put_rgba(float r, float g, float b, float a, float* rgba, uint32_t vertices) {
    for (uint32_t v = 0; v < vertices; ++v) {
        rgba[4 * v] = r;
        rgba[4 * v + 1] = g;
        rgba[4 * v + 2] = b;
        rgba[4 * v + 3] = a;
    }
}
}  // namespace

void panel_color_table(uint32_t buckets_per_octave, const float* colors, float gray_level, float* rgb) {
    const float(*pal)[3] = colors ? reinterpret_cast<const float(*)[3]>(colors) : DEFAULT_COLORS;
    const float shift = static_cast<float>(buckets_per_octave - 3u * (buckets_per_octave / 12u));   // update.rs:564
    const float bpo_f = static_cast<float>(buckets_per_octave);
    for (uint32_t k = 0; k < buckets_per_octave; ++k)
        calculate_color(static_cast<uint16_t>(buckets_per_octave), std::fmod(static_cast<float>(k) + 0.5f + shift, bpo_f), pal, gray_level,
                        panels::SPECTRUM_EASING, rgb + 3 * k);
}

void panel_disc_table(float* cs) {
    for (uint32_t i = 0; i < panels::DISC_SEGMENTS; ++i) {
        const float angle = (static_cast<float>(i) / static_cast<float>(panels::DISC_SEGMENTS)) * panels::TAU_F;   // update.rs:447
        cs[2 * i] = scene::SceneMath::cos(angle);
        cs[2 * i + 1] = scene::SceneMath::sin(angle);
    }
}

void spectrum_mesh(uint32_t n_buckets, uint32_t buckets_per_octave, const float* x, const float* center, const float* size, uint32_t n_peaks,
                   const float* rgb_table, const float* cs, float* line_pos, float* line_rgba, float* disc_pos, float* disc_rgba) {
    if (line_pos || line_rgba) {
        float best = scene::F32_MIN;   // util::arg_max (util.rs:48-57): the first maximum, bin 0 when nothing exceeds f32::MIN
        uint32_t k_max = 0;
        for (uint32_t i = 0; i < n_buckets; ++i)
            if (x[i] > best) {
                best = x[i];
                k_max = i;
            }
        const float max_size = x[k_max];   // update.rs:512-513
        for (uint32_t i = 0; i + 1u < n_buckets; ++i) {
            if (line_pos) {
                float q[12];
                panels::spectrum_quad(i, x[i], x[i + 1u], q);
                put_quad(q, line_pos + 12 * static_cast<size_t>(i));
            }
            if (line_rgba) {
                const float* c = rgb_table + 3 * (i % buckets_per_octave);
                put_rgba(c[0], c[1], c[2], panels::spectrum_alpha(x[i], max_size), line_rgba + 16 * static_cast<size_t>(i), 4);
            }
        }
    }
    for (uint32_t p = 0; p < n_peaks && (disc_pos || disc_rgba); ++p) {   // update.rs:582-615
        float cx, cy;
        uint32_t at;
        panels::disc_of_peak(buckets_per_octave, center[p], size[p], cx, cy, at);
        if (disc_pos)
            for (uint32_t v = 0; v < panels::DISC_VERTICES; ++v)
                for (uint32_t k = 0; k < 3; ++k) disc_pos[(static_cast<size_t>(p) * panels::DISC_VERTICES + v) * 3 + k] = panels::disc_coordinate(cx, cy, cs, v, k);
        if (disc_rgba)
            put_rgba(rgb_table[3 * at], rgb_table[3 * at + 1], rgb_table[3 * at + 2], panels::DISC_ALPHA,
                     disc_rgba + static_cast<size_t>(p) * panels::DISC_VERTICES * 4, panels::DISC_VERTICES);
    }
}

void calmness_histogram_mesh(uint32_t n_buckets, const float* calmness, float* pos, float* rgba) {
    for (uint32_t i = 0; i + 1u < n_buckets; ++i) {
        if (pos) {
            float q[12];
            panels::histogram_quad(i, calmness[i], calmness[i + 1u], q);
            put_quad(q, pos + 12 * static_cast<size_t>(i));
        }
        if (rgba) {
            float r, g, b;
            panels::calmness_to_color(panels::histogram_class_value(calmness[i], calmness[i + 1u]), r, g, b);
            put_rgba(r, g, b, 1.0f, rgba + 16 * static_cast<size_t>(i), 4);
        }
    }
}

void CalmnessGraph::history(float* out) const {
    const uint32_t c = capacity();
    for (uint32_t i = 0; i < c; ++i) out[i] = values_[(write_index_ + i) % c];
}

void CalmnessGraph::mesh(float* pos, float* rgba) const {
    const uint32_t c = capacity();
    for (uint32_t i = 0; i + 1u < c; ++i) {
        const float h0 = values_[(write_index_ + i) % c], h1 = values_[(write_index_ + i + 1u) % c];
        if (pos) {
            float q[12];
            panels::graph_quad(i, c, h0, h1, q);
            put_quad(q, pos + 12 * static_cast<size_t>(i));
        }
        if (rgba) {
            float r, g, b;
            panels::calmness_to_color(h0, r, g, b);   // update.rs:680-682
            put_rgba(r, g, b, 1.0f, rgba + 16 * static_cast<size_t>(i), 4);
        }
    }
}

void panel_topology(uint32_t n_quads, uint32_t n_circles, uint32_t* indices, float* uvs) {
    float cs[2 * panels::DISC_SEGMENTS];
    panel_disc_table(cs);
    static const uint32_t QUAD[6] = {2, 1, 0, 2, 0, 3};
    static const float QUAD_UV[8] = {0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 1.0f};
    for (uint32_t q = 0; q < n_quads; ++q) {
        if (indices)
            for (int j = 0; j < 6; ++j) indices[6 * static_cast<size_t>(q) + j] = 4u * q + QUAD[j];
        if (uvs)
            for (int j = 0; j < 8; ++j) uvs[8 * static_cast<size_t>(q) + j] = QUAD_UV[j];
    }
    const size_t i0 = 6 * static_cast<size_t>(n_quads), v0 = 4 * static_cast<size_t>(n_quads);
    for (uint32_t c = 0; c < n_circles; ++c) {
        const uint32_t base = static_cast<uint32_t>(v0) + panels::DISC_VERTICES * c;
        if (indices)
            for (uint32_t i = 0; i < panels::DISC_SEGMENTS; ++i) {
                uint32_t* t = indices + i0 + 3 * (static_cast<size_t>(c) * panels::DISC_SEGMENTS + i);
                t[0] = base;
                t[1] = base + 1u + i;
                t[2] = base + 1u + (i + 1u) % panels::DISC_SEGMENTS;
            }
        if (uvs) {
            float* u = uvs + 2 * (v0 + static_cast<size_t>(c) * panels::DISC_VERTICES);
            u[0] = 0.5f;
            u[1] = 0.5f;
            for (uint32_t i = 0; i < panels::DISC_SEGMENTS; ++i) {
                u[2 + 2 * i] = 0.5f + 0.5f * cs[2 * i];
                u[3 + 2 * i] = 0.5f + 0.5f * cs[2 * i + 1];
            }
        }
    }
}

}  // namespace pvq
