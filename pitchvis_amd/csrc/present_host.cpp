// present_host.cpp — see present_host.hpp.
#include "present_host.hpp"

#include <cstring>
#include <vector>

#include "stage_plan.hpp"

namespace pvq {

namespace {
struct HostTex {   // [h][w][4] floats; the fourth is not read
    const float* p;
    uint32_t w;
    void operator()(uint32_t x, uint32_t y, float rgb[3]) const {
        const float* t = p + 4 * (static_cast<size_t>(y) * w + x);
        rgb[0] = t[0];
        rgb[1] = t[1];
        rgb[2] = t[2];
    }
};
}  // namespace

bool present_settings_ok(const char* who, const present::Settings& s, std::string& err) {
    const float fields[5] = {s.low_frequency_boost, s.low_frequency_boost_curvature, s.high_pass_frequency, s.threshold, s.threshold_softness};
    for (float v : fields)
        if (!raster::finite_f(v)) {
            err = std::string(who) + ": every setting must be finite";
            return false;
        }
    if (!(s.high_pass_frequency > 0.0f)) {
        err = std::string(who) + ": high_pass_frequency must be positive";
        return false;
    }
    if (s.composite_mode != present::ENERGY_CONSERVING && s.composite_mode != present::ADDITIVE) {
        err = std::string(who) + ": unknown composite_mode";
        return false;
    }
    if (s.tonemapping != present::TONEMAP_NONE && s.tonemapping != present::TONEMAP_SOMEWHAT_BORING) {
        err = std::string(who) + ": unknown tonemapping";
        return false;
    }
    if (s.max_mip_dimension != 0 && (s.max_mip_dimension < present::MIN_MIP_DIMENSION || s.max_mip_dimension > present::MAX_MIP_DIMENSION)) {
        err = std::string(who) + ": max_mip_dimension is 0 (512) or 4 .. 4096";
        return false;
    }
    return true;
}

present::Settings present_resolved(const present::Settings& s) {
    present::Settings r = s;
    if (r.max_mip_dimension == 0) r.max_mip_dimension = present::DEFAULT_MIP_DIMENSION;
    return r;
}

bool present_plan(const char* who, uint32_t W, uint32_t H, uint32_t max_mip_dimension, PresentPlan& out, std::string& err) {
    if (!present::mip_chain(W, H, max_mip_dimension, out.mips)) {
        err = std::string(who) + ": unsupported: mip 0 of this picture would be wider than 16384 texels";
        return false;
    }
    out.texels = 0;
    for (uint32_t k = 0; k < present::MAX_MIPS; ++k) {
        out.offset[k] = out.texels;
        if (k < out.mips.n) out.texels += static_cast<size_t>(out.mips.w[k]) * out.mips.h[k];
    }
    return true;
}

size_t present_piece_rows(size_t n_rows, const PresentPlan& plan, size_t limit) { return stage_piece_frames(n_rows, 1, plan.texels * 16, limit); }

void present_blend_factors(const present::Settings& s, float intensity, uint32_t n_mips, float* out) {
    present::Factors f;
    present::blend_tables(s, n_mips, f);
    for (uint32_t k = 0; k < n_mips; ++k) out[k] = present::blend_factor(f, k, s.composite_mode, intensity);
}

void present_frame(const present::Settings& s, const PresentPlan& plan, uint32_t W, uint32_t H, const float* image, float intensity, uint8_t* out_rgba8, float* out_hdr) {
    const bool bloom = present::blooms(intensity);
    std::vector<float> chain;
    present::Factors f;
    if (bloom) {
        present::blend_tables(s, plan.mips.n, f);
        chain.assign(plan.texels * 4, 0.0f);
        const present::Mips& m = plan.mips;
        for (uint32_t k = 0; k < m.n; ++k) {   // down: the picture -> mip 0, then mip k - 1 -> mip k
            const HostTex src{k == 0 ? image : chain.data() + 4 * plan.offset[k - 1], k == 0 ? W : m.w[k - 1]};
            const uint32_t ws = k == 0 ? W : m.w[k - 1], hs = k == 0 ? H : m.h[k - 1];
            float* dst = chain.data() + 4 * plan.offset[k];
            for (uint32_t j = 0; j < m.h[k]; ++j)
                for (uint32_t i = 0; i < m.w[k]; ++i) {
                    const float u = present::pixel_uv(i, m.w[k]), v = present::pixel_uv(j, m.h[k]);
                    float* o = dst + 4 * (static_cast<size_t>(j) * m.w[k] + i);
                    if (k == 0) present::down_first(src, ws, hs, u, v, s.threshold, s.threshold_softness, o);
                    else present::down_plain(src, ws, hs, u, v, o);
                }
        }
        const float x = present::tent_x(W, H);
        for (uint32_t k = m.n - 1; k >= 1; --k) {   // up: mip k into mip k - 1
            const HostTex src{chain.data() + 4 * plan.offset[k], m.w[k]};
            float* dst = chain.data() + 4 * plan.offset[k - 1];
            const float b = present::blend_factor(f, k, s.composite_mode, intensity);
            for (uint32_t j = 0; j < m.h[k - 1]; ++j)
                for (uint32_t i = 0; i < m.w[k - 1]; ++i) {
                    float t[3];
                    present::tent(src, m.w[k], m.h[k], present::pixel_uv(i, m.w[k - 1]), present::pixel_uv(j, m.h[k - 1]), x, present::TENT, t);
                    present::composite(s.composite_mode, b, t, dst + 4 * (static_cast<size_t>(j) * m.w[k - 1] + i));
                }
        }
    }
    const float x = present::tent_x(W, H);
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const size_t at = 4 * (static_cast<size_t>(j) * W + i);
            float px[4] = {image[at], image[at + 1], image[at + 2], image[at + 3]};
            if (bloom) {
                float t[3];
                present::tent(HostTex{chain.data(), plan.mips.w[0]}, plan.mips.w[0], plan.mips.h[0], present::pixel_uv(i, W), present::pixel_uv(j, H), x,
                              present::TENT, t);
                present::composite(s.composite_mode, present::blend_factor(f, 0, s.composite_mode, intensity), t, px);
            }
            if (out_hdr) std::memcpy(out_hdr + at, px, sizeof(px));
            float shown[3];
            present::display(s.tonemapping, px, shown);
            const uint32_t bytes = present::encode(shown, px[3]);
            out_rgba8[at] = static_cast<uint8_t>(bytes);
            out_rgba8[at + 1] = static_cast<uint8_t>(bytes >> 8);
            out_rgba8[at + 2] = static_cast<uint8_t>(bytes >> 16);
            out_rgba8[at + 3] = static_cast<uint8_t>(bytes >> 24);
        }
}

}  // namespace pvq
