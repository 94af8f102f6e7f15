// scene_host.cpp — see scene_host.hpp.  Built with -ffp-contract=off.
#include "scene_host.hpp"

#include <cmath>

#include "analysis_host.hpp"
#include "consumers_host.hpp"

namespace pvq {

namespace {
// pitchvis_colors/src/lib.rs:19-36
const float DEFAULT_COLORS[12][3] = {
    {0.85f, 0.36f, 0.36f}, {0.01f, 0.52f, 0.71f}, {0.97f, 0.76f, 0.05f}, {0.45f, 0.34f, 0.63f}, {0.47f, 0.77f, 0.22f}, {0.78f, 0.32f, 0.52f},
    {0.00f, 0.64f, 0.56f}, {0.95f, 0.54f, 0.23f}, {0.30f, 0.37f, 0.64f}, {1.00f, 0.96f, 0.03f}, {0.57f, 0.30f, 0.55f}, {0.12f, 0.71f, 0.34f},
};
}  // namespace

bool scene_settings(uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, int enable_bloom, const float* colors,
                    float gray_level, float easing_pow, scene::Settings& s) {
    if (visuals_mode < scene::FULL || visuals_mode > scene::GALAXY) return false;
    s.n_bins = octaves * buckets_per_octave;
    s.bpo = buckets_per_octave;
    const uint32_t pts = octaves * 72u < 168u ? octaves * 72u : 168u;   // setup.rs:134-136: take(HIGHEST_BASSNOTE * 6) of the 72-per-octave spiral
    s.n_segments = pts ? pts - 1u : 0u;                                 // tuple_windows
    s.mode = visuals_mode;
    s.enable_bloom = enable_bloom != 0;
    s.gray_level = gray_level;
    s.easing_pow = easing_pow;
    s.semitone_offset = static_cast<float>(buckets_per_octave - 3u * (buckets_per_octave / 12u));
    s.hide_radius = static_cast<float>(buckets_per_octave / 12u) * 0.23f;
    palette_lch(colors ? reinterpret_cast<const float(*)[3]>(colors) : DEFAULT_COLORS, s.lch);
    return true;
}

void scene_fade_table(uint32_t n_bins, uint64_t frame_time_ns, float* dropoff, float& z_step) {
    const float dt = Duration{frame_time_ns}.as_secs_f32();
    for (uint32_t idx = 0; idx < n_bins; ++idx) {
        const float per_30fps_frame = 0.85f - 0.15f * (static_cast<float>(idx) / static_cast<float>(n_bins));   // update.rs:157-158
        dropoff[idx] = scene::SceneMath::pow(per_30fps_frame, 30.0f * dt);   // update.rs:159 (the host's pow in double, rounded once: scene_math.hpp)
    }
    z_step = 0.001f * 30.0f * dt;   // update.rs:172
}

void scene_initial(const scene::Settings& s, SceneBalls& b, float bass_rgba[4]) {
    const uint32_t n = s.n_bins;
    for (auto* v : {&b.x, &b.y, &b.z, &b.scale, &b.r, &b.g, &b.b, &b.a, &b.calmness, &b.accuracy, &b.deviation}) v->assign(n, 0.0f);
    b.visible.assign(n, 0);
    for (uint32_t idx = 0; idx < n; ++idx) {
        scene::bin_to_spiral(s.bpo, static_cast<float>(idx), b.x[idx], b.y[idx]);   // setup.rs:95, util.rs:3-7
        b.z[idx] = -0.01f;                                                          // setup.rs:112
        const bool intro = idx % 17u == 0u;                                         // setup.rs:106
        b.scale[idx] = intro ? 3.0f : 0.0f;                                         // setup.rs:113-117
        b.visible[idx] = intro;                                                     // setup.rs:118-122
        b.r[idx] = scene::srgb_to_linear(1.0f);                                     // setup.rs:100
        b.g[idx] = scene::srgb_to_linear(0.7f);
        b.b[idx] = scene::srgb_to_linear(0.6f);
        b.a[idx] = 1.0f;
    }
    bass_rgba[0] = 0.8f;   // setup.rs:161
    bass_rgba[1] = 0.7f;
    bass_rgba[2] = 0.6f;
    bass_rgba[3] = 1.0f;
}

SceneState::SceneState(const scene::Settings& s) : s_(s), dropoff_(s.n_bins), owner_(s.n_bins), hide_(s.n_bins) {
    scene_initial(s_, b_, bass_rgba_);
}

void SceneState::update(const float* center, const float* size, uint32_t n_peaks, const float* calmness, const float* pitch_accuracy,
                        const float* pitch_deviation, float scene_calmness, uint64_t frame_time_ns, const float* ml_prob) {
    const uint32_t n = s_.n_bins;
    if (frame_time_ns != table_ns_) {
        scene_fade_table(n, frame_time_ns, dropoff_.data(), z_step_);
        table_ns_ = frame_time_ns;
    }
    for (uint32_t idx = 0; idx < n; ++idx) {   // update.rs:80
        bool vis = b_.visible[idx] != 0;
        scene::fade_ball(b_.scale[idx], b_.a[idx], b_.z[idx], vis, dropoff_[idx], z_step_);
        b_.visible[idx] = vis;
    }
    if (n_peaks == 0) return;   // update.rs:85-87

    float best = scene::F32_MIN;   // update.rs:199-206
    uint32_t k_max = 0;
    for (uint32_t p = 0; p < n_peaks; ++p)
        if (size[p] > best) {
            best = size[p];
            k_max = p;
        }
    const float max_size = size[k_max];

    // update.rs:208-212: the map keeps the LAST entry of a key
    std::fill(owner_.begin(), owner_.end(), 0u);
    std::fill(hide_.begin(), hide_.end(), 0);
    std::vector<scene::PeakRecord> rec(n_peaks);
    for (uint32_t p = 0; p < n_peaks; ++p) {
        scene::peak_record(s_, center[p], size[p], max_size, calmness, pitch_accuracy, pitch_deviation, rec[p], ml_prob);
        if (rec[p].key < n) owner_[rec[p].key] = p + 1u;
    }
    for (uint32_t idx = 0; idx < n; ++idx) {   // update.rs:214-304
        if (!owner_[idx]) continue;
        const scene::PeakRecord& q = rec[owner_[idx] - 1u];
        b_.x[idx] = q.x; b_.y[idx] = q.y; b_.z[idx] = q.z; b_.scale[idx] = q.scale;
        b_.r[idx] = q.r; b_.g[idx] = q.g; b_.b[idx] = q.b; b_.a[idx] = q.a;
        b_.calmness[idx] = q.calmness; b_.accuracy[idx] = q.accuracy; b_.deviation[idx] = q.deviation;
        if (q.shows) b_.visible[idx] = 1;
        for (uint32_t i = q.lo; i <= q.hi && i < n; ++i) hide_[i] = 1;   // update.rs:308-319: the map's entries only
    }
    for (uint32_t idx = 0; idx < n; ++idx)   // update.rs:320-330
        if (hide_[idx] && !owner_[idx]) b_.visible[idx] = 0;

    bloom_ = scene::bloom_of(s_, scene_calmness);   // update.rs:98
    float rgba[4];
    bass_lit_ = scene::bass_of(s_, center[0], size[0], max_size, rgba);   // update.rs:100-107
    if (bass_lit_)
        for (int i = 0; i < 4; ++i) bass_rgba_[i] = rgba[i];
}

}  // namespace pvq
