// scene_host.hpp — the viewer's main picture for ONE stream on the host: the pitch-ball spiral, the bass spiral and the bloom that
// pitchvis_viewer/src/display_system/update.rs:38-426 (update_display) builds from an AnalysisState, frame after frame.
//
//   * a ball per bin (setup.rs:89-125) that lights on a peak (update_pitch_balls, update.rs:186-334), fades between frames
//     (fade_pitch_balls, update.rs:136-178) and hides beside a stronger neighbour (update.rs:307-330)
//   * the bass spiral lit up to the lowest note (update_bass_spiral, update.rs:353-426; setup.rs:127-172)
//   * the bloom intensity from the scene's calmness (update_bloom, update.rs:336-351)
//
// Stateful: a ball's scale, alpha and depth carry from frame to frame, and a frame without peaks leaves balls, bass spiral and bloom
// as the previous frame left them (update.rs:85-87).  The one-stream face and second reference of SceneBatch (scene_batch.hpp); the
// arithmetic is scene_math.hpp's on both.
//
// Bloom intensity starts at 0 here; the reference leaves Bevy's default on the camera until the first frame with peaks.
// A peak whose trunc(center) is >= n_bins is ignored (the reference would index out of range); it still counts for max_size.
// The `ml` branch (update.rs:247-255) takes the probabilities as an argument of update: a keyed ball whose MIDI pitch is inferred
// (probability > 0.35) becomes opaque, any other nearly transparent (scene_math.hpp).  Left out: params.time (the caller's clock).  The debug meshes (update_spectrum, the calmness histogram and graph) are panels_host.hpp's.
#pragma once

#include <cstdint>
#include <vector>

#include "scene_math.hpp"

namespace pvq {

// Fills `s` from the geometry and the settings; false (text in *why) for an unknown mode.  colors: 12 RGB triples, null: COLORS.
bool scene_settings(uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, int enable_bloom, const float* colors,
                    float gray_level, float easing_pow, scene::Settings& s);

// what a call knows before it starts: fade_pitch_balls' per-bin dropoff (update.rs:157-159) and z step (update.rs:172) for a frame time
void scene_fade_table(uint32_t n_bins, uint64_t frame_time_ns, float* dropoff, float& z_step);

struct SceneBalls {   // per bin
    std::vector<float> x, y, z, scale, r, g, b, a, calmness, accuracy, deviation;
    std::vector<uint8_t> visible;
};

class SceneState {
   public:
    explicit SceneState(const scene::Settings& s);
    const scene::Settings& settings() const { return s_; }
    // update_display (update.rs:80-107) for one frame; calmness / pitch_accuracy / pitch_deviation [n_bins].  ml_prob: the frame's
    // AnalysisState::ml_midi_base_pitches [128] for the `ml` branch (update.rs:247-255), or null: the branch is off.
    void update(const float* center, const float* size, uint32_t n_peaks, const float* calmness, const float* pitch_accuracy,
                const float* pitch_deviation, float scene_calmness, uint64_t frame_time_ns, const float* ml_prob = nullptr);
    const SceneBalls& balls() const { return b_; }
    uint32_t bass_lit() const { return bass_lit_; }
    const float* bass_rgba() const { return bass_rgba_; }
    float bloom() const { return bloom_; }

   private:
    scene::Settings s_;
    SceneBalls b_;
    uint32_t bass_lit_ = 0;
    float bass_rgba_[4];
    float bloom_ = 0.0f;
    uint64_t table_ns_ = ~0ull;
    std::vector<float> dropoff_;
    float z_step_ = 0.0f;
    std::vector<uint32_t> owner_;
    std::vector<uint8_t> hide_;
};

// the initial state of every scene (setup.rs:89-125, :160-167), shared with SceneBatch
void scene_initial(const scene::Settings& s, SceneBalls& b, float bass_rgba[4]);

}  // namespace pvq
