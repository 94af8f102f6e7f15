// capi_geometry.cpp — extern "C" surface of libpvq (include/pvq.h): render rows, the pitch-ball scene, the debug panels.
#include <vector>

#include "capi_support.hpp"
#include "panels_batch.hpp"
#include "panels_host.hpp"
#include "render_batch.hpp"
#include "scene_batch.hpp"
#include "scene_host.hpp"

extern "C" {

// pitchvis_viewer/src/display_system/update.rs:961-1065: the spectrogram row of one AnalysisState
pvq_status pvq_spectrogram_row(int mode, uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, const float* center,
                               const float* size, uint32_t n_peaks, const float* colors, float gray_level, float easing_pow, uint8_t* out_rgba) {
    return guarded([&] {
        if (mode != PVQ_SPECTROGRAM_VQT && mode != PVQ_SPECTROGRAM_PEAKS) return invalid_arg("unknown spectrogram mode");
        if (buckets_per_octave == 0 || !colors || (!out_rgba && n_buckets) || (mode == PVQ_SPECTROGRAM_VQT && !x_vqt_smoothed && n_buckets) ||
            (mode == PVQ_SPECTROGRAM_PEAKS && n_peaks && (!center || !size))) {
            return invalid_arg("spectrogram row: buckets_per_octave == 0 or a missing array");
        }
        pvq::spectrogram_row(mode, n_buckets, buckets_per_octave, x_vqt_smoothed, center, size, n_peaks,
                             reinterpret_cast<const float(*)[3]>(colors), gray_level, easing_pow, out_rgba);
        return PVQ_OK;
    });
}
// update.rs:1102-1131: the chroma strengths of one AnalysisState
pvq_status pvq_chroma_row(float min_freq, uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, float out12[12]) {
    return guarded([&] {
        if (buckets_per_octave == 0 || !out12 || (!x_vqt_smoothed && n_buckets))
            return invalid_arg("chroma row: buckets_per_octave == 0 or a missing array");
        pvq::chroma_row(min_freq, n_buckets, buckets_per_octave, x_vqt_smoothed, out12);
        return PVQ_OK;
    });
}
// update.rs:961-1065 + 1102-1131 and pitchvis_serial/src/main.rs:122-175 for many rows, on the device (render_batch.hpp)
pvq_status pvq_render_batch_create(int device_id, float min_freq, uint32_t octaves, uint32_t buckets_per_octave, const float* colors,
                                   float gray_level, float easing_pow, pvq_render_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::RenderBatch::create(device_id, min_freq, octaves, buckets_per_octave, colors, gray_level, easing_pow, impl);
        });
    });
}
void pvq_render_batch_destroy(pvq_render_batch* r) { destroy(r); }
pvq_status pvq_render_batch_rows_device(pvq_render_batch* r, size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center,
                                        const float* d_size, const uint32_t* d_peak_count, uint32_t max_peaks, const pvq_render_outputs* outs,
                                        void* stream) {
    return guarded([&] {
        if (!r) return null_handle();
        const pvq_render_outputs none{};
        return r->impl->rows_device(n_rows, d_x_vqt_smoothed, d_center, d_size, d_peak_count, max_peaks, outs ? *outs : none,
                                    static_cast<hipStream_t>(stream));   // update.rs:961-1065, 1102-1131; main.rs:122-175
    });
}

// pitchvis_viewer/src/display_system/update.rs:38-426: the pitch-ball scene, one stream on the host (scene_host.hpp) and many on the
// device (scene_batch.hpp)
void pvq_scene_default_settings(pvq_scene_settings* s) {
    guarded([&] {
        if (!s) return;
        s->visuals_mode = PVQ_VISUALS_FULL;
        s->enable_bloom = 1;
        s->colors = nullptr;
        s->gray_level = 60.0f;   // pitchvis_colors/src/lib.rs:56-57
        s->easing_pow = 1.3f;
    });
}
pvq_status pvq_scene_state_create(uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings* settings, pvq_scene_state** out) {
    return guarded([&] {
        if (!out) return null_handle();
        *out = nullptr;
        if (octaves == 0 || buckets_per_octave == 0 || static_cast<uint64_t>(octaves) * buckets_per_octave > 0x7FFFFFFFull)
            return invalid_arg("scene: octaves and buckets_per_octave must be positive");
        pvq_scene_settings cfg;
        pvq_scene_default_settings(&cfg);
        if (settings) cfg = *settings;
        pvq::scene::Settings s;
        if (!pvq::scene_settings(octaves, buckets_per_octave, cfg.visuals_mode, cfg.enable_bloom, cfg.colors, cfg.gray_level, cfg.easing_pow, s))
            return invalid_arg("scene: unknown visuals mode");
        *out = new pvq_scene_state{std::unique_ptr<pvq::SceneState>(new pvq::SceneState(s))};
        return PVQ_OK;
    });
}
void pvq_scene_state_destroy(pvq_scene_state* s) { destroy(s); }
uint32_t pvq_scene_state_n_bins(const pvq_scene_state* s) { return guarded(0, [&] { return s ? s->impl->settings().n_bins : 0; }); }
uint32_t pvq_scene_state_n_segments(const pvq_scene_state* s) { return guarded(0, [&] { return s ? s->impl->settings().n_segments : 0; }); }
pvq_status pvq_scene_state_update(pvq_scene_state* s, const float* center, const float* size, uint32_t n_peaks, const float* calmness,
                                  const float* pitch_accuracy, const float* pitch_deviation, float scene_calmness, uint64_t frame_time_ns) {
    return guarded([&] {
        if (!s) return null_handle();
        if (n_peaks && (!center || !size || !calmness || !pitch_accuracy || !pitch_deviation))
            return invalid_arg("scene: a frame with peaks needs center, size, calmness, pitch_accuracy and pitch_deviation");
        s->impl->update(center, size, n_peaks, calmness, pitch_accuracy, pitch_deviation, scene_calmness, frame_time_ns);
        return PVQ_OK;
    });
}
// the same frame with the `ml` branch (update.rs:247-255); ml_prob null: the call above
pvq_status pvq_ml_scene_state_update(pvq_scene_state* s, const float* center, const float* size, uint32_t n_peaks, const float* calmness,
                                     const float* pitch_accuracy, const float* pitch_deviation, float scene_calmness, uint64_t frame_time_ns,
                                     const float* ml_prob) {
    return guarded([&] {
        if (!s) return null_handle();
        if (n_peaks && (!center || !size || !calmness || !pitch_accuracy || !pitch_deviation))
            return invalid_arg("scene: a frame with peaks needs center, size, calmness, pitch_accuracy and pitch_deviation");
        s->impl->update(center, size, n_peaks, calmness, pitch_accuracy, pitch_deviation, scene_calmness, frame_time_ns, ml_prob);
        return PVQ_OK;
    });
}
// display_system/util.rs:23-31
pvq_status pvq_ml_midi_pitch(uint32_t buckets_per_octave, uint32_t bin, uint32_t* out_pitch) {
    return guarded([&] {
        if (!out_pitch || buckets_per_octave == 0) return invalid_arg("scene: midi pitch needs buckets_per_octave > 0 and an output");
        const uint32_t m = pvq::scene::midi_pitch(buckets_per_octave, bin);
        *out_pitch = m < pvq::scene::MIDI_PITCHES ? m : UINT32_MAX;
        return PVQ_OK;
    });
}
pvq_status pvq_scene_state_get(const pvq_scene_state* s, float* ball_xyzs, float* ball_rgba, float* ball_params, uint32_t* ball_visible,
                               uint32_t* bass_lit, float* bass_rgba, float* bloom) {
    return guarded([&] {
        if (!s) return null_handle();
        const pvq::SceneBalls& b = s->impl->balls();
        const uint32_t n = s->impl->settings().n_bins;
        if (ball_visible)
            for (uint32_t w = 0; w < (n + 31) / 32; ++w) ball_visible[w] = 0u;
        for (uint32_t i = 0; i < n; ++i) {
            if (ball_xyzs) { ball_xyzs[4 * i] = b.x[i]; ball_xyzs[4 * i + 1] = b.y[i]; ball_xyzs[4 * i + 2] = b.z[i]; ball_xyzs[4 * i + 3] = b.scale[i]; }
            if (ball_rgba) { ball_rgba[4 * i] = b.r[i]; ball_rgba[4 * i + 1] = b.g[i]; ball_rgba[4 * i + 2] = b.b[i]; ball_rgba[4 * i + 3] = b.a[i]; }
            if (ball_params) { ball_params[3 * i] = b.calmness[i]; ball_params[3 * i + 1] = b.accuracy[i]; ball_params[3 * i + 2] = b.deviation[i]; }
            if (ball_visible && b.visible[i]) ball_visible[i / 32] |= 1u << (i % 32);
        }
        if (bass_lit) *bass_lit = s->impl->bass_lit();
        if (bass_rgba)
            for (int i = 0; i < 4; ++i) bass_rgba[i] = s->impl->bass_rgba()[i];
        if (bloom) *bloom = s->impl->bloom();
        return PVQ_OK;
    });
}
pvq_status pvq_scene_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings* settings,
                                  uint32_t n_streams, pvq_scene_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::SceneBatch::create(device_id, octaves, buckets_per_octave, settings, n_streams, impl);
        });
    });
}
void pvq_scene_batch_destroy(pvq_scene_batch* b) { destroy(b); }
uint32_t pvq_scene_batch_n_segments(const pvq_scene_batch* b) { return guarded(0, [&] { return b ? b->impl->n_segments() : 0; }); }
pvq_status pvq_scene_batch_frames_device(pvq_scene_batch* b, size_t n_frames, const pvq_scene_inputs* in, uint64_t frame_time_ns,
                                         const uint64_t* frame_times_ns, const pvq_scene_outputs* outs, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq_scene_inputs no_in{};
        const pvq_scene_outputs none{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, frame_time_ns, frame_times_ns, outs ? *outs : none,
                                      static_cast<hipStream_t>(stream));
    });
}
// the same frames with the `ml` branch: row (s, f) reads d_ml_prob[(s * ml_stride_frames + f) * 128 + pitch]; null: the call above
pvq_status pvq_ml_scene_batch_frames_device(pvq_scene_batch* b, size_t n_frames, const pvq_scene_inputs* in, const float* d_ml_prob,
                                            size_t ml_stride_frames, uint64_t frame_time_ns, const uint64_t* frame_times_ns,
                                            const pvq_scene_outputs* outs, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq_scene_inputs no_in{};
        const pvq_scene_outputs none{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, frame_time_ns, frame_times_ns, outs ? *outs : none,
                                      static_cast<hipStream_t>(stream), d_ml_prob, ml_stride_frames);
    });
}
pvq_status pvq_scene_batch_get_state(pvq_scene_batch* b, uint32_t stream_index, float* ball_xyzs, float* ball_rgba, float* ball_params,
                                     uint32_t* ball_visible, uint32_t* bass_lit, float* bass_rgba, float* bloom) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_state(stream_index, ball_xyzs, ball_rgba, ball_params, ball_visible, bass_lit, bass_rgba, bloom);
    });
}

// pitchvis_viewer/src/display_system/update.rs:474-869: the debug panels, one stream on the host (panels_host.hpp) and many on the
// device (panels_batch.hpp)
pvq_status pvq_spectrum_mesh(uint32_t n_buckets, uint16_t buckets_per_octave, const float* x_vqt_smoothed, const float* center, const float* size,
                             uint32_t n_peaks, const float* colors, float gray_level, float* line_pos, float* line_rgba, float* disc_pos,
                             float* disc_rgba) {
    return guarded([&] {
        if (n_buckets < 2 || buckets_per_octave == 0 || !colors)
            return invalid_arg("spectrum mesh: n_buckets < 2, buckets_per_octave == 0 or no colors");
        if (((line_pos || line_rgba) && !x_vqt_smoothed) || ((disc_pos || disc_rgba) && n_peaks && (!center || !size)))
            return invalid_arg("spectrum mesh: the line reads x_vqt_smoothed, the discs read center and size");
        std::vector<float> rgb(3 * static_cast<size_t>(buckets_per_octave));
        float cs[24];
        pvq::panel_color_table(buckets_per_octave, colors, gray_level, rgb.data());
        pvq::panel_disc_table(cs);
        pvq::spectrum_mesh(n_buckets, buckets_per_octave, x_vqt_smoothed, center, size, n_peaks, rgb.data(), cs, line_pos, line_rgba, disc_pos,
                           disc_rgba);
        return PVQ_OK;
    });
}
pvq_status pvq_calmness_histogram_mesh(uint32_t n_buckets, const float* calmness, float* pos, float* rgba) {
    return guarded([&] {
        if (n_buckets < 2 || !calmness) return invalid_arg("calmness histogram: n_buckets < 2 or no calmness");
        pvq::calmness_histogram_mesh(n_buckets, calmness, pos, rgba);
        return PVQ_OK;
    });
}
pvq_status pvq_calmness_graph_create(uint32_t capacity, pvq_calmness_graph** out) {
    return guarded([&] {
        if (!out) return null_handle();
        *out = nullptr;
        const uint32_t cap = capacity ? capacity : pvq::panels::DEFAULT_GRAPH_CAPACITY;
        if (cap < 2 || cap > 1024) return invalid_arg("calmness graph: capacity must be 2 .. 1024 (0: 300)");
        *out = new pvq_calmness_graph{pvq::CalmnessGraph(cap)};
        return PVQ_OK;
    });
}
void pvq_calmness_graph_destroy(pvq_calmness_graph* g) { destroy(g); }
uint32_t pvq_calmness_graph_capacity(const pvq_calmness_graph* g) { return guarded(0, [&] { return g ? g->impl.capacity() : 0; }); }
pvq_status pvq_calmness_graph_push(pvq_calmness_graph* g, float value) {
    return guarded([&] {
        if (!g) return null_handle();
        g->impl.push(value);
        return PVQ_OK;
    });
}
pvq_status pvq_calmness_graph_mesh(const pvq_calmness_graph* g, float* pos, float* rgba, float* history) {
    return guarded([&] {
        if (!g) return null_handle();
        g->impl.mesh(pos, rgba);
        if (history) g->impl.history(history);
        return PVQ_OK;
    });
}
pvq_status pvq_panel_topology(uint32_t n_quads, uint32_t n_circles, uint32_t* indices, float* uvs) {
    return guarded([&] {
        if (4ull * n_quads + 13ull * n_circles > 0xFFFFFFFFull) return invalid_arg("panel topology: the vertex count does not fit a u32 index");
        pvq::panel_topology(n_quads, n_circles, indices, uvs);
        return PVQ_OK;
    });
}
pvq_status pvq_panels_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const float* colors, float gray_level,
                                   uint32_t n_streams, uint32_t graph_capacity, pvq_panels_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::PanelsBatch::create(device_id, octaves, buckets_per_octave, colors, gray_level, n_streams, graph_capacity, impl);
        });
    });
}
void pvq_panels_batch_destroy(pvq_panels_batch* b) { destroy(b); }
uint32_t pvq_panels_batch_graph_capacity(const pvq_panels_batch* b) { return guarded(0, [&] { return b ? b->impl->graph_capacity() : 0; }); }
pvq_status pvq_panels_batch_rows_device(pvq_panels_batch* b, size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center,
                                        const float* d_size, const uint32_t* d_peak_count, uint32_t max_peaks, const float* d_calmness,
                                        const pvq_panels_outputs* outs, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq_panels_outputs none{};
        return b->impl->rows_device(n_rows, d_x_vqt_smoothed, d_center, d_size, d_peak_count, max_peaks, d_calmness, outs ? *outs : none,
                                    static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_panels_batch_graph_device(pvq_panels_batch* b, size_t n_frames, const float* d_scene_calmness, size_t first_emitted,
                                         float* graph_pos, float* graph_rgba, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->graph_device(n_frames, d_scene_calmness, first_emitted, graph_pos, graph_rgba, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_panels_batch_get_history(pvq_panels_batch* b, uint32_t stream_index, float* out) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_history(stream_index, out);
    });
}

}  // extern "C"
