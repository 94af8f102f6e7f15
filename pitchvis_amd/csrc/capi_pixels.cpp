// capi_pixels.cpp — extern "C" surface of libpvq (include/pvq.h): the pictures in linear light: raster, backdrop, overlay, text.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "backdrop_batch.hpp"
#include "backdrop_host.hpp"
#include "capi_support.hpp"
#include "overlay_batch.hpp"
#include "overlay_host.hpp"
#include "raster_batch.hpp"
#include "raster_host.hpp"
#include "readout_batch.hpp"
#include "readout_host.hpp"
#include "stage_plan.hpp"
#include "text_batch.hpp"
#include "text_host.hpp"

namespace {
float viewport_or_default(float viewport_height) { return viewport_height == 0.0f ? pvq::raster::VIEWPORT_HEIGHT : viewport_height; }
}  // namespace

extern "C" {

// noisy_color_rings_2d.wgsl:395-428 with setup.rs:110-112, :359-365: the pitch balls as pixels, one frame on the host
// (raster_host.hpp) and many streams on the device (raster_batch.hpp)
pvq_status pvq_raster_shade(const float* rgba, const float* params, float u, float v, float* out4) {
    return guarded([&] {
        if (!rgba || !params || !out4) return invalid_arg("raster shade: rgba, params and out4 are needed");
        pvq::raster_shade(rgba, params, u, v, out4);
        return PVQ_OK;
    });
}
pvq_status pvq_raster_touch(uint32_t n_bins, const float* center, uint32_t n_peaks, float elapsed, float* time_inout) {
    return guarded([&] {
        if (!time_inout || (n_peaks && !center)) return invalid_arg("raster touch: time_inout is needed, and center with n_peaks > 0");
        pvq::raster_touch(n_bins, center, n_peaks, elapsed, time_inout);
        return PVQ_OK;
    });
}
pvq_status pvq_raster_frame(uint32_t n_bins, uint32_t width, uint32_t height, float viewport_height, int visuals_mode, const float* ball_xyzs,
                            const float* ball_rgba, const float* ball_params, const uint32_t* ball_visible, const float* ball_time,
                            const float* background, float* image_out) {
    return guarded([&] {
        if (!ball_xyzs || !ball_rgba || !ball_params || !ball_visible || !ball_time || !image_out)
            return invalid_arg("raster frame: the five ball arrays and image_out are needed");
        std::string err;
        if (!pvq::stage_image_ok("raster frame", width, height, viewport_height, err) || !pvq::stage_mode_ok("raster frame", visuals_mode, err))
            return invalid_arg(err);
        pvq::raster_frame(n_bins, width, height, viewport_or_default(viewport_height), visuals_mode,
                          ball_xyzs, ball_rgba, ball_params, ball_visible, ball_time, background, image_out);
        return PVQ_OK;
    });
}
pvq_status pvq_raster_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                   uint32_t n_streams, uint32_t width, uint32_t height, pvq_raster_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::RasterBatch::create(device_id, octaves, buckets_per_octave, visuals_mode, viewport_height, n_streams,
                                     width, height, impl);
        });
    });
}
void pvq_raster_batch_destroy(pvq_raster_batch* b) { destroy(b); }
pvq_status pvq_raster_batch_frames_device(pvq_raster_batch* b, size_t n_frames, const pvq_raster_inputs* in, const float* elapsed_s,
                                          float* d_image, float* d_ball_time, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq_raster_inputs no_in{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, elapsed_s, d_image, d_ball_time, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_raster_batch_get_times(pvq_raster_batch* b, uint32_t stream_index, float* out) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_times(stream_index, out);
    });
}

// The picture behind the balls — spider net, debug panels, lit bass spiral (setup.rs:127-222, update.rs:369-425, :474-869 as pixels):
// one frame on the host (backdrop_host.hpp) and many streams on the device (backdrop_batch.hpp)
pvq_status pvq_backdrop_geometry(uint32_t octaves, int what, float* quads_out, uint32_t* n_out) {
    return guarded([&] {
        if (octaves == 0 || octaves > 1024 || what < pvq::backdrop::NET_SPIRAL || what > pvq::backdrop::BASS)
            return invalid_arg("backdrop geometry: octaves 1 .. 1024, what one of net spiral, rays, bass");
        if (n_out) *n_out = pvq::backdrop::geometry_count(octaves, what);
        if (quads_out) {
            const std::vector<float> q = pvq::backdrop_geometry(octaves, what);
            std::copy(q.begin(), q.end(), quads_out);
        }
        return PVQ_OK;
    });
}
pvq_status pvq_backdrop_panel_transforms(uint32_t n_bins, uint32_t width, uint32_t height, float viewport_height, float* out) {
    return guarded([&] {
        if (!out) return invalid_arg("backdrop panel transforms: out is needed");
        std::string err;
        if (!pvq::stage_image_ok("backdrop panel transforms", width, height, viewport_height, err)) return invalid_arg(err);
        pvq::backdrop::panel_transforms(n_bins, width, height, viewport_or_default(viewport_height), out);
        return PVQ_OK;
    });
}
namespace {
// the one-mesh face and the one-frame face behind their one-sample and multisampled entry points: `who` heads the messages
pvq_status backdrop_mesh(const std::string& who, uint32_t samples, uint32_t width, uint32_t height, float viewport_height, size_t n_triangles,
                         const float* pos, const float* rgba, const float* transform, float* image_inout) {
    if (!pvq::backdrop::samples_ok(samples)) return invalid_arg(who + ": samples is 1 or 4");
    if (!image_inout || (n_triangles && (!pos || !rgba))) return invalid_arg(who + ": image_inout is needed, and pos and rgba with n_triangles > 0");
    std::string err;
    if (!pvq::stage_image_ok(who.c_str(), width, height, viewport_height, err)) return invalid_arg(err);
    pvq::backdrop_draw_mesh(width, height, viewport_or_default(viewport_height), n_triangles, pos, rgba, transform, image_inout, samples);
    return PVQ_OK;
}
pvq_status backdrop_one_frame(const std::string& who, uint32_t samples, uint32_t octaves, uint32_t buckets_per_octave, uint32_t width,
                              uint32_t height, float viewport_height, int visuals_mode, uint32_t bass_lit, const float* bass_rgba,
                              const pvq_backdrop_panels* panels, const float* background, float* image_out) {
    if (!pvq::backdrop::samples_ok(samples)) return invalid_arg(who + ": samples is 1 or 4");
    if (!image_out || (bass_lit && !bass_rgba)) return invalid_arg(who + ": image_out is needed, and bass_rgba with bass_lit > 0");
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (octaves == 0 || buckets_per_octave == 0 || octaves > 1024 || n < 2 || n > 0x7FFFFFFFull)
        return invalid_arg(who + ": octaves 1 .. 1024, buckets_per_octave positive, at least two bins");
    std::string err;
    if (!pvq::stage_image_ok(who.c_str(), width, height, viewport_height, err) || !pvq::stage_mode_ok(who.c_str(), visuals_mode, err))
        return invalid_arg(err);
    if (panels && (!panels->line_pos != !panels->line_rgba || !panels->disc_pos != !panels->disc_rgba ||
                   !panels->hist_pos != !panels->hist_rgba || !panels->graph_pos != !panels->graph_rgba ||
                   (panels->graph_pos && panels->graph_capacity < 2))) {
        return invalid_arg(who + ": a mesh needs its positions and its colours, the graph its graph_capacity >= 2");
    }
    pvq::backdrop_frame(octaves, buckets_per_octave, width, height, viewport_or_default(viewport_height), visuals_mode, bass_lit, bass_rgba, panels,
                        background, image_out, samples);
    return PVQ_OK;
}
}  // namespace
pvq_status pvq_backdrop_draw_mesh(uint32_t width, uint32_t height, float viewport_height, size_t n_triangles, const float* pos, const float* rgba,
                                  const float* transform, float* image_inout) {
    return guarded([&] { return backdrop_mesh("backdrop draw mesh", 1, width, height, viewport_height, n_triangles, pos, rgba, transform, image_inout); });
}
pvq_status pvq_backdrop_frame(uint32_t octaves, uint32_t buckets_per_octave, uint32_t width, uint32_t height, float viewport_height,
                              int visuals_mode, uint32_t bass_lit, const float* bass_rgba, const pvq_backdrop_panels* panels,
                              const float* background, float* image_out) {
    return guarded([&] {
        return backdrop_one_frame("backdrop frame", 1, octaves, buckets_per_octave, width, height, viewport_height, visuals_mode, bass_lit, bass_rgba,
                                  panels, background, image_out);
    });
}
pvq_status pvq_backdrop_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                     uint32_t n_streams, uint32_t width, uint32_t height, pvq_backdrop_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::BackdropBatch::create(device_id, octaves, buckets_per_octave, visuals_mode, viewport_height, n_streams,
                                       width, height, impl);
        });
    });
}
void pvq_backdrop_batch_destroy(pvq_backdrop_batch* b) { destroy(b); }
pvq_status pvq_backdrop_batch_frames_device(pvq_backdrop_batch* b, size_t n_frames, const pvq_backdrop_inputs* in, float* d_image, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq_backdrop_inputs no_in{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, d_image, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_backdrop_balls_over_device(pvq_raster_batch* b, size_t n_frames, const pvq_raster_inputs* in, const float* elapsed_s,
                                          float* d_image_inout, float* d_ball_time, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq_raster_inputs no_in{};
        return b->impl->frames_device(n_frames, in ? *in : no_in, elapsed_s, d_image_inout, d_ball_time, static_cast<hipStream_t>(stream), true);
    });
}

// The backdrop multisampled (backdrop_math.hpp: four samples a pixel, resolved at the end of the stage): the faces above with a
// sample count in front.  samples is checked first, before any device is touched; 1 gives the one-sample faces' bits.
pvq_status pvq_msaa_sample_positions(uint32_t samples, float* xy_out) {
    return guarded([&] {
        if (!pvq::backdrop::samples_ok(samples)) return invalid_arg("msaa sample positions: samples is 1 or 4");
        if (!xy_out) return invalid_arg("msaa sample positions: xy_out is needed");
        for (uint32_t k = 0; k < samples; ++k) pvq::backdrop::sample_fraction(samples, k, xy_out[2 * k], xy_out[2 * k + 1]);
        return PVQ_OK;
    });
}
pvq_status pvq_msaa_draw_mesh(uint32_t samples, uint32_t width, uint32_t height, float viewport_height, size_t n_triangles, const float* pos,
                              const float* rgba, const float* transform, float* image_inout) {
    return guarded([&] { return backdrop_mesh("msaa draw mesh", samples, width, height, viewport_height, n_triangles, pos, rgba, transform, image_inout); });
}
pvq_status pvq_msaa_frame(uint32_t samples, uint32_t octaves, uint32_t buckets_per_octave, uint32_t width, uint32_t height, float viewport_height,
                          int visuals_mode, uint32_t bass_lit, const float* bass_rgba, const pvq_backdrop_panels* panels, const float* background,
                          float* image_out) {
    return guarded([&] {
        return backdrop_one_frame("msaa frame", samples, octaves, buckets_per_octave, width, height, viewport_height, visuals_mode, bass_lit, bass_rgba,
                                  panels, background, image_out);
    });
}
pvq_status pvq_msaa_batch_create(uint32_t samples, int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode,
                                 float viewport_height, uint32_t n_streams, uint32_t width, uint32_t height, pvq_backdrop_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::BackdropBatch::create(device_id, octaves, buckets_per_octave, visuals_mode, viewport_height, n_streams, width, height, impl,
                                              samples);
        });
    });
}
uint32_t pvq_msaa_batch_samples(const pvq_backdrop_batch* b) {
    return guarded(0u, [&] { return b ? b->impl->samples() : 0u; });
}

// The spectrogram quad and the chroma boxes in front of the balls (setup.rs:418-541, update.rs:929-1172, spectrogram_scroll.wgsl):
// one stream on the host (overlay_host.hpp) and many streams on the device (overlay_batch.hpp)
namespace {
bool overlay_bins_ok(const char* who, uint32_t n_bins) {
    if (n_bins >= pvq::overlay::MIN_BINS && n_bins <= pvq::overlay::MAX_BINS) return true;
    pvq::set_last_error(std::string(who) + ": n_bins is 3 .. 1024");
    return false;
}
}  // namespace
pvq_status pvq_overlay_quad(uint32_t n_bins, uint32_t history_rows, float* out4) {
    return guarded([&] {
        std::string err;
        if (!out4) return invalid_arg("overlay quad: out4 is needed");
        if (!overlay_bins_ok("overlay quad", n_bins)) return PVQ_ERR_INVALID_ARG;
        if (!pvq::overlay_args_ok("overlay quad", history_rows, 0.0f, nullptr, err)) return invalid_arg(err);
        pvq::overlay::reference_quad(n_bins, history_rows == 0 ? pvq::overlay::HISTORY_ROWS : history_rows, out4);
        return PVQ_OK;
    });
}
pvq_status pvq_overlay_state_create(uint32_t n_bins, uint32_t history_rows, pvq_overlay_state** out) {
    return guarded([&] {
        if (!out) return null_handle();
        *out = nullptr;
        std::string err;
        if (!overlay_bins_ok("overlay state", n_bins)) return PVQ_ERR_INVALID_ARG;
        if (!pvq::overlay_args_ok("overlay state", history_rows, 0.0f, nullptr, err)) return invalid_arg(err);
        *out = new pvq_overlay_state{pvq::OverlayState(n_bins, history_rows == 0 ? pvq::overlay::HISTORY_ROWS : history_rows)};
        return PVQ_OK;
    });
}
void pvq_overlay_state_destroy(pvq_overlay_state* s) { destroy(s); }
pvq_status pvq_overlay_state_push(pvq_overlay_state* s, const uint8_t* row_rgba) {
    return guarded([&] {
        if (!s) return null_handle();
        if (!row_rgba) return invalid_arg("overlay state: row_rgba is needed");
        s->impl.push(row_rgba);
        return PVQ_OK;
    });
}
pvq_status pvq_overlay_state_texture(const pvq_overlay_state* s, uint8_t* out, uint32_t* write_index) {
    return guarded([&] {
        if (!s) return null_handle();
        if (out) std::memcpy(out, s->impl.texture(), static_cast<size_t>(s->impl.history_rows()) * s->impl.n_bins() * 4);
        if (write_index) *write_index = s->impl.write_index();
        return PVQ_OK;
    });
}
pvq_status pvq_overlay_frame(const pvq_overlay_state* state, uint32_t width, uint32_t height, float viewport_height, float ui_scale,
                             const float* quad, const float* chroma12, const float* colors, float* image_inout) {
    return guarded([&] {
        if (!image_inout || (!state && !chroma12)) return invalid_arg("overlay frame: image_inout is needed, and a state or chroma12");
        std::string err;
        if (!pvq::stage_image_ok("overlay frame", width, height, viewport_height, err) ||
            !pvq::overlay_args_ok("overlay frame", 0, ui_scale, quad, err)) {
            return invalid_arg(err);
        }
        pvq::overlay::Tables tables;
        pvq::overlay_tables(colors, tables);
        pvq::overlay_frame(state ? &state->impl : nullptr, width, height, viewport_or_default(viewport_height),
                           ui_scale == 0.0f ? 1.0f : ui_scale, quad, chroma12, tables, image_inout);
        return PVQ_OK;
    });
}
pvq_status pvq_overlay_batch_create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, uint32_t history_rows, float viewport_height,
                                    float ui_scale, const float* quad, const float* colors, uint32_t n_streams, uint32_t width, uint32_t height,
                                    pvq_overlay_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::OverlayBatch::create(device_id, octaves, buckets_per_octave, history_rows, viewport_height, ui_scale, quad, colors,
                                      n_streams, width, height, impl);
        });
    });
}
void pvq_overlay_batch_destroy(pvq_overlay_batch* b) { destroy(b); }
pvq_status pvq_overlay_batch_frames_device(pvq_overlay_batch* b, size_t n_frames, const uint8_t* d_rows, const float* d_chroma,
                                           float* d_image_inout, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->frames_device(n_frames, d_rows, d_chroma, d_image_inout, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_overlay_batch_get_texture(pvq_overlay_batch* b, uint32_t stream_index, uint8_t* out, uint32_t* write_index) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_texture(stream_index, out, write_index);
    });
}

// The pitch-name labels over the balls and under the overlay (setup.rs:386-416): a font the caller brings, one picture on the host
// (text_host.hpp) and many rows on the device (text_batch.hpp)
pvq_status pvq_text_font_from_ttf(const uint8_t* bytes, size_t n_bytes, pvq_text_font** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            std::string err;
            const pvq_status st = pvq::TextFont::from_ttf(bytes, n_bytes, impl, err);
            if (st != PVQ_OK) pvq::set_last_error(err);
            return st;
        });
    });
}
pvq_status pvq_text_font_from_outlines(uint32_t n_glyphs, const uint32_t* codepoints, const float* advances, const uint32_t* n_contours,
                                       const uint32_t* contour_ends, const uint32_t* n_points, const float* points, const uint8_t* on_curve,
                                       uint32_t units_per_em, float ascent, float descent, pvq_text_font** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            std::string err;
            const pvq_status st = pvq::TextFont::from_outlines(n_glyphs, codepoints, advances, n_contours, contour_ends, n_points, points, on_curve,
                                                               units_per_em, ascent, descent, impl, err);
            if (st != PVQ_OK) pvq::set_last_error(err);
            return st;
        });
    });
}
void pvq_text_font_destroy(pvq_text_font* f) { destroy(f); }
pvq_status pvq_text_font_metrics(const pvq_text_font* f, uint32_t* units_per_em, float* ascent, float* descent) {
    return guarded([&] {
        if (!f) return null_handle();
        if (units_per_em) *units_per_em = f->impl->units_per_em();
        if (ascent) *ascent = f->impl->ascent();
        if (descent) *descent = f->impl->descent();
        return PVQ_OK;
    });
}
pvq_status pvq_text_font_glyph(pvq_text_font* f, uint32_t codepoint, float* advance, uint32_t* n_contours, uint32_t* n_points,
                               uint32_t cap_contours, uint32_t cap_points, uint32_t* contour_ends, float* points, uint8_t* on_curve) {
    return guarded([&] {
        if (!f) return null_handle();
        const pvq::TextGlyph* g = nullptr;
        std::string err;
        const pvq_status st = f->impl->glyph(codepoint, g, err);
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        if (advance) *advance = g->advance;
        if (n_contours) *n_contours = static_cast<uint32_t>(g->contour_ends.size());
        if (n_points) *n_points = static_cast<uint32_t>(g->on_curve.size());
        if ((contour_ends && cap_contours < g->contour_ends.size()) || ((points || on_curve) && cap_points < g->on_curve.size()))
            return invalid_arg("text font glyph: an array is smaller than the glyph; ask for the counts first");
        if (contour_ends) std::copy(g->contour_ends.begin(), g->contour_ends.end(), contour_ends);
        if (points) std::copy(g->points.begin(), g->points.end(), points);
        if (on_curve) std::copy(g->on_curve.begin(), g->on_curve.end(), on_curve);
        return PVQ_OK;
    });
}
pvq_status pvq_text_pitch_labels(uint32_t octaves, const float* colors, pvq_text_label* out12) {
    return guarded([&] {
        if (!out12 || octaves == 0 || octaves > 255) return invalid_arg("text pitch labels: octaves is 1 .. 255 and out12 is needed");
        pvq::text_pitch_labels(octaves, colors, out12);
        return PVQ_OK;
    });
}
namespace {
pvq_status text_plans(const char* who, pvq_text_font* font, const pvq_text_label* labels, uint32_t n, uint32_t width, uint32_t height,
                      float viewport_height, std::vector<pvq::TextLabelPlan>& plans) {
    std::string err;
    if (!pvq::stage_image_ok(who, width, height, viewport_height, err)) return invalid_arg(err);
    const pvq_status st = pvq::text_plan(who, *font->impl, labels, n, width, height,
                                         viewport_or_default(viewport_height), plans, err);
    if (st != PVQ_OK) pvq::set_last_error(err);
    return st;
}
}  // namespace
pvq_status pvq_text_layout_query(pvq_text_font* font, const pvq_text_label* labels, uint32_t n, uint32_t width, uint32_t height,
                                 float viewport_height, pvq_text_layout* out_n) {
    return guarded([&] {
        if (!font) return null_handle();
        if (!out_n) return invalid_arg("text layout: out_n is needed");
        std::vector<pvq::TextLabelPlan> plans;
        if (pvq_status st = text_plans("text layout", font, labels, n, width, height, viewport_height, plans)) return st;
        for (uint32_t l = 0; l < n; ++l) {
            const pvq::TextLabelPlan& p = plans[l];
            out_n[l] = pvq_text_layout{p.on_image ? 1u : 0u, p.x0, p.y0, p.x1, p.y1, p.on_image ? static_cast<uint32_t>(p.segments.size()) : 0u,
                                       p.n_tiles(), p.origin_x, p.baseline_y};
        }
        return PVQ_OK;
    });
}
pvq_status pvq_text_frame(pvq_text_font* font, const pvq_text_label* labels, uint32_t n, uint32_t width, uint32_t height, float viewport_height,
                          float* image_inout, float* coverage_out) {
    return guarded([&] {
        if (!font) return null_handle();
        if (!image_inout && !coverage_out) return invalid_arg("text frame: image_inout or coverage_out is needed");
        std::vector<pvq::TextLabelPlan> plans;
        if (pvq_status st = text_plans("text frame", font, labels, n, width, height, viewport_height, plans)) return st;
        pvq::text_frame(plans, width, height, image_inout, coverage_out);
        return PVQ_OK;
    });
}
pvq_status pvq_text_batch_create(int device_id, pvq_text_font* font, const pvq_text_label* labels, uint32_t n, float viewport_height,
                                 uint32_t width, uint32_t height, pvq_text_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            if (!font) return null_handle();
            return pvq::TextBatch::create(device_id, *font->impl, labels, n, viewport_height, width, height, impl);
        });
    });
}
void pvq_text_batch_destroy(pvq_text_batch* b) { destroy(b); }
pvq_status pvq_text_batch_rows_device(pvq_text_batch* b, size_t n_rows, float* d_image_inout, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->rows_device(n_rows, d_image_inout, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_text_batch_get_coverage(pvq_text_batch* b, int label, float* out) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_coverage(label, out);
    });
}

// The tuning-drift readout over the finished picture (common.rs:348-432): the value's text and colour, one picture on the host
// (readout_host.hpp) and many rows, each its own value, on the device (readout_batch.hpp)
pvq_status pvq_readout_text(float value, char text_out[12], float srgb_out[3]) {
    return guarded([&] {
        uint64_t text;
        float r;
        const uint32_t n = pvq::readout::value_glyphs(value, text, r);
        if (text_out) {
            for (uint32_t k = 0; k < n; ++k) text_out[k] = static_cast<char>(pvq::readout::codepoint_of(pvq::readout::slot_glyph(text, pvq::readout::N_PREFIX + k)));
            text_out[n] = 0;
        }
        if (srgb_out) pvq::readout::value_srgb(r, srgb_out);
        return PVQ_OK;
    });
}
namespace {
pvq_status readout_plan_of(const char* who, pvq_text_font* font, uint32_t width, uint32_t height, float ui_scale, pvq::ReadoutPlan& plan) {
    std::string err;
    const pvq_status st = pvq::readout_plan(who, *font->impl, width, height, ui_scale, plan, err);
    if (st != PVQ_OK) pvq::set_last_error(err);
    return st;
}
}  // namespace
pvq_status pvq_readout_layout_query(pvq_text_font* font, float value, uint32_t width, uint32_t height, float ui_scale, pvq_readout_layout* out) {
    return guarded([&] {
        if (!font) return null_handle();
        if (!out) return invalid_arg("readout layout: out is needed");
        pvq::ReadoutPlan plan;
        if (pvq_status st = readout_plan_of("readout layout", font, width, height, ui_scale, plan)) return st;
        pvq::ReadoutRow row;
        pvq::readout_row(plan, value, row);
        std::memset(out, 0, sizeof(*out));
        out->xl = row.box.xl, out->xr = row.box.xr, out->yt = row.box.yt, out->yb = row.box.yb;
        out->text_width = row.text_width, out->font_px = plan.font_px, out->baseline = plan.baseline;
        out->baseline_row = row.baseline_row;
        out->n_slots = row.n_slots;
        for (uint32_t s = 0; s < row.n_slots; ++s) {
            const pvq::readout::Cell& c = plan.cells[row.glyph[s]];
            out->text[s] = static_cast<char>(pvq::readout::codepoint_of(row.glyph[s]));
            out->origin_x[s] = row.origin_x[s];
            out->cell_x0[s] = row.origin_x[s] + c.x0;
            out->cell_y0[s] = row.baseline_row + c.y0;
            out->cell_w[s] = c.w;
            out->cell_h[s] = c.h;
        }
        for (int c = 0; c < 3; ++c) out->value_srgb[c] = row.value_srgb[c], out->value_linear[c] = row.value_linear[c];
        return PVQ_OK;
    });
}
pvq_status pvq_readout_frame(pvq_text_font* font, float value, uint32_t width, uint32_t height, float ui_scale, float* image_inout) {
    return guarded([&] {
        if (!font) return null_handle();
        if (!image_inout) return invalid_arg("readout frame: image_inout is needed");
        pvq::ReadoutPlan plan;
        if (pvq_status st = readout_plan_of("readout frame", font, width, height, ui_scale, plan)) return st;
        pvq::readout_cover(plan);
        pvq::readout_frame(plan, value, image_inout);
        return PVQ_OK;
    });
}
pvq_status pvq_readout_batch_create(int device_id, pvq_text_font* font, uint32_t width, uint32_t height, float ui_scale, pvq_readout_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            if (!font) return null_handle();
            return pvq::ReadoutBatch::create(device_id, *font->impl, width, height, ui_scale, impl);
        });
    });
}
void pvq_readout_batch_destroy(pvq_readout_batch* b) { destroy(b); }
pvq_status pvq_readout_batch_rows_device(pvq_readout_batch* b, size_t n_rows, const float* d_values, float* d_image_inout, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->rows_device(n_rows, d_values, d_image_inout, static_cast<hipStream_t>(stream));
    });
}
pvq_status pvq_readout_batch_get_atlas(pvq_readout_batch* b, uint32_t codepoint, int32_t* x0, int32_t* y0, uint32_t* w, uint32_t* h, float* advance,
                                       size_t cap_floats, float* out) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_atlas(codepoint, x0, y0, w, h, advance, cap_floats, out);
    });
}

}  // extern "C"
