// raster_host.hpp — the pitch balls as pixels for ONE frame on the host: what Bevy draws from the ball records the scene stage
// (scene_host.hpp) leaves — the ball material's fragment (noisy_color_rings_2d.wgsl:395-428) over a 20 x 20 rectangle per ball
// (setup.rs:110-112), seen by the orthographic camera of setup.rs:359-365, the balls blended back to front over the clear colour
// (mod.rs:19-21).  The one-frame face and second reference of RasterBatch (raster_batch.hpp); the arithmetic is raster_math.hpp's
// on both.
//
// The output is the linear HDR target before bloom and tone mapping.  Left out: bloom and the display transform (Bevy's own passes,
// not in the reference tree), the spider net, the bass spiral and the text (the background argument is their hook).
#pragma once

#include <cstdint>

#include "raster_math.hpp"

namespace pvq {

// one fragment: rgba linear, params (calmness, time, pitch_accuracy, pitch_deviation), mesh uv -> premultiplication-free rgba
void raster_shade(const float rgba[4], const float params[4], float u, float v, float out[4]);

// params.time of every ball after a frame with this peak list (update.rs:239): every entry's key bin takes `elapsed`
void raster_touch(uint32_t n_bins, const float* center, uint32_t n_peaks, float elapsed, float* time_inout);

// One frame: ball_xyzs / ball_rgba [n_bins][4], ball_params [n_bins][3], ball_visible [ceil(n_bins / 32)] bit mask, ball_time
// [n_bins].  background [H][W][4] or null: the clear colour of visuals_mode.  image_out [H][W][4].  viewport_height > 0.
void raster_frame(uint32_t n_bins, uint32_t W, uint32_t H, float viewport_height, int visuals_mode, const float* ball_xyzs,
                  const float* ball_rgba, const float* ball_params, const uint32_t* ball_visible, const float* ball_time,
                  const float* background, float* image_out);

}  // namespace pvq
