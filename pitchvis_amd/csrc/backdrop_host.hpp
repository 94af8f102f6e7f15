// backdrop_host.hpp — the picture behind the pitch balls for ONE frame on the host: the spider net (setup.rs:174-222), the debug
// panels' meshes (panels_host.hpp) and the lit part of the bass spiral (setup.rs:127-172, update.rs:369-425), blended in the
// viewer's order over the clear colour or the caller's background.  The one-frame face and second reference of BackdropBatch
// (backdrop_batch.hpp); the arithmetic is backdrop_math.hpp's on both.  raster_frame(background = this image) is the whole 2-D
// picture but for what pvq.h lists as left out.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/pvq.h"
#include "backdrop_math.hpp"

namespace pvq {

// the static quads of `what` (backdrop::What), [n][4][2]
std::vector<float> backdrop_geometry(uint32_t octaves, int what);

// n_triangles flat-coloured triangles, pos [n][3][2] and rgba [n][4] (linear), blended in index order into image [H][W][4];
// transform (tx, ty, sx, sy) or null.  viewport_height > 0.  samples 1, or 4 (backdrop_math.hpp, multisampling: image_inout is a
// resolved picture, every sample starts from its pixel, and the result is resolved back; the four sample planes are host memory
// of 4 x the image's size for the length of the call).  The caller has checked samples.
void backdrop_draw_mesh(uint32_t W, uint32_t H, float viewport_height, size_t n_triangles, const float* pos, const float* rgba,
                        const float* transform, float* image_inout, uint32_t samples = 1);

// One frame.  panels (one row of host pointers) or null; background [H][W][4] or null: the clear colour of visuals_mode.
// samples as above: layers 0 - 6 drawn per sample, resolved into image_out.
void backdrop_frame(uint32_t octaves, uint32_t buckets_per_octave, uint32_t W, uint32_t H, float viewport_height, int visuals_mode,
                    uint32_t bass_lit, const float* bass_rgba, const pvq_backdrop_panels* panels, const float* background,
                    float* image_out, uint32_t samples = 1);

}  // namespace pvq
