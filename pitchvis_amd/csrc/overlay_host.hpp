// overlay_host.hpp — what DisplayMode::Debugging draws in front of the pitch balls, for ONE stream on the host: the ring of
// spectrogram rows kept literally as the viewer keeps its texture (update.rs:1066-1087: the vertical flip, the clear of the next
// line, the write index), the quad that scrolls it (spectrogram_scroll.wgsl) and the twelve chroma boxes, blended over a finished
// image.  The one-frame face and second reference of OverlayBatch (overlay_batch.hpp); the arithmetic is overlay_math.hpp's on both.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "overlay_math.hpp"

namespace pvq {

// history_rows 0 (the viewer's 200) or 2 .. 4096; ui_scale 0 (1) or positive and finite; quad null or finite with positive extents.
// false leaves the text, which begins with `who`, in err (as stage_plan.hpp's checks do).
bool overlay_args_ok(const char* who, uint32_t history_rows, float ui_scale, const float* quad, std::string& err);

// colors: 12 RGB triples in [0, 1] or null (pitchvis_colors::COLORS)
void overlay_tables(const float* colors, overlay::Tables& out);

// The reference's texture: [history_rows][n_bins][4] bytes, all zeros at start.
class OverlayState {
   public:
    OverlayState(uint32_t n_bins, uint32_t history_rows)
        : n_bins_(n_bins), h_(history_rows), texture_(static_cast<size_t>(history_rows) * n_bins * 4, 0) {}
    // update.rs:1066-1087: the row goes to texture row h - 1 - write_index, the row of the next index is zeroed
    void push(const uint8_t* row_rgba);
    uint32_t n_bins() const { return n_bins_; }
    uint32_t history_rows() const { return h_; }
    uint32_t write_index() const { return write_index_; }
    const uint8_t* texture() const { return texture_.data(); }

   private:
    uint32_t n_bins_, h_, write_index_ = 0;
    std::vector<uint8_t> texture_;
};

// Both layers over image_inout [H][W][4].  state or null: no quad; quad (cx, cy, ex, ey) or null: the reference's for the state;
// chroma12 or null: no boxes.  viewport_height > 0, ui_scale > 0.
void overlay_frame(const OverlayState* state, uint32_t W, uint32_t H, float viewport_height, float ui_scale, const float* quad,
                   const float* chroma12, const overlay::Tables& tables, float* image_inout);

// The 16 x 16 tiles of a W x H image, row-major numbers, that either layer can touch, for the device stage's launch: tile |
// QUAD_TILE where the quad's pixel box meets it, | BOX_TILE where the chroma boxes' does.  The boxes err outwards.
constexpr uint32_t QUAD_TILE = 1u << 30, BOX_TILE = 1u << 31, TILE_MASK = QUAD_TILE - 1u;
std::vector<uint32_t> overlay_tiles(uint32_t W, uint32_t H, float viewport_height, float ui_scale, const float quad[4]);

}  // namespace pvq
