// readout_batch.hpp — the tuning-drift readout (readout_host.hpp) for MANY rows on the GPU: "Tuning drift: NNN" in its
// half-transparent box, blended in place over every row's finished picture [H][W][4] of linear f32, after OverlayBatch and before
// PresentBatch, in the Debugging display mode only.  The string, its width, its colour and so the box differ row by row: the value
// is one f32 a row in device memory (AnalysisBatch's tuning_grid_inaccuracy), formatted and laid out on the device.  The handle
// owns a glyph atlas, computed on the device once at create.  Stateless after create.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "readout_host.hpp"

namespace pvq {

class ReadoutBatch {
   public:
    // The arguments are checked and the atlas laid out before any device is touched.  device_id < 0: a host-only object whose
    // rows_device returns PVQ_ERR_NO_DEVICE after the argument checks, and whose atlas is the host face's.
    static pvq_status create(int device_id, TextFont& font, uint32_t width, uint32_t height, float ui_scale, std::unique_ptr<ReadoutBatch>& out);
    // Asynchronous on `stream`; one handle's calls are stream-ordered.
    pvq_status rows_device(size_t n_rows, const float* d_values, float* d_image_inout, hipStream_t stream);
    // A codepoint's cell: its box relative to (origin column, baseline row), and its coverages to out [h][w] where out is given and
    // cap_floats holds them (synchronises).  Any of the pointers may be null.
    pvq_status get_atlas(uint32_t codepoint, int32_t* x0, int32_t* y0, uint32_t* w, uint32_t* h, float* advance, size_t cap_floats, float* out);

   private:
    ReadoutBatch() = default;
    int device_id_ = -1;
    ReadoutPlan plan_;        // the cells and, on a host-only handle after the first get_atlas, the host face's atlas
    uint32_t n_tiles_ = 0;    // of the draw grid
    DeviceBuffer atlas_;      // every cell's [h][w] coverages
    DeviceBuffer cells_;      // [N_GLYPHS] readout::Cell
};

}  // namespace pvq
