// text_batch.hpp — the pitch-name labels (text_host.hpp) for MANY rows on the GPU: the labels are blended, in place, over every
// row's finished picture [H][W][4] of linear f32 (BackdropBatch, then RasterBatch::frames_device(.., over = true)), before
// OverlayBatch.  The text is the same for every row, so the handle owns a compact coverage layer, computed on the device once at
// create: one f32 per pixel of each (tile, label) entry, entries sorted by tile then label, over the stage::TILE tiles that the
// labels' pixel boxes meet only.  Stateless after create.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "text_host.hpp"

namespace pvq {

class TextBatch {
   public:
    // The arguments are checked and the labels laid out before any device is touched.  device_id < 0: a host-only object whose
    // device calls return PVQ_ERR_NO_DEVICE after the argument checks.
    static pvq_status create(int device_id, TextFont& font, const pvq_text_label* labels, uint32_t n, float viewport_height, uint32_t width,
                             uint32_t height, std::unique_ptr<TextBatch>& out);
    // Asynchronous on `stream`; one handle's calls are stream-ordered.
    pvq_status rows_device(size_t n_rows, float* d_image_inout, hipStream_t stream);
    // out [H][W]: label 0 .. n - 1, or -1: the largest over the labels (synchronises)
    pvq_status get_coverage(int label, float* out);

   private:
    TextBatch() = default;
    int device_id_ = -1;
    uint32_t n_labels_ = 0, width_ = 0, height_ = 0, n_tiles_ = 0;
    std::vector<uint32_t> entries_;   // [n_entries][2]: tile, label — the layer's index, kept for get_coverage
    DeviceBuffer layer_;              // [n_entries][256] coverages, a tile's pixels in the order of its workgroup's threads
    DeviceBuffer tiles_;              // [n_tiles][4]: tile, first entry, entries, 0
    DeviceBuffer entry_labels_;       // [n_entries] label of each entry
    DeviceBuffer colors_;             // [n_labels][4] linear RGB
};

}  // namespace pvq
