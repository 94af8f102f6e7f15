// present_batch.hpp — the present stage (present_host.hpp) for MANY pictures on the GPU: every row [H][W][4] of linear f32 that the
// picture chain leaves in device memory (BackdropBatch, RasterBatch::frames_device(.., over = true), OverlayBatch) is bloomed with
// the row's intensity — SceneBatch's `bloom` buffer as it lies —, display-transformed and encoded to [H][W][4] bytes.  Stateless:
// the handle owns one grow-only workspace for the mip chains of a piece of a call's rows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "device_support.hpp"
#include "present_host.hpp"

namespace pvq {

class PresentBatch {
   public:
    // The arguments are checked before any device is touched.  device_id < 0: a host-only object whose device call returns
    // PVQ_ERR_NO_DEVICE after the argument checks.  settings: checked, max_mip_dimension 0 allowed.
    static pvq_status create(int device_id, const present::Settings& settings, uint32_t width, uint32_t height, std::unique_ptr<PresentBatch>& out);
    // upper bound of the mip-chain workspace (default 1 GiB): a call whose rows need more runs in pieces; one row's chain always fits
    pvq_status set_workspace_limit(uint64_t bytes);
    // d_image [n_rows][H][W][4] f32, 16-byte aligned, never written; d_intensity [n_rows] or null (no bloom in any row); d_rgba8
    // [n_rows][H][W][4] bytes, 4-byte aligned; d_hdr null or [n_rows][H][W][4] f32, 16-byte aligned, may be d_image.  Asynchronous on
    // `stream`; one handle's calls are stream-ordered.
    pvq_status rows_device(size_t n_rows, const float* d_image, const float* d_intensity, uint8_t* d_rgba8, float* d_hdr, hipStream_t stream);

   private:
    PresentBatch() = default;
    int device_id_ = -1;
    uint32_t width_ = 0, height_ = 0;
    present::Settings settings_{};
    PresentPlan plan_{};
    present::Factors factors_{};
    uint64_t limit_ = 1ull << 30;
    bool staged_first_ = false, staged_last_ = false;   // the picture's two passes stage their tiles' source footprints in LDS
    DeviceBuffer chains_;                        // [rows of a piece][plan_.texels] 16-byte texels
};

}  // namespace pvq
