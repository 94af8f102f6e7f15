// backdrop_batch.hpp — the picture behind the pitch balls (backdrop_host.hpp) for MANY streams on the GPU: every (stream, frame) row
// of bass state that SceneBatch leaves and of panel meshes that PanelsBatch leaves in device memory becomes an image [H][W][4] of
// linear f32 — net, panels, lit bass segments over the clear colour — which RasterBatch::frames_device(.., over = true) then
// draws the balls on.  Stateless: the handle holds the static geometry and a grow-only workspace.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "../../include/pvq.h"
#include "backdrop_host.hpp"
#include "device_support.hpp"

namespace pvq {

class BackdropBatch {
   public:
    // The arguments are RasterBatch::create's, checked before any device is touched.  device_id < 0: a host-only object whose
    // frames_device returns PVQ_ERR_NO_DEVICE after the argument checks.  samples: 1, or 4 for the multisampled rule
    // (backdrop_math.hpp), resolved at the end of the stage; anything else is refused first of all.
    static pvq_status create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                             uint32_t n_streams, uint32_t width, uint32_t height, std::unique_ptr<BackdropBatch>& out, uint32_t samples = 1);
    // n_frames frames of every stream.  Asynchronous on `stream`.
    pvq_status frames_device(size_t n_frames, const pvq_backdrop_inputs& in, float* d_image, hipStream_t stream);
    uint32_t samples() const { return samples_; }

   private:
    BackdropBatch() = default;
    int device_id_ = -1;
    uint32_t n_streams_ = 0, n_bins_ = 0, width_ = 0, height_ = 0;
    float vh_ = 0.0f;
    bool galaxy_ = false;
    uint32_t samples_ = 1;
    float clear_[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    uint32_t n_net_ = 0, n_bass_ = 0;   // the net's finished triangles that meet the image; the bass quads
    DeviceBuffer net_;                  // [n_net] backdrop::Tri, shared by all rows
    DeviceBuffer bass_;                 // [n_bass][4][2] floats
    DeviceBuffer ws_;                   // grow-only: the lists and counts of one piece of a call
};

}  // namespace pvq
