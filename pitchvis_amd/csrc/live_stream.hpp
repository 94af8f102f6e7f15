// live_stream.hpp — the live front end of one stream (pitchvis_viewer/src/audio_system/audio_desktop.rs:83-118): a device ring the
// audio callback appends to, with the callback's AGC and drop rule, and one VQT frame over the newest n_fft samples on demand.
#pragma once

#include <cstddef>
#include <memory>

#include "consumers_host.hpp"
#include "device_support.hpp"

namespace pvq {

class Vqt;

// device-resident ring: the newest buf_size samples are d_ring[w - buf_size, w); compacted when the linear
// buffer (4 x buf_size) runs out
class LiveStream {
   public:
    // The transform handle must outlive the stream.  PVQ_ERR_BAD_LENGTH for a ring shorter than n_fft, PVQ_ERR_NO_DEVICE for a handle
    // without a GPU.
    static pvq_status create(Vqt* vqt, size_t buf_size, bool with_agc, std::unique_ptr<LiveStream>& out);
    ~LiveStream();   // also runs when create fails half way: no device buffer is leaked
    LiveStream(const LiveStream&) = delete;
    LiveStream& operator=(const LiveStream&) = delete;

    pvq_status push(const float* data, size_t n);    // a chunk with a non-finite sample is dropped; one longer than the ring is refused
    pvq_status frame_db(float* out_db);              // [n_bins]
    pvq_status read(float* out, size_t n_last);      // the newest n_last <= buf_size samples of the ring
    float gain() const { return gain_; }
    float chunk_size_ms() const { return chunk_size_ms_; }

   private:
    LiveStream() = default;
    Vqt* vqt = nullptr;
    size_t buf_size = 0, cap = 0, w = 0;
    float* d_ring = nullptr;
    float* d_db = nullptr;
    bool with_agc = false;
    MonoAgc agc{0.07f, 0.0001f};   // audio_desktop.rs:93
    float gain_ = 0.0f;            // audio_desktop.rs:83
    float chunk_size_ms_ = 0.0f;
    // page-locked staging and a stream of the object's own: a push is one asynchronous DMA behind the conditioning on the host, a frame
    // the kernels + one asynchronous copy back + ONE wait (pageable buffers cost a staged, synchronous copy each way)
    hipStream_t stream = nullptr;
    float* h_in = nullptr;    // [buf_size]: the chunk being appended
    float* h_out = nullptr;   // [n_bins]
    bool in_flight = false;   // h_in is being read by a copy queued on `stream`
};

}  // namespace pvq
