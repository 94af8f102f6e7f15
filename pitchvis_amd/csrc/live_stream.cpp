// live_stream.cpp — see live_stream.hpp.  Compiled as the extern "C" units are (its sum of squares decides the frozen gain).
#include "live_stream.hpp"

#include <algorithm>
#include <cmath>

#include "vqt_engine.hpp"

namespace pvq {

LiveStream::~LiveStream() {
    if (stream) {
        (void)hipStreamSynchronize(stream);
        (void)hipStreamDestroy(stream);
    }
    if (d_ring) (void)hipFree(d_ring);
    if (d_db) (void)hipFree(d_db);
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
}

pvq_status LiveStream::create(Vqt* vqt, size_t buf_size, bool with_agc, std::unique_ptr<LiveStream>& out) {
    const size_t n_fft = vqt->params().n_fft;
    if (buf_size < n_fft) {
        pvq::set_last_error("ring buffer shorter than n_fft");
        return PVQ_ERR_BAD_LENGTH;
    }
    if (!vqt->has_device()) {
        pvq::set_last_error("the streaming front end needs a GPU handle");
        return PVQ_ERR_NO_DEVICE;
    }
    std::unique_ptr<LiveStream> s(new LiveStream());
    s->vqt = vqt;
    s->buf_size = buf_size;
    s->cap = 4 * buf_size;
    s->with_agc = with_agc;
    PVQ_HIP(hipSetDevice(vqt->device()));
    PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_ring), s->cap * sizeof(float)));
    PVQ_HIP(hipMemset(s->d_ring, 0, s->cap * sizeof(float)));
    PVQ_HIP(hipStreamSynchronize(nullptr));   // (the object's own stream does not wait for the null stream)
    PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_db), vqt->n_bins() * sizeof(float)));
    PVQ_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_in), buf_size * sizeof(float), hipHostMallocDefault));
    PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_out), vqt->n_bins() * sizeof(float), hipHostMallocDefault));
    s->w = buf_size;
    out = std::move(s);
    return PVQ_OK;
}

pvq_status LiveStream::push(const float* data, size_t n) {
    if (n == 0) return PVQ_OK;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(data[i])) return PVQ_OK;   // audio_desktop.rs:97-100: the chunk is dropped
    if (n > buf_size) {                               // Vec::drain(..n) would panic
        pvq::set_last_error("chunk longer than the ring buffer");
        return PVQ_ERR_BAD_LENGTH;
    }
    PVQ_HIP(hipSetDevice(vqt->device()));
    if (in_flight) {   // a second push before the previous one's copy was waited for (no frame in between)
        PVQ_HIP(hipStreamSynchronize(stream));
        in_flight = false;
    }
    std::copy(data, data + n, h_in);
    if (with_agc) {
        float sq = 0.0f;
        for (size_t i = 0; i < n; ++i) sq += data[i] * data[i];     // audio_desktop.rs:101
        agc.freeze_gain(sq < 1e-6f);                                // :102
        agc.process(h_in, n);                                       // :111 (over the newest samples of the ring)
        gain_ = agc.gain();                                         // :112
    }
    if (w + n > cap) {   // compact: newest buf_size samples to the front (ranges do not overlap: cap = 4 buf_size)
        PVQ_HIP(hipMemcpyAsync(d_ring, d_ring + w - buf_size, buf_size * sizeof(float), hipMemcpyDeviceToDevice, stream));
        w = buf_size;
    }
    PVQ_HIP(hipMemcpyAsync(d_ring + w, h_in, n * sizeof(float), hipMemcpyHostToDevice, stream));
    in_flight = true;
    w += n;
    chunk_size_ms_ = static_cast<float>(n) / vqt->params().sr * 1000.0f;   // :118
    return PVQ_OK;
}

pvq_status LiveStream::frame_db(float* out_db) {
    const size_t n_fft = vqt->params().n_fft;
    // one frame over the newest n_fft samples: n_lead = n_fft - 1 samples of history + a hop of 1
    pvq_status st = vqt->calculate_batch_db_device(d_ring + w - n_fft, n_fft - 1, 1, 1, d_db, nullptr, stream);
    if (st != PVQ_OK) return st;
    const size_t nb = vqt->n_bins();
    PVQ_HIP(hipMemcpyAsync(h_out, d_db, nb * sizeof(float), hipMemcpyDeviceToHost, stream));
    PVQ_HIP(hipStreamSynchronize(stream));
    in_flight = false;
    std::copy(h_out, h_out + nb, out_db);
    return PVQ_OK;
}

pvq_status LiveStream::read(float* out, size_t n_last) {
    if (n_last > buf_size) {
        pvq::set_last_error("n_last exceeds the ring buffer");
        return PVQ_ERR_BAD_LENGTH;
    }
    PVQ_HIP(hipSetDevice(vqt->device()));
    PVQ_HIP(hipStreamSynchronize(stream));   // the appends queued on the object's stream
    in_flight = false;
    PVQ_HIP(hipMemcpy(out, d_ring + w - n_last, n_last * sizeof(float), hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
