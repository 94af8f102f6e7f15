// capi_consumers.cpp — extern "C" surface of libpvq (include/pvq.h): mono AGC, training helpers, AGC batch, .npy, the live front end,
// pinned host memory, colour / LED.
#include <string>

#include "capi_support.hpp"
#include "condition_batch.hpp"
#include "consumers_host.hpp"
#include "live_stream.hpp"
#include "vqt_engine.hpp"

extern "C" {

// ------------------------------------------------------------------------------------------------
// callers either side of the path
// ------------------------------------------------------------------------------------------------
pvq_status pvq_mono_agc_create(float desired_output_rms, float distortion_factor, pvq_mono_agc** out) {
    return guarded([&] {
        if (!out) return null_handle();
        *out = nullptr;
        std::string why;
        if (!pvq::MonoAgc::valid(desired_output_rms, distortion_factor, &why)) return invalid_arg(why);
        *out = new pvq_mono_agc{pvq::MonoAgc(desired_output_rms, distortion_factor)};
        return PVQ_OK;
    });
}
void pvq_mono_agc_destroy(pvq_mono_agc* a) { destroy(a); }
void pvq_mono_agc_freeze_gain(pvq_mono_agc* a, int freeze) {
    guarded([&] {
        if (a) a->impl.freeze_gain(freeze != 0);
    });
}
int pvq_mono_agc_is_gain_frozen(const pvq_mono_agc* a) {
    return guarded(0, [&] {
        return a && a->impl.is_gain_frozen() ? 1 : 0;
    });
}
float pvq_mono_agc_gain(const pvq_mono_agc* a) {
    return guarded(0.0f, [&] {
        return a ? a->impl.gain() : 0.0f;
    });
}
void pvq_mono_agc_process(pvq_mono_agc* a, float* samples, size_t n) {
    guarded([&] {
        if (a && samples) a->impl.process(samples, n);
    });
}

size_t pvq_train_chunk_samples(const pvq_vqt* v) {
    return guarded(0, [&] {
        return v ? pvq::train_chunk_samples(v->impl->delay_seconds(), v->impl->params().sr) : 0;
    });
}
pvq_status pvq_train_condition_stream(pvq_mono_agc* a, const float* left, const float* right, size_t n_chunks, size_t chunk,
                                      float* mono_out, float* gain_out) {
    return guarded([&] {
        if (!a || !left || !mono_out) return null_handle();
        pvq::train_condition_stream(a->impl, left, right, n_chunks, chunk, mono_out, gain_out);
        return PVQ_OK;
    });
}
// train.rs:146-163 + 286-301: the conditioning of many files side by side, on the device (condition_batch.hpp)
pvq_status pvq_agc_batch_create(int device_id, uint32_t n_streams, float desired_output_rms, float distortion_factor, pvq_agc_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::AgcBatch::create(device_id, n_streams, desired_output_rms, distortion_factor, impl);   // lib.rs:35-53
        });
    });
}
void pvq_agc_batch_destroy(pvq_agc_batch* b) { destroy(b); }
pvq_status pvq_agc_batch_condition_device(pvq_agc_batch* b, const float* const* d_left, const float* const* d_right, const size_t* n_chunks,
                                          size_t chunk, float* const* d_mono_out, float* d_gain_out, size_t gain_stride, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->condition_device(d_left, d_right, n_chunks, chunk, d_mono_out, d_gain_out, gain_stride,
                                         static_cast<hipStream_t>(stream));   // train.rs:286-301
    });
}
pvq_status pvq_agc_batch_get_gains(pvq_agc_batch* b, float* gains) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->get_gains(gains);   // lib.rs:72
    });
}
pvq_status pvq_train_frames_db(pvq_vqt* v, const float* mono, size_t n_chunks, size_t chunk, size_t step, float* out_db) {
    return guarded([&] {
        if (!v || !mono || !out_db) return null_handle();
        if (chunk == 0 || step == 0) return invalid_arg("chunk and step must be positive");
        const size_t n_frames = n_chunks / step;
        if (n_frames == 0) return PVQ_OK;
        return v->impl->calculate_batch_db(mono, 0, chunk * step, n_frames, out_db);
    });
}
pvq_status pvq_train_rows(const float* db, size_t n_frames, uint32_t n_bins, const uint32_t* voice_ptr, const int32_t* voice_key,
                          const float* voice_gain_left, const float* voice_gain_right, const float* agc_gain, float* out_rows) {
    return guarded([&] {
        if (!db || !voice_ptr || !agc_gain || !out_rows) return null_handle();
        std::string why;
        if (!pvq::train_rows(db, n_frames, n_bins, voice_ptr, voice_key, voice_gain_left, voice_gain_right, agc_gain, out_rows, &why))
            return invalid_arg(why);
        return PVQ_OK;
    });
}
pvq_status pvq_npy_write_f32(const char* path, const float* data, uint64_t n) {
    return guarded([&] {
        if (!path || (!data && n)) return null_handle();
        std::string why;
        if (!pvq::npy_write_f32(path, data, n, &why)) return invalid_arg(why);
        return PVQ_OK;
    });
}

pvq_status pvq_stream_create(pvq_vqt* v, size_t buf_size, int with_agc, pvq_stream** out) {
    return guarded([&] {
        if (!v) return null_handle();
        return make_handle(out, [&](auto& impl) { return pvq::LiveStream::create(v->impl.get(), buf_size, with_agc != 0, impl); });
    });
}
void pvq_stream_destroy(pvq_stream* s) { destroy(s); }
pvq_status pvq_stream_push(pvq_stream* s, const float* data, size_t n) {
    return guarded([&] {
        if (!s || (!data && n)) return null_handle();
        return s->impl->push(data, n);
    });
}
float pvq_stream_gain(const pvq_stream* s) {
    return guarded(0.0f, [&] {
        return s ? s->impl->gain() : 0.0f;
    });
}
float pvq_stream_chunk_size_ms(const pvq_stream* s) {
    return guarded(0.0f, [&] {
        return s ? s->impl->chunk_size_ms() : 0.0f;
    });
}
pvq_status pvq_stream_frame_db(pvq_stream* s, float* out_db) {
    return guarded([&] {
        if (!s || !out_db) return null_handle();
        return s->impl->frame_db(out_db);
    });
}
pvq_status pvq_stream_read(pvq_stream* s, float* out, size_t n_last) {
    return guarded([&] {
        if (!s || !out) return null_handle();
        return s->impl->read(out, n_last);
    });
}

void* pvq_host_alloc(size_t bytes) {
    return guarded(nullptr, [&]() -> void* {
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
        if (e != hipSuccess) {
            pvq::set_last_error(std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
            return nullptr;
        }
        return p;
    });
}
void pvq_host_free(void* p) {
    guarded([&] {
        if (p) (void)hipHostFree(p);
    });
}

void pvq_calculate_color(uint16_t buckets_per_octave, float bucket, const float* colors, float gray_level, float easing_pow,
                         float out_rgb[3]) {
    guarded([&] {
        pvq::calculate_color(buckets_per_octave, bucket, reinterpret_cast<const float(*)[3]>(colors), gray_level, easing_pow, out_rgb);
    });
}
size_t pvq_led_frame(uint32_t n_buckets, uint16_t buckets_per_octave, const float* center, const float* size, uint32_t n_peaks,
                     const float* colors, float gray_level, float easing_pow, uint8_t* out) {
    return guarded(0, [&] {
        return pvq::led_frame(n_buckets, buckets_per_octave, center, size, n_peaks, reinterpret_cast<const float(*)[3]>(colors),
                              gray_level, easing_pow, out);
    });
}

}  // extern "C"
