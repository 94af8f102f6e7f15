// multi_batch.hip — the multi-device driver: one stream of host PCM analysed on several pvq::Vqt handles at once, a host thread per
// handle (analyze_batch_multi, its handle checks, and the handle's shard buffers Vqt::multi_buffers).  No kernel: this unit only calls
// the HIP runtime and the handles' device entry points (vqt_engine.hip).  Shard geometry: multi_host.hpp.
#include "vqt_engine.hpp"

#include <cstring>
#include <string>
#include <thread>

namespace pvq {

namespace {
struct MultiBuf {   // (a view of one of the handle's shard buffers)
    void* p = nullptr;
    template <typename T> T* as() { return static_cast<T*>(p); }
};
}  // namespace

// A handle's shard resources for the multi-device driver: one stream and six grow-only device buffers, kept between calls (a call per
// shard used to pay a hipStreamCreate and up to six hipMalloc / hipFree: milliseconds, and every hipFree synchronises the device).
pvq_status Vqt::multi_buffers(const size_t (&bytes)[6], void* (&out)[6], hipStream_t* st) {
    if (!multi_stream_) PVQ_HIP(hipStreamCreateWithFlags(&multi_stream_, hipStreamNonBlocking));
    for (int i = 0; i < 6; ++i) {
        if (bytes[i] == 0) {
            out[i] = nullptr;
            continue;
        }
        pvq_status e = multi_buf_[i].reserve(bytes[i]);
        if (e != PVQ_OK) return e;
        out[i] = multi_buf_[i].as<void>();
    }
    *st = multi_stream_;
    return PVQ_OK;
}

// every handle present, on a device, passed once, of the same parameters
static pvq_status check_multi_handles(Vqt* const* handles, uint32_t n_handles) {
    for (uint32_t g = 0; g < n_handles; ++g) {
        if (!handles[g]) {
            set_last_error("analyze_batch_multi: null handle");
            return PVQ_ERR_INVALID_ARG;
        }
        if (pvq_status ds = handles[g]->require_device(); ds != PVQ_OK) return ds;
        for (uint32_t h = 0; h < g; ++h)
            if (handles[h] == handles[g]) {
                set_last_error("analyze_batch_multi: a handle is exclusive to one worker; the same handle was passed twice");
                return PVQ_ERR_INVALID_ARG;
            }
        const VqtParameters &p0 = handles[0]->params(), &pg = handles[g]->params();
        if (std::memcmp(&p0, &pg, sizeof(VqtParameters)) != 0) {
            set_last_error("analyze_batch_multi: the handles were created with different parameters");
            return PVQ_ERR_INVALID_ARG;
        }
    }
    return PVQ_OK;
}

pvq_status analyze_batch_multi(Vqt* const* handles, uint32_t n_handles, const float* pcm, size_t n_lead, size_t hop, size_t n_frames,
                               const AnalysisParameters& ap, float* out_db, uint32_t* peak_mask, uint32_t* peak_count, float* center,
                               float* size, uint32_t max_peaks) {
    if (!handles || n_handles == 0) {
        set_last_error("analyze_batch_multi: no handles");
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_frames == 0) return PVQ_OK;
    if (!pcm || !out_db || hop == 0) {
        set_last_error("analyze_batch_multi: null pointer or zero hop");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((center != nullptr) != (size != nullptr) || (center && max_peaks == 0)) {
        set_last_error("analyze_batch_multi: center and size go together, with max_peaks > 0");
        return PVQ_ERR_INVALID_ARG;
    }
    if (pvq_status hs = check_multi_handles(handles, n_handles); hs != PVQ_OK) return hs;
    const size_t nb = handles[0]->n_bins(), words = (nb + 31) / 32;
    const size_t wu = handles[0]->plan().window_union;
    const bool want_peaks = peak_mask || peak_count || center;
    // one decision for the whole stream (what ONE handle would do with it), applied to every shard
    if (hipSetDevice(handles[0]->device()) != hipSuccess) {
        set_last_error("hipSetDevice failed");
        return PVQ_ERR_DEVICE;
    }
    const pvq_algo whole = handles[0]->resolve_algo(hop, n_frames);
    std::vector<pvq_status> status(n_handles, PVQ_OK);
    std::vector<std::string> message(n_handles);
    auto work = [&](uint32_t g) {
        // the worker's error text is thread-local: hand it back with the status
        auto fail = [&](pvq_status st, const std::string& msg) {
            status[g] = st;
            message[g] = msg;
        };
        try {
            ShardPlan sh;
            if (!plan_shard(n_frames, hop, wu, g, n_handles, &sh)) return fail(PVQ_ERR_INTERNAL, "plan_shard failed");
            if (sh.n_frames == 0) return;
            // plan_shard counts samples from the stream's first hop; the caller's array starts n_lead samples earlier, and a shard's
            // halo may reach into that history
            const size_t hop_begin = n_lead + (size_t)sh.first_frame * hop;
            const size_t halo = wu > hop ? wu - hop : 0;
            const size_t begin = hop_begin > halo ? hop_begin - halo : 0;
            const size_t lead = hop_begin - begin, n_samp = lead + (size_t)sh.n_frames * hop, nf = (size_t)sh.n_frames;
            Vqt* v = handles[g];
            if (hipSetDevice(v->device()) != hipSuccess) return fail(PVQ_ERR_DEVICE, "hipSetDevice failed");
            // the handle's own stream and grow-only shard buffers (kept between calls); with page-locked caller arrays (pvq_host_alloc)
            // the copies below are asynchronous DMA, with pageable ones the runtime stages them
            MultiBuf d_pcm, d_db, d_mask, d_count, d_center, d_size;
            hipStream_t st = nullptr;
            {
                const size_t bytes[6] = {n_samp * 4, nf * nb * 4, want_peaks ? nf * words * 4 : 0, want_peaks ? nf * 4 : 0,
                                         center ? nf * max_peaks * 4 : 0, center ? nf * max_peaks * 4 : 0};
                void* ptrs[6];
                const pvq_status bs = v->multi_buffers(bytes, ptrs, &st);
                if (bs != PVQ_OK) return fail(bs, get_last_error());
                d_pcm.p = ptrs[0]; d_db.p = ptrs[1]; d_mask.p = ptrs[2]; d_count.p = ptrs[3]; d_center.p = ptrs[4]; d_size.p = ptrs[5];
            }
            if (hipMemcpyAsync(d_pcm.p, pcm + begin, n_samp * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(PVQ_ERR_DEVICE, "upload failed");
            if (center) {   // entries beyond a frame's count are left as the caller passed them: start from the caller's contents
                const size_t off = (size_t)sh.first_frame * max_peaks;
                if (hipMemcpyAsync(d_center.p, center + off, nf * max_peaks * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
                    hipMemcpyAsync(d_size.p, size + off, nf * max_peaks * 4, hipMemcpyHostToDevice, st) != hipSuccess)
                    return fail(PVQ_ERR_DEVICE, "upload failed");
            }
            pvq_status rs;
            const pvq_algo own = v->algo();
            v->set_algo(whole);
            if (want_peaks)
                rs = v->vqt_analyze_batch_device(d_pcm.as<float>(), lead, hop, nf, ap, d_db.as<float>(), d_mask.as<uint32_t>(), d_count.as<uint32_t>(),
                                                 center ? d_center.as<float>() : nullptr, center ? d_size.as<float>() : nullptr, max_peaks, st);
            else
                rs = v->calculate_batch_db_device(d_pcm.as<float>(), lead, hop, nf, d_db.as<float>(), nullptr, st);
            v->set_algo(own);
            if (rs != PVQ_OK) return fail(rs, get_last_error());
            const size_t f0 = (size_t)sh.first_frame;
            bool cp = hipMemcpyAsync(out_db + f0 * nb, d_db.p, nf * nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (cp && peak_mask) cp = hipMemcpyAsync(peak_mask + f0 * words, d_mask.p, nf * words * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (cp && peak_count) cp = hipMemcpyAsync(peak_count + f0, d_count.p, nf * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (cp && center)
                cp = hipMemcpyAsync(center + f0 * max_peaks, d_center.p, nf * max_peaks * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
                     hipMemcpyAsync(size + f0 * max_peaks, d_size.p, nf * max_peaks * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (!cp || hipStreamSynchronize(st) != hipSuccess) return fail(PVQ_ERR_DEVICE, "download failed");
            rs = v->input_status(st);
            if (rs != PVQ_OK) return fail(rs, get_last_error());
        } catch (const std::bad_alloc&) {
            fail(PVQ_ERR_INTERNAL, "out of host memory");
        } catch (const std::exception& e) {
            fail(PVQ_ERR_INTERNAL, e.what());
        } catch (...) {
            fail(PVQ_ERR_INTERNAL, "unknown exception in a shard worker");
        }
    };
    std::vector<std::thread> threads;
    threads.reserve(n_handles);
    for (uint32_t g = 1; g < n_handles; ++g) threads.emplace_back(work, g);
    work(0);
    for (auto& t : threads) t.join();
    for (uint32_t g = 0; g < n_handles; ++g)
        if (status[g] != PVQ_OK) {
            set_last_error("shard " + std::to_string(g) + ": " + message[g]);
            return status[g];
        }
    return PVQ_OK;
}

}  // namespace pvq
