// capi_present.cpp — extern "C" surface of libpvq (include/pvq.h): bloom, display transform and sRGB bytes.
#include <string>

#include "capi_support.hpp"
#include "present_batch.hpp"
#include "present_host.hpp"
#include "stage_plan.hpp"

extern "C" {

// Bloom, display transform and sRGB bytes (setup.rs:347-383, update.rs:346-347): one picture on the host (present_host.hpp) and many
// on the device (present_batch.hpp)
namespace {
pvq::present::Settings present_settings(const pvq_present_settings* s) {
    if (!s) return pvq::present::default_settings();
    return pvq::present::Settings{s->low_frequency_boost, s->low_frequency_boost_curvature, s->high_pass_frequency, s->threshold,
                                  s->threshold_softness,  s->composite_mode,                s->max_mip_dimension,   s->tonemapping};
}
}  // namespace
void pvq_present_default_settings(pvq_present_settings* s) {
    guarded([&] {
        if (!s) return;
        const pvq::present::Settings d = pvq::present::default_settings();
        *s = pvq_present_settings{d.low_frequency_boost, d.low_frequency_boost_curvature, d.high_pass_frequency, d.threshold,
                                  d.threshold_softness,  d.composite_mode,                d.max_mip_dimension,   d.tonemapping};
    });
}
pvq_status pvq_present_mips(uint32_t width, uint32_t height, uint32_t max_mip_dimension, uint32_t* out_count, uint32_t* out_sizes) {
    return guarded([&] {
        std::string err;
        pvq::present::Settings s = pvq::present::default_settings();
        s.max_mip_dimension = max_mip_dimension;
        if (!pvq::stage_image_ok("present mips", width, height, 0.0f, err) || !pvq::present_settings_ok("present mips", s, err))
            return invalid_arg(err);
        pvq::PresentPlan plan;
        if (!pvq::present_plan("present mips", width, height, pvq::present_resolved(s).max_mip_dimension, plan, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_UNSUPPORTED;
        }
        if (out_count) *out_count = plan.mips.n;
        if (out_sizes)
            for (uint32_t k = 0; k < plan.mips.n; ++k) {
                out_sizes[2 * k] = plan.mips.w[k];
                out_sizes[2 * k + 1] = plan.mips.h[k];
            }
        return PVQ_OK;
    });
}
pvq_status pvq_present_blend_factors(const pvq_present_settings* settings, float intensity, uint32_t n_mips, float* out) {
    return guarded([&] {
        std::string err;
        const pvq::present::Settings s = present_settings(settings);
        if (!out || n_mips == 0 || n_mips > pvq::present::MAX_MIPS) return invalid_arg("present blend factors: out is needed, and n_mips 1 .. 11");
        if (!pvq::present_settings_ok("present blend factors", s, err)) return invalid_arg(err);
        pvq::present_blend_factors(s, intensity, n_mips, out);
        return PVQ_OK;
    });
}
pvq_status pvq_present_frame(const pvq_present_settings* settings, uint32_t width, uint32_t height, const float* image, float intensity,
                             uint8_t* out_rgba8, float* out_hdr) {
    return guarded([&] {
        if (!image || !out_rgba8) return invalid_arg("present frame: image and out_rgba8 are needed");
        std::string err;
        const pvq::present::Settings raw = present_settings(settings);
        if (!pvq::stage_image_ok("present frame", width, height, 0.0f, err) || !pvq::present_settings_ok("present frame", raw, err))
            return invalid_arg(err);
        const pvq::present::Settings s = pvq::present_resolved(raw);
        pvq::PresentPlan plan;
        if (!pvq::present_plan("present frame", width, height, s.max_mip_dimension, plan, err)) {
            pvq::set_last_error(err);
            return PVQ_ERR_UNSUPPORTED;
        }
        pvq::present_frame(s, plan, width, height, image, intensity, out_rgba8, out_hdr);
        return PVQ_OK;
    });
}
pvq_status pvq_present_batch_create(int device_id, const pvq_present_settings* settings, uint32_t width, uint32_t height, pvq_present_batch** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            return pvq::PresentBatch::create(device_id, present_settings(settings), width, height, impl);
        });
    });
}
void pvq_present_batch_destroy(pvq_present_batch* b) { destroy(b); }
pvq_status pvq_present_batch_set_workspace_limit(pvq_present_batch* b, uint64_t bytes) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->set_workspace_limit(bytes);
    });
}
pvq_status pvq_present_batch_rows_device(pvq_present_batch* b, size_t n_rows, const float* d_image, const float* d_intensity, uint8_t* d_rgba8,
                                         float* d_hdr, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->rows_device(n_rows, d_image, d_intensity, d_rgba8, d_hdr, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
