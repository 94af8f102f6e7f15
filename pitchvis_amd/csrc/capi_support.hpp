// capi_support.hpp — what every unit of the extern "C" surface (capi_*.cpp over include/pvq.h) needs, once: the opaque handle
// structs, the exception barrier, the common constructor and destructor.  Private to the library: not installed.
#pragma once

#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/pvq.h"
#include "consumers_host.hpp"   // the three handles that hold their object by value: MonoAgc,
#include "device_support.hpp"
#include "overlay_host.hpp"     // OverlayState,
#include "panels_host.hpp"      // CalmnessGraph
#include "vqt_host.hpp"

namespace pvq {   // every other handle holds a pointer: the unit that makes and destroys one includes its stage's header
class Vqt;
class AnalysisState;
class AnalysisBatch;
class AgcBatch;
class LiveStream;
class RenderBatch;
class SceneState;
class SceneBatch;
class RasterBatch;
class BackdropBatch;
class OverlayBatch;
class TextFont;
class TextBatch;
class ReadoutBatch;
class SynthBank;
class SynthState;
class SynthBatch;
class SynthEffects;
class PresentBatch;
class PanelsBatch;
class NoteModel;
class NoteCarry;
class NoteTrainer;
}  // namespace pvq

struct pvq_vqt {
    std::unique_ptr<pvq::Vqt> impl;
};
struct pvq_analysis_state {
    std::unique_ptr<pvq::AnalysisState> impl;
};
struct pvq_analysis_batch {
    std::unique_ptr<pvq::AnalysisBatch> impl;
};
struct pvq_mono_agc {
    pvq::MonoAgc impl;
};
struct pvq_agc_batch {
    std::unique_ptr<pvq::AgcBatch> impl;
};
struct pvq_stream {
    std::unique_ptr<pvq::LiveStream> impl;
};
struct pvq_render_batch {
    std::unique_ptr<pvq::RenderBatch> impl;
};
struct pvq_scene_state {
    std::unique_ptr<pvq::SceneState> impl;
};
struct pvq_scene_batch {
    std::unique_ptr<pvq::SceneBatch> impl;
};
struct pvq_raster_batch {
    std::unique_ptr<pvq::RasterBatch> impl;
};
struct pvq_backdrop_batch {
    std::unique_ptr<pvq::BackdropBatch> impl;
};
struct pvq_overlay_state {
    pvq::OverlayState impl;
};
struct pvq_overlay_batch {
    std::unique_ptr<pvq::OverlayBatch> impl;
};
struct pvq_text_font {
    std::unique_ptr<pvq::TextFont> impl;
};
struct pvq_text_batch {
    std::unique_ptr<pvq::TextBatch> impl;
};
struct pvq_readout_batch_s {
    std::unique_ptr<pvq::ReadoutBatch> impl;
};
struct pvq_synth_bank {
    std::shared_ptr<const pvq::SynthBank> impl;
};
struct pvq_synth_state {
    std::unique_ptr<pvq::SynthState> impl;
};
struct pvq_synth_batch {
    std::unique_ptr<pvq::SynthBatch> impl;
};
struct pvq_synth_effects_s {
    std::unique_ptr<pvq::SynthEffects> impl;
};
struct pvq_present_batch {
    std::unique_ptr<pvq::PresentBatch> impl;
};
struct pvq_calmness_graph {
    pvq::CalmnessGraph impl;
};
struct pvq_panels_batch {
    std::unique_ptr<pvq::PanelsBatch> impl;
};
struct pvq_note_model {
    std::unique_ptr<pvq::NoteModel> impl;
};
struct pvq_note_carry {
    std::unique_ptr<pvq::NoteCarry> impl;
};
struct pvq_note_trainer {
    std::unique_ptr<pvq::NoteTrainer> impl;
};

namespace {
inline pvq_status null_handle() {
    pvq::set_last_error("null handle");
    return PVQ_ERR_INVALID_ARG;
}
inline pvq_status invalid_arg(const std::string& text) {
    pvq::set_last_error(text);
    return PVQ_ERR_INVALID_ARG;
}
// include/pvq.h: "no exceptions cross the ABI".  Every extern "C" body runs inside guarded() below and lands here:
// a PanicError (the reference's assert! / expect texts, vqt.rs:785-792) becomes PVQ_ERR_INVALID_ARG, anything else
// (std::bad_alloc from a table or staging vector, std::length_error, ...) PVQ_ERR_INTERNAL; the text goes to pvq_last_error.
inline pvq_status translate_exception() noexcept {
    try {
        throw;
    } catch (const pvq::PanicError& e) {
        pvq::set_last_error_noexcept(e.what());
        return PVQ_ERR_INVALID_ARG;
    } catch (const std::bad_alloc&) {
        pvq::set_last_error_noexcept("out of host memory");
        return PVQ_ERR_INTERNAL;
    } catch (const std::exception& e) {
        pvq::set_last_error_noexcept(e.what());
        return PVQ_ERR_INTERNAL;
    } catch (...) {
        pvq::set_last_error_noexcept("unknown exception");
        return PVQ_ERR_INTERNAL;
    }
}
// The barrier.  A body that returns pvq_status answers with the translated status, a void body returns;
template <class Body>
auto guarded(Body&& body) noexcept -> decltype(body()) {
    try {
        return body();
    } catch (...) {
        if constexpr (std::is_void_v<decltype(body())>)
            (void)translate_exception();
        else
            return translate_exception();
    }
}
// a getter answers with the value it gives for a null handle: 0, 0.0f, nullptr, PVQ_ALGO_AUTO.
template <class T, class Body>
auto guarded(T fallback, Body&& body) noexcept -> decltype(body()) {
    try {
        return body();
    } catch (...) {
        (void)translate_exception();
        return fallback;
    }
}
// The common constructor, to be called inside guarded(): a null `out` is refused, *out is cleared, create(impl) is the stage's own
// create (with whatever the entry point checks after clearing *out), and the handle is made on PVQ_OK.
template <class Handle, class Create>
pvq_status make_handle(Handle** out, Create&& create) {
    if (!out) return null_handle();
    *out = nullptr;
    decltype(Handle::impl) impl;
    const pvq_status st = create(impl);
    if (st != PVQ_OK) return st;
    *out = new Handle{std::move(impl)};
    return PVQ_OK;
}
template <class Handle>
void destroy(Handle* h) noexcept {
    guarded([&] { delete h; });
}
}  // namespace
