// capi_synth.cpp — extern "C" surface of libpvq (include/pvq.h): the synthesizer: bank, state, batch.
#include <cstring>
#include <string>
#include <vector>

#include "capi_support.hpp"
#include "synth_batch.hpp"
#include "synth_host.hpp"

extern "C" {

// The synthesizer (rustysynth_fork; the dry path, or with PVQ_SYNTH_EFFECTS its reverb and chorus too): the bank, one stream on the
// host (synth_host.hpp) and many on the device (synth_batch.hpp), and the effects alone on the host
namespace {
static_assert(sizeof(pvq_synth_record) == sizeof(pvq::synth::Record), "one layout");
static_assert(sizeof(pvq_synth_sends) == sizeof(pvq::synth::Sends), "one layout");
pvq_status synth_flags(uint32_t flags, bool& effects) {
    if (flags & ~static_cast<uint32_t>(PVQ_SYNTH_EFFECTS)) return invalid_arg("synth: unknown flag bits (PVQ_SYNTH_EFFECTS is the only flag)");
    effects = (flags & PVQ_SYNTH_EFFECTS) != 0;
    return PVQ_OK;
}
pvq_status synth_state_make(const pvq_synth_bank* bank, int32_t sample_rate, uint32_t maximum_polyphony, uint32_t flags, pvq_synth_state** out) {
    if (!out) return null_handle();
    *out = nullptr;
    if (!bank) return null_handle();
    bool effects = false;
    if (pvq_status st = synth_flags(flags, effects)) return st;
    std::unique_ptr<pvq::SynthState> impl;
    std::string err;
    const pvq_status st = pvq::SynthState::create(bank->impl, sample_rate, maximum_polyphony, impl, err, effects);   // synthesizer.rs:58-174
    if (st != PVQ_OK) {
        pvq::set_last_error(err);
        return st;
    }
    *out = new pvq_synth_state{std::move(impl)};
    return PVQ_OK;
}
pvq_status synth_batch_make(int device_id, const pvq_synth_bank* bank, uint32_t n_streams, int32_t sample_rate, uint32_t maximum_polyphony, uint32_t flags,
                            pvq_synth_batch** out) {
    return make_handle(out, [&](auto& impl) {
        if (!bank) return null_handle();
        bool effects = false;
        if (pvq_status st = synth_flags(flags, effects)) return st;
        return pvq::SynthBatch::create(device_id, bank->impl, n_streams, sample_rate, maximum_polyphony, impl, effects);   // synthesizer.rs:58-174
    });
}
pvq_status synth_snapshots_out(const pvq::SynthPlan& p, uint32_t* out_counts, uint32_t* voice_ptr, size_t ptr_capacity, int32_t* key, float* gain_left,
                               float* gain_right, size_t capacity) {
    const size_t n_snap = p.snapshot_ptr.empty() ? 0 : p.snapshot_ptr.size() - 1, n_voices = p.snapshots.size();
    if (out_counts) {
        out_counts[0] = static_cast<uint32_t>(n_snap);
        out_counts[1] = static_cast<uint32_t>(n_voices);
    }
    if (!voice_ptr && !key && !gain_left && !gain_right) return PVQ_OK;
    if (!voice_ptr || !key || !gain_left || !gain_right || ptr_capacity < n_snap + 1 || capacity < n_voices)
        return invalid_arg("synth snapshots: all four arrays are needed, voice_ptr of snapshots + 1 and the others of as many entries as there are voices");
    for (size_t k = 0; k <= n_snap; ++k) voice_ptr[k] = p.snapshot_ptr.empty() ? 0u : p.snapshot_ptr[k];
    for (size_t k = 0; k < n_voices; ++k) {
        key[k] = p.snapshots[k].key;
        gain_left[k] = p.snapshots[k].current_mix_gain_left;
        gain_right[k] = p.snapshots[k].current_mix_gain_right;
    }
    return PVQ_OK;
}
}  // namespace
pvq_status pvq_synth_bank_create(const int16_t* wave_data, size_t n_wave, const int32_t* samples, uint32_t n_samples, const int16_t* instrument_gs,
                                 const uint32_t* instrument_sample, uint32_t n_instrument_regions, const uint32_t* instruments, uint32_t n_instruments,
                                 const int16_t* preset_gs, const uint32_t* preset_instrument, uint32_t n_preset_regions, const int32_t* presets,
                                 uint32_t n_presets, pvq_synth_bank** out) {
    return guarded([&] {
        if (!out) return null_handle();
        *out = nullptr;
        std::shared_ptr<const pvq::SynthBank> impl;
        std::string err;
        const pvq_status st = pvq::SynthBank::create(wave_data, n_wave, samples, n_samples, instrument_gs, instrument_sample, n_instrument_regions,
                                                     instruments, n_instruments, preset_gs, preset_instrument, n_preset_regions, presets, n_presets, impl,
                                                     err);   // soundfont.rs, instrument_region.rs:33-87, preset_region.rs:26-53
        if (st != PVQ_OK) {
            pvq::set_last_error(err);
            return st;
        }
        *out = new pvq_synth_bank{std::move(impl)};
        return PVQ_OK;
    });
}
void pvq_synth_bank_destroy(pvq_synth_bank* b) { destroy(b); }
pvq_status pvq_synth_bank_counts(const pvq_synth_bank* b, uint64_t* out4) {
    return guarded([&] {
        if (!b || !out4) return null_handle();
        out4[0] = b->impl->wave.size();
        out4[1] = b->impl->iregions.size();
        out4[2] = b->impl->pregions.size();
        out4[3] = b->impl->presets.size();
        return PVQ_OK;
    });
}
pvq_status pvq_synth_state_create(const pvq_synth_bank* bank, int32_t sample_rate, uint32_t maximum_polyphony, pvq_synth_state** out) {
    return guarded([&] { return synth_state_make(bank, sample_rate, maximum_polyphony, 0, out); });
}
pvq_status pvq_synth_state_create_ex(const pvq_synth_bank* bank, int32_t sample_rate, uint32_t maximum_polyphony, uint32_t flags, pvq_synth_state** out) {
    return guarded([&] { return synth_state_make(bank, sample_rate, maximum_polyphony, flags, out); });
}
void pvq_synth_state_destroy(pvq_synth_state* s) { destroy(s); }
pvq_status pvq_synth_state_render(pvq_synth_state* s, const double* time_s, const int32_t* channel, const int32_t* command, const int32_t* data1,
                                  const int32_t* data2, size_t n_events, size_t n_blocks, const uint32_t* snapshot_blocks, size_t n_snapshots, float* left,
                                  float* right) {
    return guarded([&] {
        if (!s) return null_handle();
        std::string err;
        const pvq::SynthEvents ev{time_s, channel, command, data1, data2, n_events};
        const pvq_status st = s->impl->render(ev, n_blocks, snapshot_blocks, n_snapshots, left, right, err);   // midifile_sequencer.rs:52-104
        if (st != PVQ_OK) pvq::set_last_error(err);
        return st;
    });
}
pvq_status pvq_synth_state_get_snapshots(const pvq_synth_state* s, uint32_t* out_counts, uint32_t* voice_ptr, size_t ptr_capacity, int32_t* key,
                                         float* gain_left, float* gain_right, size_t capacity) {
    return guarded([&] {
        if (!s) return null_handle();
        return synth_snapshots_out(s->impl->last_plan(), out_counts, voice_ptr, ptr_capacity, key, gain_left, gain_right, capacity);   // synthesizer.rs:525
    });
}
pvq_status pvq_synth_state_get_plan(const pvq_synth_state* s, uint32_t* out_counts, uint32_t* block_ptr, size_t ptr_capacity, pvq_synth_record* records,
                                    size_t capacity) {
    return guarded([&] {
        if (!s) return null_handle();
        const pvq::SynthPlan& p = s->impl->last_plan();
        const size_t n_blocks = p.block_ptr.empty() ? 0 : p.block_ptr.size() - 1, n_records = p.records.size();
        if (out_counts) {
            out_counts[0] = static_cast<uint32_t>(n_blocks);
            out_counts[1] = static_cast<uint32_t>(n_records);
        }
        if (!block_ptr && !records) return PVQ_OK;
        if (!block_ptr || !records || ptr_capacity < n_blocks + 1 || capacity < n_records)
            return invalid_arg("synth plan: block_ptr of blocks + 1 entries and records of as many as the plan holds are needed");
        for (size_t k = 0; k <= n_blocks; ++k) block_ptr[k] = p.block_ptr.empty() ? 0u : p.block_ptr[k];
        if (n_records) std::memcpy(records, p.records.data(), n_records * sizeof(pvq_synth_record));
        return PVQ_OK;
    });
}
pvq_status pvq_synth_state_get_sends(const pvq_synth_state* s, uint32_t* out_counts, uint32_t* block_ptr, size_t ptr_capacity, pvq_synth_sends* sends,
                                     size_t capacity) {
    return guarded([&] {
        if (!s) return null_handle();
        const pvq::SynthPlan& p = s->impl->last_plan();
        const bool fx = s->impl->effects();
        const size_t n_blocks = !fx || p.block_ptr.empty() ? 0 : p.block_ptr.size() - 1, n_sends = fx ? p.sends.size() : 0;
        if (out_counts) {
            out_counts[0] = static_cast<uint32_t>(n_blocks);
            out_counts[1] = static_cast<uint32_t>(n_sends);
        }
        if (!block_ptr && !sends) return PVQ_OK;
        if (!block_ptr || !sends || ptr_capacity < n_blocks + 1 || capacity < n_sends)
            return invalid_arg("synth sends: block_ptr of blocks + 1 entries and sends of as many as the plan holds are needed");
        for (size_t k = 0; k <= n_blocks; ++k) block_ptr[k] = fx && !p.block_ptr.empty() ? p.block_ptr[k] : 0u;
        if (n_sends) std::memcpy(sends, p.sends.data(), n_sends * sizeof(pvq_synth_sends));
        return PVQ_OK;
    });
}
uint32_t pvq_synth_state_active_voices(const pvq_synth_state* s) {
    return guarded(0, [&] {
        return s ? s->impl->active_voice_count() : 0;   // voice_collection.rs:11
    });
}
pvq_status pvq_synth_batch_create(int device_id, const pvq_synth_bank* bank, uint32_t n_streams, int32_t sample_rate, uint32_t maximum_polyphony,
                                  pvq_synth_batch** out) {
    return guarded([&] { return synth_batch_make(device_id, bank, n_streams, sample_rate, maximum_polyphony, 0, out); });
}
pvq_status pvq_synth_batch_create_ex(int device_id, const pvq_synth_bank* bank, uint32_t n_streams, int32_t sample_rate, uint32_t maximum_polyphony,
                                     uint32_t flags, pvq_synth_batch** out) {
    return guarded([&] { return synth_batch_make(device_id, bank, n_streams, sample_rate, maximum_polyphony, flags, out); });
}
void pvq_synth_batch_destroy(pvq_synth_batch* b) { destroy(b); }
pvq_status pvq_synth_batch_render_device(pvq_synth_batch* b, const uint64_t* event_ptr, const double* time_s, const int32_t* channel,
                                         const int32_t* command, const int32_t* data1, const int32_t* data2, const size_t* n_blocks, float* const* d_left,
                                         float* const* d_right, const uint32_t* snapshot_blocks, size_t n_snapshots, void* stream) {
    return guarded([&] {
        if (!b) return null_handle();
        if (!event_ptr) return invalid_arg("synth batch: event_ptr is needed");
        const uint32_t n = b->impl->n_streams();
        std::vector<pvq::SynthEvents> ev(n);
        for (uint32_t s = 0; s < n; ++s) {
            const uint64_t e0 = event_ptr[s], e1 = event_ptr[s + 1];
            if (e1 < e0 || (e1 > e0 && !(time_s && channel && command && data1 && data2)))
                return invalid_arg("synth batch: event_ptr must ascend, and the event arrays are needed where it names events");
            if (e1 > e0) ev[s] = pvq::SynthEvents{time_s + e0, channel + e0, command + e0, data1 + e0, data2 + e0, static_cast<size_t>(e1 - e0)};
        }
        return b->impl->render_device(ev.data(), n_blocks, d_left, d_right, snapshot_blocks, n_snapshots,
                                      static_cast<hipStream_t>(stream));   // midifile_sequencer.rs:52-104 for every stream
    });
}
pvq_status pvq_synth_batch_last_times(pvq_synth_batch* b, float* out_ms4, uint64_t* out_records) {
    return guarded([&] {
        if (!b) return null_handle();
        return b->impl->last_times(out_ms4, out_records);
    });
}
pvq_status pvq_synth_batch_get_snapshots(const pvq_synth_batch* b, uint32_t stream_index, uint32_t* out_counts, uint32_t* voice_ptr, size_t ptr_capacity,
                                         int32_t* key, float* gain_left, float* gain_right, size_t capacity) {
    return guarded([&] {
        if (!b) return null_handle();
        const pvq::SynthPlan* p = b->impl->plan_of(stream_index);
        if (!p) return invalid_arg("synth batch: stream_index is 0 .. n_streams - 1");
        return synth_snapshots_out(*p, out_counts, voice_ptr, ptr_capacity, key, gain_left, gain_right, capacity);   // synthesizer.rs:525
    });
}
pvq_status pvq_synth_effects_create(int32_t sample_rate, pvq_synth_effects** out) {
    return guarded([&] {
        return make_handle(out, [&](auto& impl) {
            std::string err;
            const pvq_status st = pvq::SynthEffects::create(sample_rate, impl, err);   // Reverb::new, Chorus::new (synthesizer.rs:102-126)
            if (st != PVQ_OK) pvq::set_last_error(err);
            return st;
        });
    });
}
void pvq_synth_effects_destroy(pvq_synth_effects* e) { destroy(e); }
pvq_status pvq_synth_effects_process(pvq_synth_effects* e, size_t n_blocks, const float* chorus_in_left, const float* chorus_in_right, const float* reverb_in,
                                     float* chorus_out_left, float* chorus_out_right, float* reverb_out_left, float* reverb_out_right) {
    return guarded([&] {
        if (!e) return null_handle();
        if (n_blocks > 0x7fffffffull / pvq::synth::BLOCK) return invalid_arg("synth effects: too many blocks in one call");
        if (n_blocks && !(chorus_in_left && chorus_in_right && reverb_in && chorus_out_left && chorus_out_right && reverb_out_left && reverb_out_right))
            return invalid_arg("synth effects: the three inputs and the four outputs are needed");
        e->impl->process(n_blocks, chorus_in_left, chorus_in_right, reverb_in, chorus_out_left, chorus_out_right, reverb_out_left,
                         reverb_out_right);   // Chorus::process, Reverb::process
        return PVQ_OK;
    });
}
uint32_t pvq_synth_chorus_table(int32_t sample_rate, float* out, size_t capacity) {
    return guarded(0u, [&]() -> uint32_t {
        if (sample_rate < 16000 || sample_rate > 192000) {
            pvq::set_last_error("The sample rate must be between 16000 and 192000, but was " + std::to_string(sample_rate) + ".");
            return 0;
        }
        const std::vector<float> table = pvq::synth_chorus_table(sample_rate);   // chorus.rs:24-29
        if (out && capacity >= table.size()) std::memcpy(out, table.data(), table.size() * sizeof(float));
        return static_cast<uint32_t>(table.size());
    });
}

}  // extern "C"
