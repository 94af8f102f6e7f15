// synth_host.hpp — the SoundFont synthesizer of pitchvis_train (rustysynth_fork; by default the dry path, enable_reverb_and_chorus =
// false; with `effects` the reverb and chorus of synthesizer.rs:393-475 too, which is what train.rs:264 renders) on the host: the sound bank at generator level, the control rate, and the planner that turns MIDI-style events into a PLAN the audio
// rate replays without further decisions — on the host (SynthState::render, the one-stream face) and on the device (synth_batch.hpp)
// with synth_math.hpp's arithmetic, so both consume the same plan by construction.
//
// Work splits at the 64-sample block.  Once per voice and block: both envelopes, both LFOs, the pitch and pitch_ratio_fp, the filter
// coefficients, the four mix gains, and every decision about which voices exist (note_on, exclusive class, stealing, swap-removal,
// release, hold pedal, kill).  None of it depends on sample VALUES, only on times and on the oscillator's integer position, which the
// planner tracks exactly in O(loop wraps) per block.  All libm calls (powf, exp, sinf, cosf, log10f) live here.
// With effects, the control rate also gives every record its chorus and reverb gains (synth::Sends), and the audio rate adds three
// more sums per block, the chorus, the reverb and the final sum with synth_fx_math.hpp's arithmetic (SynthEffects below).
// Left out: SF2 / MIDI file parsing, play_loop, polyphony above 64, other block sizes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pvq.h"
#include "synth_fx_math.hpp"
#include "synth_math.hpp"

namespace pvq {

constexpr uint32_t SYNTH_GEN_COUNT = 61;        // generator_type.rs:71
constexpr uint32_t SYNTH_MAX_POLYPHONY = 64;    // SynthesizerSettings::DEFAULT_MAXIMUM_POLYPHONY: one wavefront
constexpr uint32_t SYNTH_CHANNELS = 16;         // synthesizer.rs:55

// SoundFont after parsing (soundfont.rs, instrument_region.rs, preset_region.rs): arrays in, no file format here.
class SynthBank {
   public:
    struct Sample {   // sample_header.rs: start, end, start_loop, end_loop, sample_rate, original_pitch, pitch_correction
        int32_t start, end, start_loop, end_loop, sample_rate, original_pitch, pitch_correction;
    };
    struct InstrumentRegion {   // instrument_region.rs:21-30
        int16_t gs[SYNTH_GEN_COUNT];
        Sample sample;
    };
    struct PresetRegion {   // preset_region.rs:20-23
        int16_t gs[SYNTH_GEN_COUNT];
        uint32_t instrument;
    };
    struct Preset {
        int32_t bank_number, patch_number;
        uint32_t first, count;
    };
    // samples [n_samples][7]; instrument_gs [n_ir][61] (the generators after the defaults and the zones, instrument_region.rs:39-66)
    // with instrument_sample [n_ir]; instruments [n_instruments][2] = first region, regions; preset_gs [n_pr][61] with
    // preset_instrument [n_pr]; presets [n_presets][4] = bank, patch, first region, regions.  Every index is checked here
    // (PVQ_ERR_INVALID_ARG, the text names it): the reference's InvalidSampleId / InvalidInstrumentId, and sample points outside
    // wave_data, which the reference meets as a panic while rendering.
    static pvq_status create(const int16_t* wave, size_t n_wave, const int32_t* samples, uint32_t n_samples, const int16_t* instrument_gs,
                             const uint32_t* instrument_sample, uint32_t n_ir, const uint32_t* instruments, uint32_t n_instruments,
                             const int16_t* preset_gs, const uint32_t* preset_instrument, uint32_t n_pr, const int32_t* presets,
                             uint32_t n_presets, std::shared_ptr<const SynthBank>& out, std::string& err);
    std::vector<int16_t> wave;
    std::vector<InstrumentRegion> iregions;
    std::vector<uint32_t> instruments;   // [n][2]
    std::vector<PresetRegion> pregions;
    std::vector<Preset> presets;
    std::vector<synth::SampleDesc> descs;   // [n_ir]: what a voice started from instrument region i reads
    std::map<int32_t, size_t> preset_lookup;   // synthesizer.rs:64-84
    size_t default_preset = 0;
};

struct SynthEvents {   // midifile_sequencer.rs: times in seconds, ascending; the four bytes of a NORMAL message, each 0 .. 255
    const double* time = nullptr;
    const int32_t* channel = nullptr;
    const int32_t* command = nullptr;
    const int32_t* data1 = nullptr;
    const int32_t* data2 = nullptr;
    size_t n = 0;
};

struct SynthActiveVoice {   // synthesizer.rs:525, voice.rs:38-48: what the trainer reads of a voice
    int32_t key;
    float current_mix_gain_left, current_mix_gain_right;
};

struct SynthPlan {
    std::vector<uint32_t> block_ptr;         // [n_blocks + 1] into records
    std::vector<synth::Record> records;      // per block in the active list's order: the order of the sum
    std::vector<uint32_t> snapshot_ptr;      // [n_snapshots + 1] into snapshots
    std::vector<SynthActiveVoice> snapshots;
    std::vector<synth::Sends> sends;         // a plan made with effects: one per record; otherwise empty
    void clear() {
        block_ptr.assign(1, 0u);
        records.clear();
        sends.clear();
        snapshot_ptr.assign(1, 0u);
        snapshots.clear();
    }
};

// Chorus::new's delay table (chorus.rs:24-29, synthesizer.rs:124): round(sample_rate / 0.4) entries, each
// (sample_rate * (0.002 + 0.0019 * sin(phase))) as f32 from an f64 sin
std::vector<float> synth_chorus_table(int32_t sample_rate);

// Reverb + Chorus (reverb.rs, chorus.rs) for one stream on the host, fed with chosen inputs: the effect state and nothing else.
// SynthState's effect path is this object; the device keeps the same state in SynthBatch's buffers.
class SynthEffects {
   public:
    // sample_rate as SynthState::create's.  PVQ_ERR_INTERNAL if a table entry falls outside 1 <= delay < ring - 1: the bound that
    // lets the device index the ring without a test (it holds at every admitted rate; it is checked, not assumed).
    static pvq_status create(int32_t sample_rate, std::unique_ptr<SynthEffects>& out, std::string& err);
    // n_blocks * 64 values each; the state goes on from call to call.  One sample at a time, in the reference's order.
    void process(size_t n_blocks, const float* chorus_in_left, const float* chorus_in_right, const float* reverb_in, float* chorus_out_left,
                 float* chorus_out_right, float* reverb_out_left, float* reverb_out_right);
    const synth::FxLayout& layout() const { return layout_; }
    const std::vector<float>& table() const { return table_; }

   private:
    SynthEffects() = default;
    synth::FxLayout layout_{};
    synth::ReverbConstants k_{};
    std::vector<float> table_, reverb_, ring_;   // ring_: [2][layout_.ring]
    float store_[2 * synth::FX_COMBS] = {};      // CombFilter::filter_store
    uint32_t pos_[synth::FX_BUFFERS] = {};       // every buffer_index: the sample count modulo the buffer's length
    uint32_t ring_index_ = 0, table_index_[2] = {0, 0};
};

// Synthesizer + MidiFileSequencer (synthesizer.rs, midifile_sequencer.rs:52-104) for one stream, control rate only.
class SynthState {
   public:
    // PVQ_ERR_INVALID_ARG with the reference's texts: sample_rate outside 16 000 .. 192 000, maximum_polyphony outside 8 .. 256
    // (synthesizer_settings.rs:35-57); PVQ_ERR_UNSUPPORTED: a polyphony above 64
    // effects: enable_reverb_and_chorus (synthesizer_settings.rs): plans carry `sends`, render adds the effects.  plan_only: no
    // host effect state is made (SynthBatch: the device holds it); render is then not to be called.
    static pvq_status create(std::shared_ptr<const SynthBank> bank, int32_t sample_rate, uint32_t maximum_polyphony,
                             std::unique_ptr<SynthState>& out, std::string& err, bool effects = false, bool plan_only = false);
    ~SynthState();
    // Advances n_blocks blocks.  `events` is the stream's whole list; the state keeps how many it has consumed, so the next call goes
    // on where this one stopped.  Before each block every event with time <= current_time is applied, and current_time grows by the
    // repeated f64 addition of 64 / sample_rate (midifile_sequencer.rs:61-64, 87-103).  snapshot_blocks (ascending block numbers of
    // this call): the active voices after that block.  The plan is appended to (the caller clears it).  A read that would leave
    // wave_data — where the reference panics — ends the call with PVQ_ERR_INVALID_ARG naming stream, block and key; the state is
    // then no longer usable.
    pvq_status plan(const SynthEvents& events, size_t n_blocks, const uint32_t* snapshot_blocks, size_t n_snapshots, uint32_t stream_index,
                    SynthPlan& out, std::string& err);
    // plan, then the replay: left / right [n_blocks * 64].  The plan of the call stays readable in last_plan().
    pvq_status render(const SynthEvents& events, size_t n_blocks, const uint32_t* snapshot_blocks, size_t n_snapshots, float* left, float* right,
                      std::string& err);
    const SynthPlan& last_plan() const { return last_plan_; }
    uint32_t active_voice_count() const;
    uint32_t maximum_polyphony() const { return maximum_polyphony_; }
    int32_t sample_rate() const { return sample_rate_; }
    const SynthBank& bank() const { return *bank_; }
    void set_master_volume(float v) { master_volume_ = v; }   // synthesizer.rs:521
    float master_volume() const { return master_volume_; }
    bool effects() const { return effects_; }

   private:
    SynthState() = default;
    struct Impl;
    std::unique_ptr<Impl> impl_;
    std::shared_ptr<const SynthBank> bank_;
    int32_t sample_rate_ = 0;
    uint32_t maximum_polyphony_ = 0;
    float master_volume_ = 0.5f;   // synthesizer.rs:100
    bool effects_ = false;
    std::unique_ptr<SynthEffects> fx_;
    synth::Lane lanes_[SYNTH_MAX_POLYPHONY];
    uint32_t lane_desc_[SYNTH_MAX_POLYPHONY] = {};
    SynthPlan last_plan_;
};

// the replay of one stream's plan on the host: blocks [0, n_blocks) of `plan` into left / right [n_blocks * 64].  With `fx` (the
// plan then carries sends): the three effect sums, chorus, reverb and the final sum too (synthesizer.rs:393-475).
void synth_replay(const SynthBank& bank, const SynthPlan& plan, size_t n_blocks, synth::Lane* lanes, uint32_t* lane_desc, float* left, float* right,
                  SynthEffects* fx = nullptr, float master_volume = 0.5f);

// plan() of many states side by side, on at most 16 threads.  events / n_blocks / plans [n]; the first failing stream's status and text.
pvq_status synth_plan_streams(SynthState* const* states, const SynthEvents* events, const size_t* n_blocks, size_t n, const uint32_t* snapshot_blocks,
                              size_t n_snapshots, SynthPlan* plans, std::string& err);

}  // namespace pvq
