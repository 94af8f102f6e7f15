// synth_host.cpp — rustysynth_fork's control rate restated (synth_host.hpp): every f32 / f64 expression is the reference's, in its
// order, file:line cited; built with -ffp-contract=off.  The audio rate is synth_math.hpp's, the effects' synth_fx_math.hpp's.
#include "synth_host.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>
#include <utility>

namespace pvq {

namespace {
using synth::NON_AUDIBLE;

// generator_type.rs:9-69
enum Gen : uint32_t {
    START_ADDRESS_OFFSET = 0, END_ADDRESS_OFFSET = 1, START_LOOP_ADDRESS_OFFSET = 2, END_LOOP_ADDRESS_OFFSET = 3, START_ADDRESS_COARSE_OFFSET = 4,
    MODULATION_LFO_TO_PITCH = 5, VIBRATO_LFO_TO_PITCH = 6, MODULATION_ENVELOPE_TO_PITCH = 7, INITIAL_FILTER_CUTOFF_FREQUENCY = 8,
    INITIAL_FILTER_Q = 9, MODULATION_LFO_TO_FILTER_CUTOFF_FREQUENCY = 10, MODULATION_ENVELOPE_TO_FILTER_CUTOFF_FREQUENCY = 11,
    END_ADDRESS_COARSE_OFFSET = 12, MODULATION_LFO_TO_VOLUME = 13, CHORUS_EFFECTS_SEND = 15, REVERB_EFFECTS_SEND = 16, PAN = 17,
    DELAY_MODULATION_LFO = 21, FREQUENCY_MODULATION_LFO = 22, DELAY_VIBRATO_LFO = 23, FREQUENCY_VIBRATO_LFO = 24,
    DELAY_MODULATION_ENVELOPE = 25, ATTACK_MODULATION_ENVELOPE = 26, HOLD_MODULATION_ENVELOPE = 27, DECAY_MODULATION_ENVELOPE = 28,
    SUSTAIN_MODULATION_ENVELOPE = 29, RELEASE_MODULATION_ENVELOPE = 30, KEY_NUMBER_TO_MODULATION_ENVELOPE_HOLD = 31,
    KEY_NUMBER_TO_MODULATION_ENVELOPE_DECAY = 32, DELAY_VOLUME_ENVELOPE = 33, ATTACK_VOLUME_ENVELOPE = 34, HOLD_VOLUME_ENVELOPE = 35,
    DECAY_VOLUME_ENVELOPE = 36, SUSTAIN_VOLUME_ENVELOPE = 37, RELEASE_VOLUME_ENVELOPE = 38, KEY_NUMBER_TO_VOLUME_ENVELOPE_HOLD = 39,
    KEY_NUMBER_TO_VOLUME_ENVELOPE_DECAY = 40, INSTRUMENT = 41, KEY_RANGE = 43, VELOCITY_RANGE = 44, START_LOOP_ADDRESS_COARSE_OFFSET = 45,
    INITIAL_ATTENUATION = 48, END_LOOP_ADDRESS_COARSE_OFFSET = 50, COARSE_TUNE = 51, FINE_TUNE = 52, SAMPLE_ID = 53, SAMPLE_MODES = 54,
    SCALE_TUNING = 56, EXCLUSIVE_CLASS = 57, OVERRIDING_ROOT_KEY = 58,
};
constexpr int32_t NO_LOOP = 0, LOOP_UNTIL_NOTE_OFF = 3;   // loop_mode.rs
constexpr int32_t DELAY = 0, ATTACK = 1, HOLD = 2, DECAY = 3, RELEASE = 4;   // envelope_stage.rs
constexpr float PI_F = 3.14159265358979323846f;
constexpr float HALF_PI = PI_F / 2.0f;                 // soundfont_math.rs:10
constexpr float LOG_NON_AUDIBLE = -6.9077554f;         // soundfont_math.rs:12
constexpr int64_t MAX_RATIO_FP = int64_t{1} << 55;     // past this the position would leave i64 within a block

// soundfont_math.rs:14-62
inline float sf_max(float x, float y) { return x > y ? x : y; }
inline float sf_clamp(float value, float min, float max) { return value < min ? min : (value > max ? max : value); }
inline float timecents_to_seconds(float x) { return powf(2.0f, (1.0f / 1200.0f) * x); }
inline float cents_to_hertz(float x) { return 8.176f * powf(2.0f, (1.0f / 1200.0f) * x); }
inline float cents_to_multiplying_factor(float x) { return powf(2.0f, (1.0f / 1200.0f) * x); }
inline float decibels_to_linear(float x) { return powf(10.0f, 0.05f * x); }
inline float linear_to_decibels(float x) { return 20.0f * log10f(x); }
inline float key_number_to_multiplying_factor(int32_t cents, int32_t key) { return timecents_to_seconds(static_cast<float>(cents * (60 - key))); }
inline double exp_cutoff(double x) { return x < static_cast<double>(LOG_NON_AUDIBLE) ? 0.0 : exp(x); }

// Rust's `f64 as i64`: saturating, NaN -> 0
inline int64_t f64_as_i64(double v) {
    if (!(v == v)) return 0;
    if (v >= 9223372036854775807.0) return std::numeric_limits<int64_t>::max();
    if (v <= -9223372036854775808.0) return std::numeric_limits<int64_t>::min();
    return static_cast<int64_t>(v);
}

// instrument_region.rs:128-162
inline int32_t ir_offset(const int16_t* gs, Gen coarse, Gen fine) { return 32768 * static_cast<int32_t>(gs[coarse]) + static_cast<int32_t>(gs[fine]); }

// region_pair.rs: preset + instrument generators
struct RegionPair {
    const SynthBank::PresetRegion* preset;
    const SynthBank::InstrumentRegion* instrument;
    int32_t gs(uint32_t i) const { return static_cast<int32_t>(preset->gs[i]) + static_cast<int32_t>(instrument->gs[i]); }   // :19-21
    float gf(uint32_t i) const { return static_cast<float>(gs(i)); }
    float timecents(uint32_t i) const { return timecents_to_seconds(gf(i)); }
    int32_t sample_modes() const {   // instrument_region.rs:344-350
        return instrument->gs[SAMPLE_MODES] != 2 ? static_cast<int32_t>(instrument->gs[SAMPLE_MODES]) : NO_LOOP;
    }
    int32_t root_key() const {       // instrument_region.rs:360-366
        return instrument->gs[OVERRIDING_ROOT_KEY] != -1 ? static_cast<int32_t>(instrument->gs[OVERRIDING_ROOT_KEY]) : instrument->sample.original_pitch;
    }
    int32_t fine_tune() const { return gs(FINE_TUNE) + instrument->sample.pitch_correction; }   // region_pair.rs:215-217
};

bool region_contains(const int16_t* gs, int32_t key, int32_t velocity) {   // instrument_region.rs:121-126, 316-330; preset_region.rs:87-92
    const int32_t kr = gs[KEY_RANGE], vr = gs[VELOCITY_RANGE];
    return (kr & 0xFF) <= key && key <= ((kr >> 8) & 0xFF) && (vr & 0xFF) <= velocity && velocity <= ((vr >> 8) & 0xFF);
}

// channel.rs
struct Channel {
    bool is_percussion_channel = false;
    int32_t bank_number = 0, patch_number = 0;
    int16_t modulation = 0, volume = 0, pan = 0, expression = 0;
    bool hold_pedal = false;
    uint8_t reverb_send = 0, chorus_send = 0;
    int16_t rpn = 0, pitch_bend_range = 0, coarse_tune = 0, fine_tune = 0;
    float pitch_bend = 0.0f;
    static int16_t coarse(int16_t cur, int32_t value) {   // (cur & 0x7F) | (value << 7) as i16
        return static_cast<int16_t>((cur & 0x7F) | static_cast<int16_t>(static_cast<uint32_t>(value) << 7));
    }
    static int16_t fine(int16_t cur, int32_t value) {     // ((cur as i32 & 0xFF80) | value) as i16
        return static_cast<int16_t>(static_cast<uint32_t>((static_cast<int32_t>(cur) & 0xFF80) | value));
    }
    void reset() {   // :52-71
        bank_number = is_percussion_channel ? 128 : 0;
        patch_number = 0;
        modulation = 0;
        volume = 100 << 7;
        pan = 64 << 7;
        expression = 127 << 7;
        hold_pedal = false;
        reverb_send = 40;
        chorus_send = 0;
        rpn = -1;
        pitch_bend_range = 2 << 7;
        coarse_tune = 0;
        fine_tune = 8192;
        pitch_bend = 0.0f;
    }
    void reset_all_controllers() {   // :73-81
        modulation = 0;
        expression = 127 << 7;
        hold_pedal = false;
        rpn = -1;
        pitch_bend = 0.0f;
    }
    void set_bank(int32_t value) { bank_number = value + (is_percussion_channel ? 128 : 0); }   // :83-89
    void data_entry_coarse(int32_t value) {   // :147-155
        if (rpn == 0) pitch_bend_range = coarse(pitch_bend_range, value);
        else if (rpn == 1) fine_tune = coarse(fine_tune, value);
        else if (rpn == 2) coarse_tune = static_cast<int16_t>(value - 64);
    }
    void data_entry_fine(int32_t value) {     // :157-163
        if (rpn == 0) pitch_bend_range = fine(pitch_bend_range, value);
        else if (rpn == 1) fine_tune = fine(fine_tune, value);
    }
    void set_pitch_bend(int32_t value1, int32_t value2) { pitch_bend = (1.0f / 8192.0f) * static_cast<float>((value1 | (value2 << 7)) - 8192); }   // :165-167
    float get_modulation() const { return (50.0f / 16383.0f) * static_cast<float>(modulation); }   // :177-215
    float get_volume() const { return (1.0f / 16383.0f) * static_cast<float>(volume); }
    float get_pan() const { return (100.0f / 16383.0f) * static_cast<float>(pan) - 50.0f; }
    float get_expression() const { return (1.0f / 16383.0f) * static_cast<float>(expression); }
    float get_pitch_bend_range() const { return static_cast<float>(pitch_bend_range >> 7) + 0.01f * static_cast<float>(pitch_bend_range & 0x7F); }
    float get_tune() const { return static_cast<float>(coarse_tune) + (1.0f / 8192.0f) * static_cast<float>(fine_tune - 8192); }
    float get_pitch_bend() const { return get_pitch_bend_range() * pitch_bend; }
    float get_reverb_send() const { return (1.0f / 127.0f) * static_cast<float>(reverb_send); }
    float get_chorus_send() const { return (1.0f / 127.0f) * static_cast<float>(chorus_send); }
};

// volume_envelope.rs
struct VolumeEnvelope {
    int32_t sample_rate = 0;
    double attack_slope = 0, decay_slope = 0, release_slope = 0, attack_start_time = 0, hold_start_time = 0, decay_start_time = 0, release_start_time = 0;
    float sustain_level = 0, release_level = 0;
    size_t processed_sample_count = 0;
    int32_t stage = 0;
    float value = 0, priority = 0;
    void start(float delay, float attack, float hold, float decay, float sustain, float release) {   // :50-76
        attack_slope = 1.0 / static_cast<double>(attack);
        decay_slope = -9.226 / static_cast<double>(decay);
        release_slope = -9.226 / static_cast<double>(release);
        attack_start_time = static_cast<double>(delay);
        hold_start_time = attack_start_time + static_cast<double>(attack);
        decay_start_time = hold_start_time + static_cast<double>(hold);
        release_start_time = 0.0;
        sustain_level = sf_clamp(sustain, 0.0f, 1.0f);
        release_level = 0.0f;
        processed_sample_count = 0;
        stage = DELAY;
        value = 0.0f;
        process(0);
    }
    void release() {   // :78-82
        stage = RELEASE;
        release_start_time = static_cast<double>(processed_sample_count) / static_cast<double>(sample_rate);
        release_level = value;
    }
    bool process(size_t sample_count) {   // :84-134
        processed_sample_count += sample_count;
        const double current_time = static_cast<double>(processed_sample_count) / static_cast<double>(sample_rate);
        while (stage <= HOLD) {
            const double end_time = stage == DELAY ? attack_start_time : (stage == ATTACK ? hold_start_time : decay_start_time);
            if (current_time < end_time) break;
            stage += 1;
        }
        if (stage == DELAY) {
            value = 0.0f;
            priority = 4.0f + value;
            return true;
        } else if (stage == ATTACK) {
            value = static_cast<float>(attack_slope * (current_time - attack_start_time));
            priority = 3.0f + value;
            return true;
        } else if (stage == HOLD) {
            value = 1.0f;
            priority = 2.0f + value;
            return true;
        } else if (stage == DECAY) {
            value = sf_max(static_cast<float>(exp_cutoff(decay_slope * (current_time - decay_start_time))), sustain_level);
            priority = 1.0f + value;
            return value > NON_AUDIBLE;
        }
        value = static_cast<float>(static_cast<double>(release_level) * exp_cutoff(release_slope * (current_time - release_start_time)));
        priority = value;
        return value > NON_AUDIBLE;
    }
};

// modulation_envelope.rs
struct ModulationEnvelope {
    int32_t sample_rate = 0;
    double attack_slope = 0, decay_slope = 0, release_slope = 0, attack_start_time = 0, hold_start_time = 0, decay_start_time = 0, decay_end_time = 0,
           release_end_time = 0;
    float sustain_level = 0, release_level = 0;
    size_t processed_sample_count = 0;
    int32_t stage = 0;
    float value = 0;
    void start(float delay, float attack, float hold, float decay, float sustain, float release) {   // :50-78
        attack_slope = 1.0 / static_cast<double>(attack);
        decay_slope = 1.0 / static_cast<double>(decay);
        release_slope = 1.0 / static_cast<double>(release);
        attack_start_time = static_cast<double>(delay);
        hold_start_time = attack_start_time + static_cast<double>(attack);
        decay_start_time = hold_start_time + static_cast<double>(hold);
        decay_end_time = decay_start_time + static_cast<double>(decay);
        release_end_time = static_cast<double>(release);
        sustain_level = sf_clamp(sustain, 0.0f, 1.0f);
        release_level = 0.0f;
        processed_sample_count = 0;
        stage = DELAY;
        value = 0.0f;
        process(0);
    }
    void release() {   // :80-84
        stage = RELEASE;
        release_end_time += static_cast<double>(processed_sample_count) / static_cast<double>(sample_rate);
        release_level = value;
    }
    bool process(size_t sample_count) {   // :86-132
        processed_sample_count += sample_count;
        const double current_time = static_cast<double>(processed_sample_count) / static_cast<double>(sample_rate);
        while (stage <= HOLD) {
            const double end_time = stage == DELAY ? attack_start_time : (stage == ATTACK ? hold_start_time : decay_start_time);
            if (current_time < end_time) break;
            stage += 1;
        }
        if (stage == DELAY) {
            value = 0.0f;
            return true;
        } else if (stage == ATTACK) {
            value = static_cast<float>(attack_slope * (current_time - attack_start_time));
            return true;
        } else if (stage == HOLD) {
            value = 1.0f;
            return true;
        } else if (stage == DECAY) {
            value = sf_max(static_cast<float>(decay_slope * (decay_end_time - current_time)), sustain_level);
            return value > NON_AUDIBLE;
        }
        value = sf_max(static_cast<float>(static_cast<double>(release_level) * release_slope * (release_end_time - current_time)), 0.0f);
        return value > NON_AUDIBLE;
    }
};

// lfo.rs
struct Lfo {
    int32_t sample_rate = 0;
    bool active = false;
    double delay = 0, period = 0;
    size_t processed_sample_count = 0;
    float value = 0;
    void start(float delay_, float frequency) {   // :32-45
        if (frequency > 1.0e-3f) {
            active = true;
            delay = static_cast<double>(delay_);
            period = 1.0 / static_cast<double>(frequency);
            processed_sample_count = 0;
            value = 0.0f;
        } else {
            active = false;
            value = 0.0f;
        }
    }
    void process() {   // :47-68
        if (!active) return;
        processed_sample_count += synth::BLOCK;
        const double current_time = static_cast<double>(processed_sample_count) / static_cast<double>(sample_rate);
        if (current_time < delay) {
            value = 0.0f;
        } else {
            const double phase = fmod(current_time - delay, period) / period;
            if (phase < 0.25) value = static_cast<float>(4.0 * phase);
            else if (phase < 0.75) value = static_cast<float>(4.0 * (0.5 - phase));
            else value = static_cast<float>(4.0 * (phase - 1.0));
        }
    }
};

constexpr int32_t PLAYING = 0, RELEASE_REQUESTED = 1, RELEASED = 2;   // voice.rs:307-311

enum class OscStep { Sounds, Ended, BadRead };

// voice.rs with oscillator.rs's control part and bi_quad_filter.rs:51-75, 101-107
struct Voice {
    uint32_t id = 0;   // the voice object: VoiceCollection::process swaps objects, their position and filter memory go with them
    int32_t sample_rate = 0;
    VolumeEnvelope vol_env;
    ModulationEnvelope mod_env;
    Lfo vib_lfo, mod_lfo;
    // Oscillator
    int32_t loop_mode = 0, root_key = 0;
    synth::SampleDesc desc{0, 0, 0, 0};
    uint32_t desc_index = 0;
    float tune = 0, pitch_change_scale = 0, sample_rate_ratio = 0;
    bool looping = false;
    int64_t position_fp = 0;
    // BiQuadFilter
    bool filter_active = false;
    float a[5] = {0, 0, 0, 0, 0};
    float previous_mix_gain_left = 0, previous_mix_gain_right = 0, current_mix_gain_left = 0, current_mix_gain_right = 0;
    float previous_reverb_send = 0, previous_chorus_send = 0, current_reverb_send = 0, current_chorus_send = 0, instrument_reverb = 0, instrument_chorus = 0;
    int32_t exclusive_class = 0, channel = 0, key = 0, velocity = 0;
    float note_gain = 0, cutoff = 0, resonance = 0, vib_lfo_to_pitch = 0, mod_lfo_to_pitch = 0, mod_env_to_pitch = 0;
    int32_t mod_lfo_to_cutoff = 0, mod_env_to_cutoff = 0;
    bool dynamic_cutoff = false;
    float mod_lfo_to_volume = 0;
    bool dynamic_volume = false;
    float instrument_pan = 0, smoothed_cutoff = 0;
    int32_t voice_state = 0;
    size_t voice_length = 0, min_voice_length = 0;
    bool started = false;   // start() ran and no record has carried it yet

    void set_low_pass_filter(float cutoff_frequency, float resonance_) {   // bi_quad_filter.rs:51-75
        if (cutoff_frequency < 0.499f * static_cast<float>(sample_rate)) {
            filter_active = true;
            const float q = resonance_ - (1.0f - 1.0f / 1.41421356237309504880f) / (1.0f + 6.0f * (resonance_ - 1.0f));
            const float w = 2.0f * PI_F * cutoff_frequency / static_cast<float>(sample_rate);
            const float cosw = cosf(w);
            const float alpha = sinf(w) / (2.0f * q);
            const float b0 = (1.0f - cosw) / 2.0f, b1 = 1.0f - cosw, b2 = (1.0f - cosw) / 2.0f;
            const float a0 = 1.0f + alpha, a1 = -2.0f * cosw, a2 = 1.0f - alpha;
            a[0] = b0 / a0;   // :101-107
            a[1] = b1 / a0;
            a[2] = b2 / a0;
            a[3] = a1 / a0;
            a[4] = a2 / a0;
        } else {
            filter_active = false;
        }
    }

    void start(const RegionPair& region, uint32_t region_index, const synth::SampleDesc& d, int32_t channel_, int32_t key_, int32_t velocity_) {   // voice.rs:125-174
        exclusive_class = region.instrument->gs[EXCLUSIVE_CLASS];
        channel = channel_;
        key = key_;
        velocity = velocity_;
        if (velocity > 0) {
            const float sample_attenuation = 0.4f * (0.1f * region.gf(INITIAL_ATTENUATION));
            const float filter_attenuation = 0.5f * (0.1f * region.gf(INITIAL_FILTER_Q));
            const float decibels = 2.0f * linear_to_decibels(static_cast<float>(velocity) / 127.0f) - sample_attenuation - filter_attenuation;
            note_gain = decibels_to_linear(decibels);
        } else {
            note_gain = 0.0f;
        }
        cutoff = cents_to_hertz(region.gf(INITIAL_FILTER_CUTOFF_FREQUENCY));
        resonance = decibels_to_linear(0.1f * region.gf(INITIAL_FILTER_Q));
        vib_lfo_to_pitch = 0.01f * region.gf(VIBRATO_LFO_TO_PITCH);
        mod_lfo_to_pitch = 0.01f * region.gf(MODULATION_LFO_TO_PITCH);
        mod_env_to_pitch = 0.01f * region.gf(MODULATION_ENVELOPE_TO_PITCH);
        mod_lfo_to_cutoff = region.gs(MODULATION_LFO_TO_FILTER_CUTOFF_FREQUENCY);
        mod_env_to_cutoff = region.gs(MODULATION_ENVELOPE_TO_FILTER_CUTOFF_FREQUENCY);
        dynamic_cutoff = mod_lfo_to_cutoff != 0 || mod_env_to_cutoff != 0;
        mod_lfo_to_volume = 0.1f * region.gf(MODULATION_LFO_TO_VOLUME);
        dynamic_volume = mod_lfo_to_volume > 0.05f;
        instrument_pan = sf_clamp(0.1f * region.gf(PAN), -50.0f, 50.0f);
        instrument_reverb = 0.01f * (0.1f * region.gf(REVERB_EFFECTS_SEND));   // voice.rs:159-160, region_pair.rs:89-95
        instrument_chorus = 0.01f * (0.1f * region.gf(CHORUS_EFFECTS_SEND));
        {   // region_ex.rs:41-65
            const float delay = region.timecents(DELAY_VOLUME_ENVELOPE), attack = region.timecents(ATTACK_VOLUME_ENVELOPE);
            const float hold = region.timecents(HOLD_VOLUME_ENVELOPE) * key_number_to_multiplying_factor(region.gs(KEY_NUMBER_TO_VOLUME_ENVELOPE_HOLD), key);
            const float decay = region.timecents(DECAY_VOLUME_ENVELOPE) * key_number_to_multiplying_factor(region.gs(KEY_NUMBER_TO_VOLUME_ENVELOPE_DECAY), key);
            const float sustain = decibels_to_linear(-(0.1f * region.gf(SUSTAIN_VOLUME_ENVELOPE)));
            const float release = sf_max(region.timecents(RELEASE_VOLUME_ENVELOPE), 0.01f);
            vol_env.start(delay, attack, hold, decay, sustain, release);
        }
        {   // region_ex.rs:67-91
            const float delay = region.timecents(DELAY_MODULATION_ENVELOPE);
            const float attack = region.timecents(ATTACK_MODULATION_ENVELOPE) * (static_cast<float>(145 - velocity) / 144.0f);
            const float hold = region.timecents(HOLD_MODULATION_ENVELOPE) * key_number_to_multiplying_factor(region.gs(KEY_NUMBER_TO_MODULATION_ENVELOPE_HOLD), key);
            const float decay = region.timecents(DECAY_MODULATION_ENVELOPE) * key_number_to_multiplying_factor(region.gs(KEY_NUMBER_TO_MODULATION_ENVELOPE_DECAY), key);
            const float sustain = 1.0f - (0.1f * region.gf(SUSTAIN_MODULATION_ENVELOPE)) / 100.0f;
            const float release = region.timecents(RELEASE_MODULATION_ENVELOPE);
            mod_env.start(delay, attack, hold, decay, sustain, release);
        }
        vib_lfo.start(region.timecents(DELAY_VIBRATO_LFO), cents_to_hertz(region.gf(FREQUENCY_VIBRATO_LFO)));       // region_ex.rs:93-98
        mod_lfo.start(region.timecents(DELAY_MODULATION_LFO), cents_to_hertz(region.gf(FREQUENCY_MODULATION_LFO)));   // region_ex.rs:100-105
        {   // region_ex.rs:15-39, oscillator.rs:56-88
            loop_mode = region.sample_modes();
            desc = d;
            desc_index = region_index;
            root_key = region.root_key();
            tune = static_cast<float>(region.gs(COARSE_TUNE)) + 0.01f * static_cast<float>(region.fine_tune());
            pitch_change_scale = 0.01f * static_cast<float>(region.gs(SCALE_TUNING));
            sample_rate_ratio = static_cast<float>(region.instrument->sample.sample_rate) / static_cast<float>(sample_rate);
            looping = loop_mode != NO_LOOP;
            position_fp = static_cast<int64_t>(desc.start) << synth::FRAC_BITS;
        }
        set_low_pass_filter(cutoff, resonance);   // (clear_buffer: F_START)
        smoothed_cutoff = cutoff;
        voice_state = PLAYING;
        voice_length = 0;
        started = true;
    }

    void end() {   // voice.rs:176-180
        if (voice_state == PLAYING) voice_state = RELEASE_REQUESTED;
    }
    void kill() { note_gain = 0.0f; }   // voice.rs:182-184

    float get_priority() const { return note_gain < NON_AUDIBLE ? 0.0f : vol_env.priority; }   // voice.rs:294-300

    // The oscillator's 64 steps on the integer position alone (oscillator.rs:112-176), in O(loop wraps): where the reads lie, whether
    // the sample ends, where the position stands afterwards.  `ends` is set when a sample without a loop stops inside the block.
    OscStep advance(int64_t ratio_fp, int64_t n_wave, bool& ends) {
        ends = false;
        int64_t pos = position_fp;
        int remaining = synth::BLOCK;
        if (!looping) {   // :112-139
            const int64_t end_fp = static_cast<int64_t>(desc.end) << synth::FRAC_BITS;
            if (pos < 0) return OscStep::BadRead;
            if (pos >= end_fp) return OscStep::Ended;   // t == 0: false
            int64_t j = remaining;
            if (ratio_fp > 0) j = std::min<int64_t>(remaining, (end_fp - pos + ratio_fp - 1) / ratio_fp);
            const int64_t last = (pos + (j - 1) * ratio_fp) >> synth::FRAC_BITS;
            if (last + 1 >= n_wave) return OscStep::BadRead;
            pos += j * ratio_fp;
            ends = j < remaining;
            position_fp = pos;
            return OscStep::Sounds;
        }
        const int64_t end_loop = desc.end_loop, loop_length = static_cast<int64_t>(desc.end_loop) - desc.start_loop;   // :141-176
        const int64_t end_loop_fp = end_loop << synth::FRAC_BITS, loop_length_fp = loop_length * synth::FRAC_UNIT;
        auto index2_of = [&](int64_t index1) { return index1 + 1 >= end_loop ? index1 + 1 - loop_length : index1 + 1; };
        auto inside = [&](int64_t i) { return i >= 0 && i < n_wave; };
        while (remaining > 0) {
            if (pos >= end_loop_fp) pos -= loop_length_fp;
            if (pos >= end_loop_fp || pos < 0) {   // the subtraction did not bring it back: one sample at a time until the read leaves wave_data
                const int64_t index1 = pos >> synth::FRAC_BITS;
                if (!inside(index1) || !inside(index2_of(index1))) return OscStep::BadRead;
                pos += ratio_fp;
                remaining -= 1;
                continue;
            }
            int64_t j = remaining;
            if (ratio_fp > 0) j = std::min<int64_t>(remaining, (end_loop_fp - pos + ratio_fp - 1) / ratio_fp);
            const int64_t last = (pos + (j - 1) * ratio_fp) >> synth::FRAC_BITS;   // < end_loop
            if (!inside(last) || !inside(index2_of(last))) return OscStep::BadRead;
            pos += j * ratio_fp;
            remaining -= static_cast<int>(j);
        }
        position_fp = pos;
        return OscStep::Sounds;
    }

    // voice.rs:186-278; fills `rec` and `snd` when the voice sounds
    OscStep process(const Channel* channels, int64_t n_wave, float master_volume, synth::Record& rec, synth::Sends& snd) {
        if (note_gain < NON_AUDIBLE) return OscStep::Ended;
        const Channel& channel_info = channels[channel];
        if (voice_length >= min_voice_length) {   // release_if_necessary, voice.rs:280-292
            if (voice_state == RELEASE_REQUESTED && !channel_info.hold_pedal) {
                vol_env.release();
                mod_env.release();
                if (loop_mode == LOOP_UNTIL_NOTE_OFF) looping = false;   // oscillator.rs:90-94
                voice_state = RELEASED;
            }
        }
        if (!vol_env.process(synth::BLOCK)) return OscStep::Ended;
        mod_env.process(synth::BLOCK);
        vib_lfo.process();
        mod_lfo.process();
        const float vib_pitch_change = (0.01f * channel_info.get_modulation() + vib_lfo_to_pitch) * vib_lfo.value;
        const float mod_pitch_change = mod_lfo_to_pitch * mod_lfo.value + mod_env_to_pitch * mod_env.value;
        const float channel_pitch_change = channel_info.get_tune() + channel_info.get_pitch_bend();
        const float pitch = static_cast<float>(key) + vib_pitch_change + mod_pitch_change + channel_pitch_change;
        const float pitch_change = pitch_change_scale * (pitch - static_cast<float>(root_key)) + tune;   // oscillator.rs:96-103
        const float pitch_ratio = sample_rate_ratio * powf(2.0f, pitch_change / 12.0f);
        const int64_t pitch_ratio_fp = f64_as_i64(static_cast<double>(synth::FRAC_UNIT) * static_cast<double>(pitch_ratio));
        if (pitch_ratio_fp < 0 || pitch_ratio_fp > MAX_RATIO_FP) return OscStep::BadRead;
        const bool looping_now = looping;
        bool ends = false;
        const OscStep st = advance(pitch_ratio_fp, n_wave, ends);
        if (st != OscStep::Sounds) return st;
        if (dynamic_cutoff) {
            const float cents = static_cast<float>(mod_lfo_to_cutoff) * mod_lfo.value + static_cast<float>(mod_env_to_cutoff) * mod_env.value;
            const float factor = cents_to_multiplying_factor(cents);
            const float new_cutoff = factor * cutoff;
            const float lower_limit = 0.5f * smoothed_cutoff, upper_limit = 2.0f * smoothed_cutoff;
            smoothed_cutoff = sf_clamp(new_cutoff, lower_limit, upper_limit);
            set_low_pass_filter(smoothed_cutoff, resonance);
        }
        previous_mix_gain_left = current_mix_gain_left;
        previous_mix_gain_right = current_mix_gain_right;
        previous_reverb_send = current_reverb_send;
        previous_chorus_send = current_chorus_send;
        const float ve = channel_info.get_volume() * channel_info.get_expression();
        const float channel_gain = ve * ve;
        float mix_gain = note_gain * channel_gain * vol_env.value;
        if (dynamic_volume) {
            const float decibels = mod_lfo_to_volume * mod_lfo.value;
            mix_gain *= decibels_to_linear(decibels);
        }
        const float angle = (PI_F / 200.0f) * (channel_info.get_pan() + instrument_pan + 50.0f);
        if (angle <= 0.0f) {
            current_mix_gain_left = mix_gain;
            current_mix_gain_right = 0.0f;
        } else if (angle >= HALF_PI) {
            current_mix_gain_left = 0.0f;
            current_mix_gain_right = mix_gain;
        } else {
            current_mix_gain_left = mix_gain * cosf(angle);
            current_mix_gain_right = mix_gain * sinf(angle);
        }
        current_reverb_send = sf_clamp(channel_info.get_reverb_send() + instrument_reverb, 0.0f, 1.0f);   // voice.rs:257-266
        current_chorus_send = sf_clamp(channel_info.get_chorus_send() + instrument_chorus, 0.0f, 1.0f);
        if (voice_length == 0) {
            previous_mix_gain_left = current_mix_gain_left;
            previous_mix_gain_right = current_mix_gain_right;
            previous_reverb_send = current_reverb_send;
            previous_chorus_send = current_chorus_send;
        }
        voice_length += synth::BLOCK;
        rec.voice = id;
        rec.flags = (started ? synth::F_START : 0u) | (looping_now ? synth::F_LOOP : 0u) | (filter_active ? synth::F_FILTER : 0u) | (ends ? synth::F_ENDS : 0u);
        rec.ratio_lo = static_cast<uint32_t>(static_cast<uint64_t>(pitch_ratio_fp));
        rec.ratio_hi = static_cast<uint32_t>(static_cast<uint64_t>(pitch_ratio_fp) >> 32);
        std::copy(a, a + 5, rec.a);
        rec.gain[0] = master_volume * previous_mix_gain_left;   // synthesizer.rs:373-383
        rec.gain[1] = master_volume * current_mix_gain_left;
        rec.gain[2] = master_volume * previous_mix_gain_right;
        rec.gain[3] = master_volume * current_mix_gain_right;
        rec.desc = desc_index;
        rec.key = key;
        rec.stage = static_cast<uint32_t>(vol_env.stage);
        snd.chorus[0] = previous_chorus_send * previous_mix_gain_left;   // synthesizer.rs:404-415: not times master_volume
        snd.chorus[1] = current_chorus_send * current_mix_gain_left;
        snd.chorus[2] = previous_chorus_send * previous_mix_gain_right;
        snd.chorus[3] = current_chorus_send * current_mix_gain_right;
        snd.reverb[0] = synth::FX_REVERB_GAIN * previous_reverb_send * (previous_mix_gain_left + previous_mix_gain_right);   // synthesizer.rs:449-454
        snd.reverb[1] = synth::FX_REVERB_GAIN * current_reverb_send * (current_mix_gain_left + current_mix_gain_right);
        started = false;
        return OscStep::Sounds;
    }
};
}  // namespace

struct SynthState::Impl {
    Channel channels[SYNTH_CHANNELS];
    std::vector<Voice> voices;
    size_t active_voice_count = 0;
    double current_time = 0.0;   // midifile_sequencer.rs:41
    size_t msg_index = 0;
    bool broken = false;

    // voice_collection.rs:27-70
    Voice& request_new(const SynthBank::InstrumentRegion& region, int32_t channel) {
        const int32_t exclusive_class = region.gs[EXCLUSIVE_CLASS];
        if (exclusive_class != 0)
            for (size_t i = 0; i < active_voice_count; ++i)
                if (voices[i].exclusive_class == exclusive_class && voices[i].channel == channel) return voices[i];
        if (active_voice_count < voices.size()) return voices[active_voice_count++];
        size_t candidate = 0;
        float lowest_priority = std::numeric_limits<float>::max();
        for (size_t i = 0; i < active_voice_count; ++i) {
            const float priority = voices[i].get_priority();
            if (priority < lowest_priority) {
                lowest_priority = priority;
                candidate = i;
            } else if (priority == lowest_priority) {
                if (voices[i].voice_length > voices[candidate].voice_length) candidate = i;   // the older one
            }
        }
        return voices[candidate];
    }
    void note_off(int32_t channel, int32_t key) {   // synthesizer.rs:215-225
        for (size_t i = 0; i < active_voice_count; ++i)
            if (voices[i].channel == channel && voices[i].key == key) voices[i].end();
    }
    void note_on(const SynthBank& bank, int32_t channel, int32_t key, int32_t velocity) {   // synthesizer.rs:227-278
        if (velocity == 0) {
            note_off(channel, key);
            return;
        }
        const Channel& channel_info = channels[channel];
        const int32_t preset_id = static_cast<int32_t>(static_cast<uint32_t>(channel_info.bank_number) << 16) | channel_info.patch_number;
        size_t preset = bank.default_preset;
        auto it = bank.preset_lookup.find(preset_id);
        if (it != bank.preset_lookup.end()) {
            preset = it->second;
        } else {
            const int32_t gm_preset_id = channel_info.bank_number < 128 ? channel_info.patch_number : (128 << 16);
            it = bank.preset_lookup.find(gm_preset_id);
            if (it != bank.preset_lookup.end()) preset = it->second;
        }
        const SynthBank::Preset& p = bank.presets[preset];
        for (uint32_t pr = p.first; pr < p.first + p.count; ++pr) {
            const SynthBank::PresetRegion& preset_region = bank.pregions[pr];
            if (!region_contains(preset_region.gs, key, velocity)) continue;
            const uint32_t first = bank.instruments[2 * preset_region.instrument], count = bank.instruments[2 * preset_region.instrument + 1];
            for (uint32_t ir = first; ir < first + count; ++ir) {
                const SynthBank::InstrumentRegion& instrument_region = bank.iregions[ir];
                if (!region_contains(instrument_region.gs, key, velocity)) continue;
                const RegionPair pair{&preset_region, &instrument_region};
                request_new(instrument_region, channel).start(pair, ir, bank.descs[ir], channel, key, velocity);
            }
        }
    }
    // synthesizer.rs:176-213
    void process_midi_message(const SynthBank& bank, int32_t channel, int32_t command, int32_t data1, int32_t data2) {
        if (!(0 <= channel && channel < static_cast<int32_t>(SYNTH_CHANNELS))) return;
        Channel& c = channels[channel];
        switch (command) {
            case 0x80: note_off(channel, data1); break;
            case 0x90: note_on(bank, channel, data1, data2); break;
            case 0xB0:
                switch (data1) {
                    case 0x00: c.set_bank(data2); break;
                    case 0x01: c.modulation = Channel::coarse(c.modulation, data2); break;
                    case 0x21: c.modulation = Channel::fine(c.modulation, data2); break;
                    case 0x06: c.data_entry_coarse(data2); break;
                    case 0x26: c.data_entry_fine(data2); break;
                    case 0x07: c.volume = Channel::coarse(c.volume, data2); break;
                    case 0x27: c.volume = Channel::fine(c.volume, data2); break;
                    case 0x0A: c.pan = Channel::coarse(c.pan, data2); break;
                    case 0x2A: c.pan = Channel::fine(c.pan, data2); break;
                    case 0x0B: c.expression = Channel::coarse(c.expression, data2); break;
                    case 0x2B: c.expression = Channel::fine(c.expression, data2); break;
                    case 0x40: c.hold_pedal = data2 >= 64; break;
                    case 0x5B: c.reverb_send = static_cast<uint8_t>(data2); break;
                    case 0x5D: c.chorus_send = static_cast<uint8_t>(data2); break;
                    case 0x65: c.rpn = Channel::coarse(c.rpn, data2); break;
                    case 0x64: c.rpn = Channel::fine(c.rpn, data2); break;
                    case 0x78:   // All Sound Off (synthesizer.rs:290-296)
                        for (size_t i = 0; i < active_voice_count; ++i)
                            if (voices[i].channel == channel) voices[i].kill();
                        break;
                    case 0x79: c.reset_all_controllers(); break;
                    case 0x7B:   // All Note Off (synthesizer.rs:297-303)
                        for (size_t i = 0; i < active_voice_count; ++i)
                            if (voices[i].channel == channel) voices[i].end();
                        break;
                    default: break;
                }
                break;
            case 0xC0: c.patch_number = data1; break;
            case 0xE0: c.set_pitch_bend(data1, data2); break;
            default: break;
        }
    }
};

pvq_status SynthBank::create(const int16_t* wave, size_t n_wave, const int32_t* samples, uint32_t n_samples, const int16_t* instrument_gs,
                             const uint32_t* instrument_sample, uint32_t n_ir, const uint32_t* instruments, uint32_t n_instruments,
                             const int16_t* preset_gs, const uint32_t* preset_instrument, uint32_t n_pr, const int32_t* presets, uint32_t n_presets,
                             std::shared_ptr<const SynthBank>& out, std::string& err) {
    out.reset();
    if (!wave || !samples || !instrument_gs || !instrument_sample || !instruments || !preset_gs || !preset_instrument || !presets) {
        err = "synth bank: a null array";
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_wave == 0 || n_wave > 0x7fffffffull || n_samples == 0 || n_ir == 0 || n_instruments == 0 || n_pr == 0 || n_presets == 0) {
        err = "synth bank: wave_data (1 .. 2^31 - 1 values), samples, regions, instruments and presets must not be empty";
        return PVQ_ERR_INVALID_ARG;
    }
    auto b = std::make_shared<SynthBank>();
    b->wave.assign(wave, wave + n_wave);
    const int64_t nw = static_cast<int64_t>(n_wave);
    for (uint32_t i = 0; i < n_samples; ++i) {
        if (samples[7 * i + 4] <= 0) {
            err = "synth bank: sample " + std::to_string(i) + " has a sample rate that is not positive";
            return PVQ_ERR_INVALID_ARG;
        }
        if (samples[7 * i + 5] < 0 || samples[7 * i + 5] > 255 || samples[7 * i + 6] < -128 || samples[7 * i + 6] > 127) {   // sample_header.rs: u8, i8
            err = "synth bank: sample " + std::to_string(i) + " has an original pitch outside 0 .. 255 or a pitch correction outside -128 .. 127";
            return PVQ_ERR_INVALID_ARG;
        }
    }
    b->iregions.resize(n_ir);
    b->descs.resize(n_ir);
    for (uint32_t i = 0; i < n_ir; ++i) {
        if (instrument_sample[i] >= n_samples) {   // InvalidSampleId, instrument_region.rs:68-74
            err = "synth bank: instrument region " + std::to_string(i) + " names sample " + std::to_string(instrument_sample[i]) + " of " + std::to_string(n_samples);
            return PVQ_ERR_INVALID_ARG;
        }
        InstrumentRegion& r = b->iregions[i];
        std::memcpy(r.gs, instrument_gs + static_cast<size_t>(i) * SYNTH_GEN_COUNT, sizeof r.gs);
        std::memcpy(&r.sample, samples + 7 * static_cast<size_t>(instrument_sample[i]), sizeof r.sample);
        const int64_t pts[4] = {static_cast<int64_t>(r.sample.start) + ir_offset(r.gs, START_ADDRESS_COARSE_OFFSET, START_ADDRESS_OFFSET),
                                static_cast<int64_t>(r.sample.end) + ir_offset(r.gs, END_ADDRESS_COARSE_OFFSET, END_ADDRESS_OFFSET),
                                static_cast<int64_t>(r.sample.start_loop) + ir_offset(r.gs, START_LOOP_ADDRESS_COARSE_OFFSET, START_LOOP_ADDRESS_OFFSET),
                                static_cast<int64_t>(r.sample.end_loop) + ir_offset(r.gs, END_LOOP_ADDRESS_COARSE_OFFSET, END_LOOP_ADDRESS_OFFSET)};
        for (int k = 0; k < 4; ++k)
            if (pts[k] < 0 || pts[k] > nw) {
                static const char* const names[4] = {"start", "end", "start_loop", "end_loop"};
                err = "synth bank: instrument region " + std::to_string(i) + " has its sample's " + names[k] + " at " + std::to_string(pts[k]) +
                      ", outside wave_data (" + std::to_string(n_wave) + " values)";
                return PVQ_ERR_INVALID_ARG;
            }
        b->descs[i] = synth::SampleDesc{static_cast<int32_t>(pts[0]), static_cast<int32_t>(pts[1]), static_cast<int32_t>(pts[2]), static_cast<int32_t>(pts[3])};
    }
    b->instruments.assign(instruments, instruments + 2 * static_cast<size_t>(n_instruments));
    for (uint32_t i = 0; i < n_instruments; ++i)
        if (static_cast<uint64_t>(instruments[2 * i]) + instruments[2 * i + 1] > n_ir) {
            err = "synth bank: instrument " + std::to_string(i) + " names regions past the " + std::to_string(n_ir) + " given";
            return PVQ_ERR_INVALID_ARG;
        }
    b->pregions.resize(n_pr);
    for (uint32_t i = 0; i < n_pr; ++i) {
        if (preset_instrument[i] >= n_instruments) {   // InvalidInstrumentId, preset_region.rs:44-50
            err = "synth bank: preset region " + std::to_string(i) + " names instrument " + std::to_string(preset_instrument[i]) + " of " + std::to_string(n_instruments);
            return PVQ_ERR_INVALID_ARG;
        }
        std::memcpy(b->pregions[i].gs, preset_gs + static_cast<size_t>(i) * SYNTH_GEN_COUNT, sizeof b->pregions[i].gs);
        b->pregions[i].instrument = preset_instrument[i];
    }
    b->presets.resize(n_presets);
    int32_t min_preset_id = std::numeric_limits<int32_t>::max();
    for (uint32_t i = 0; i < n_presets; ++i) {   // synthesizer.rs:64-84
        const int32_t* p = presets + 4 * static_cast<size_t>(i);
        if (p[0] < 0 || p[0] > 0x7fff || p[1] < 0 || p[1] > 0xffff || p[2] < 0 || p[3] < 0 || static_cast<uint64_t>(p[2]) + static_cast<uint64_t>(p[3]) > n_pr) {
            err = "synth bank: preset " + std::to_string(i) + " has a bank or patch number out of range, or names regions past the " + std::to_string(n_pr) + " given";
            return PVQ_ERR_INVALID_ARG;
        }
        b->presets[i] = Preset{p[0], p[1], static_cast<uint32_t>(p[2]), static_cast<uint32_t>(p[3])};
        const int32_t preset_id = (p[0] << 16) | p[1];
        b->preset_lookup[preset_id] = i;
        if (preset_id < min_preset_id) {
            b->default_preset = i;
            min_preset_id = preset_id;
        }
    }
    out = std::move(b);
    return PVQ_OK;
}

SynthState::~SynthState() = default;

std::vector<float> synth_chorus_table(int32_t sample_rate) {   // chorus.rs:24-29
    const synth::FxLayout l = synth::fx_layout(sample_rate);
    std::vector<float> table(l.table);
    for (size_t t = 0; t < table.size(); ++t) {
        const double phase = 2.0 * 3.14159265358979323846 * static_cast<double>(t) / static_cast<double>(table.size());
        table[t] = static_cast<float>(static_cast<double>(sample_rate) * (synth::FX_CHORUS_DELAY + synth::FX_CHORUS_DEPTH * sin(phase)));
    }
    return table;
}

pvq_status SynthEffects::create(int32_t sample_rate, std::unique_ptr<SynthEffects>& out, std::string& err) {
    out.reset();
    if (sample_rate < 16000 || sample_rate > 192000) {   // synthesizer_settings.rs:35-41
        err = "The sample rate must be between 16000 and 192000, but was " + std::to_string(sample_rate) + ".";
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<SynthEffects> e(new SynthEffects());
    e->layout_ = synth::fx_layout(sample_rate);
    e->k_ = synth::reverb_constants();
    e->table_ = synth_chorus_table(sample_rate);
    const synth::FxLayout& l = e->layout_;
    for (uint32_t i = 0; i < synth::FX_BUFFERS; ++i)
        if (l.len[i] <= static_cast<uint32_t>(synth::BLOCK)) {
            err = "synth effects: a reverb buffer no longer than a block";
            return PVQ_ERR_INTERNAL;
        }
    if (l.ring < static_cast<uint32_t>(synth::BLOCK) || l.table < 4 * static_cast<uint32_t>(synth::BLOCK)) {
        err = "synth effects: a chorus ring shorter than a block, or a delay table shorter than four";
        return PVQ_ERR_INTERNAL;
    }
    for (size_t t = 0; t < e->table_.size(); ++t)
        if (!(e->table_[t] >= 1.0f && e->table_[t] < static_cast<float>(l.ring - 1))) {
            err = "synth effects: delay table entry " + std::to_string(t) + " lies outside 1 <= delay < ring - 1";
            return PVQ_ERR_INTERNAL;
        }
    e->reverb_.assign(l.total, 0.0f);
    e->ring_.assign(2 * static_cast<size_t>(l.ring), 0.0f);
    e->table_index_[1] = l.table / 4;   // chorus.rs:35
    out = std::move(e);
    return PVQ_OK;
}

void SynthEffects::process(size_t n_blocks, const float* chorus_in_left, const float* chorus_in_right, const float* reverb_in, float* chorus_out_left,
                           float* chorus_out_right, float* reverb_out_left, float* reverb_out_right) {
    const synth::FxLayout& l = layout_;
    const float* chorus_in[2] = {chorus_in_left, chorus_in_right};
    float* chorus_out[2] = {chorus_out_left, chorus_out_right};
    for (size_t t = 0; t < n_blocks * synth::BLOCK; ++t) {
        for (int c = 0; c < 2; ++c) {   // chorus.rs:59-117
            float* ring = ring_.data() + static_cast<size_t>(c) * l.ring;
            const synth::ChorusTap tap = synth::chorus_tap(ring_index_, table_[table_index_[c]], l.ring);
            chorus_out[c][t] = synth::chorus_mix(tap, ring[tap.index1], ring[tap.index2]);
            ring[ring_index_] = chorus_in[c][t];
            if (++table_index_[c] == l.table) table_index_[c] = 0;
        }
        if (++ring_index_ == l.ring) ring_index_ = 0;
        float out[2];
        for (int c = 0; c < 2; ++c) {   // reverb.rs:161-182
            float* const buf = reverb_.data();
            const uint32_t first = c * synth::FX_COMBS;
            float x = synth::comb_output_sum([&](int i) { return buf[l.off[first + i] + pos_[first + i]]; });
            for (int i = 0; i < synth::FX_COMBS; ++i) {
                float& slot = buf[l.off[first + i] + pos_[first + i]];
                slot = synth::comb_step(slot, reverb_in[t], store_[first + i], k_);
            }
            for (int k = 0; k < synth::FX_ALLPASSES; ++k) {
                const uint32_t b = synth::FX_FIRST_ALLPASS + c * synth::FX_ALLPASSES + k;
                x = synth::allpass_step(buf[l.off[b] + pos_[b]], x);
            }
            out[c] = x;
        }
        synth::reverb_wet_mix(out[0], out[1], k_);
        reverb_out_left[t] = out[0];
        reverb_out_right[t] = out[1];
        for (uint32_t i = 0; i < synth::FX_BUFFERS; ++i)
            if (++pos_[i] == l.len[i]) pos_[i] = 0;
    }
}

pvq_status SynthState::create(std::shared_ptr<const SynthBank> bank, int32_t sample_rate, uint32_t maximum_polyphony, std::unique_ptr<SynthState>& out,
                              std::string& err, bool effects, bool plan_only) {
    out.reset();
    if (!bank) {
        err = "synth state: a bank is needed";
        return PVQ_ERR_INVALID_ARG;
    }
    if (sample_rate < 16000 || sample_rate > 192000) {   // synthesizer_settings.rs:35-41
        err = "The sample rate must be between 16000 and 192000, but was " + std::to_string(sample_rate) + ".";
        return PVQ_ERR_INVALID_ARG;
    }
    if (maximum_polyphony < 8 || maximum_polyphony > 256) {   // synthesizer_settings.rs:51-57
        err = "The maximum number of polyphony must be between 8 and 256, but was " + std::to_string(maximum_polyphony) + ".";
        return PVQ_ERR_INVALID_ARG;
    }
    if (maximum_polyphony > SYNTH_MAX_POLYPHONY) {
        err = "unsupported: a polyphony above 64 (a voice object is a lane of one wavefront)";
        return PVQ_ERR_UNSUPPORTED;
    }
    std::unique_ptr<SynthState> s(new SynthState());
    s->bank_ = std::move(bank);
    s->sample_rate_ = sample_rate;
    s->maximum_polyphony_ = maximum_polyphony;
    s->impl_.reset(new Impl());
    Impl& m = *s->impl_;
    for (uint32_t i = 0; i < SYNTH_CHANNELS; ++i) {   // synthesizer.rs:86-89
        m.channels[i].is_percussion_channel = i == 9;
        m.channels[i].reset();
    }
    m.voices.resize(maximum_polyphony);
    for (uint32_t i = 0; i < maximum_polyphony; ++i) {   // voice.rs:81-123
        Voice& v = m.voices[i];
        v.id = i;
        v.sample_rate = v.vol_env.sample_rate = v.mod_env.sample_rate = v.vib_lfo.sample_rate = v.mod_lfo.sample_rate = sample_rate;
        v.min_voice_length = static_cast<size_t>(sample_rate / 500);
    }
    s->effects_ = effects;
    if (effects && !plan_only)
        if (pvq_status st = SynthEffects::create(sample_rate, s->fx_, err)) return st;
    s->last_plan_.clear();
    out = std::move(s);
    return PVQ_OK;
}

uint32_t SynthState::active_voice_count() const { return static_cast<uint32_t>(impl_->active_voice_count); }

pvq_status SynthState::plan(const SynthEvents& events, size_t n_blocks, const uint32_t* snapshot_blocks, size_t n_snapshots, uint32_t stream_index,
                            SynthPlan& out, std::string& err) {
    Impl& m = *impl_;
    const std::string who = "synth: stream " + std::to_string(stream_index);
    if (m.broken) {
        err = who + ": an earlier call failed; the state cannot go on";
        return PVQ_ERR_INVALID_ARG;
    }
    if (events.n && !(events.time && events.channel && events.command && events.data1 && events.data2)) {
        err = who + ": a null event array";
        return PVQ_ERR_INVALID_ARG;
    }
    if (events.n < m.msg_index) {
        err = who + ": the event list is shorter than the " + std::to_string(m.msg_index) + " events already consumed";
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_blocks > 0x7fffffffull / synth::BLOCK) {
        err = who + ": too many blocks in one call";
        return PVQ_ERR_INVALID_ARG;
    }
    for (size_t i = m.msg_index; i < events.n; ++i) {
        const int32_t v[4] = {events.channel[i], events.command[i], events.data1[i], events.data2[i]};
        for (int32_t x : v)
            if (x < 0 || x > 255) {
                err = who + ": event " + std::to_string(i) + " has a byte outside 0 .. 255";
                return PVQ_ERR_INVALID_ARG;
            }
        if (!(events.time[i] == events.time[i]) || (i > 0 && events.time[i] < events.time[i - 1])) {
            err = who + ": event " + std::to_string(i) + " has a time that is NaN or earlier than the event before it";
            return PVQ_ERR_INVALID_ARG;
        }
    }
    if (n_snapshots && !snapshot_blocks) {
        err = who + ": snapshot_blocks is null";
        return PVQ_ERR_INVALID_ARG;
    }
    for (size_t k = 0; k < n_snapshots; ++k)
        if ((k > 0 && snapshot_blocks[k] <= snapshot_blocks[k - 1])) {
            err = who + ": snapshot_blocks must ascend";
            return PVQ_ERR_INVALID_ARG;
        }
    if (out.block_ptr.empty()) out.clear();
    const SynthBank& bank = *bank_;
    const int64_t n_wave = static_cast<int64_t>(bank.wave.size());
    size_t next_snapshot = 0;
    for (size_t b = 0; b < n_blocks; ++b) {
        while (m.msg_index < events.n && events.time[m.msg_index] <= m.current_time) {   // midifile_sequencer.rs:87-103
            const size_t i = m.msg_index++;
            m.process_midi_message(bank, events.channel[i], events.command[i], events.data1[i], events.data2[i]);
        }
        m.current_time += static_cast<double>(synth::BLOCK) / static_cast<double>(sample_rate_);   // :63-64
        size_t i = 0;   // voice_collection.rs:72-87
        while (i != m.active_voice_count) {
            synth::Record rec{};
            synth::Sends snd{};
            const OscStep st = m.voices[i].process(m.channels, n_wave, master_volume_, rec, snd);
            if (st == OscStep::Sounds) {
                out.records.push_back(rec);
                if (effects_) out.sends.push_back(snd);
                ++i;
            } else if (st == OscStep::Ended) {
                m.active_voice_count -= 1;
                std::swap(m.voices[i], m.voices[m.active_voice_count]);
            } else {
                m.broken = true;
                err = who + ", block " + std::to_string(b) + ", key " + std::to_string(m.voices[i].key) +
                      ": the voice would read outside wave_data (a loop shorter than the pitch step, or a sample without its guard "
                      "point): the reference panics here";
                return PVQ_ERR_INVALID_ARG;
            }
        }
        out.block_ptr.push_back(static_cast<uint32_t>(out.records.size()));
        if (next_snapshot < n_snapshots && snapshot_blocks[next_snapshot] == b) {
            for (size_t k = 0; k < m.active_voice_count; ++k)   // synthesizer.rs:525
                out.snapshots.push_back(SynthActiveVoice{m.voices[k].key, m.voices[k].current_mix_gain_left, m.voices[k].current_mix_gain_right});
            out.snapshot_ptr.push_back(static_cast<uint32_t>(out.snapshots.size()));
            ++next_snapshot;
        }
    }
    return PVQ_OK;
}

void synth_replay(const SynthBank& bank, const SynthPlan& plan, size_t n_blocks, synth::Lane* lanes, uint32_t* lane_desc, float* left, float* right,
                  SynthEffects* fx, float master_volume) {
    const int16_t* wave = bank.wave.data();
    for (size_t b = 0; b < n_blocks; ++b) {
        float* l = left + b * synth::BLOCK;
        float* r = right + b * synth::BLOCK;
        std::fill(l, l + synth::BLOCK, 0.0f);   // synthesizer.rs:367-370
        std::fill(r, r + synth::BLOCK, 0.0f);
        if (fx) {   // synthesizer.rs:393-475: the five sums in one walk (each is a sum over the same records in the same order)
            float in[3][synth::BLOCK] = {}, out[4][synth::BLOCK];
            float* const sum[synth::FX_CHANNELS] = {l, r, in[0], in[1], in[2]};
            for (uint32_t k = plan.block_ptr[b]; k < plan.block_ptr[b + 1]; ++k) {
                const synth::Record& rec = plan.records[k];
                if (rec.flags & synth::F_START) lane_desc[rec.voice] = rec.desc;
                const synth::SampleDesc& d = bank.descs[lane_desc[rec.voice]];
                synth::MixGain g[synth::FX_CHANNELS];
                synth::fx_gains(rec, plan.sends[k], g);
                bool add[synth::FX_CHANNELS];
                for (int c = 0; c < synth::FX_CHANNELS; ++c) add[c] = g[c].mode != synth::MIX_SKIP;
                synth::Walk w = synth::walk_begin(rec, d, lanes[rec.voice]);
                synth::walk_span<synth::FX_CHANNELS>(rec, d, wave, lanes[rec.voice], w, g, 0, synth::BLOCK, [&](int t, const float (&p)[synth::FX_CHANNELS]) {
                    for (int c = 0; c < synth::FX_CHANNELS; ++c)
                        if (add[c]) sum[c][t] += p[c];
                });
                synth::walk_end(rec, lanes[rec.voice], w);
            }
            fx->process(1, in[0], in[1], in[2], out[0], out[1], out[2], out[3]);
            for (int t = 0; t < synth::BLOCK; ++t) {
                l[t] = synth::fx_final(l[t], out[0][t], out[2][t], master_volume);
                r[t] = synth::fx_final(r[t], out[1][t], out[3][t], master_volume);
            }
            continue;
        }
        for (uint32_t k = plan.block_ptr[b]; k < plan.block_ptr[b + 1]; ++k) {   // synthesizer.rs:372-391
            const synth::Record& rec = plan.records[k];
            if (rec.flags & synth::F_START) lane_desc[rec.voice] = rec.desc;
            const synth::MixGain gl = synth::mix_gain(rec.gain[0], rec.gain[1]), gr = synth::mix_gain(rec.gain[2], rec.gain[3]);
            synth::walk_block(rec, bank.descs[lane_desc[rec.voice]], wave, lanes[rec.voice], gl, gr, [&](int t, float pl, float pr) {
                if (gl.mode != synth::MIX_SKIP) l[t] += pl;
                if (gr.mode != synth::MIX_SKIP) r[t] += pr;
            });
        }
    }
}

pvq_status SynthState::render(const SynthEvents& events, size_t n_blocks, const uint32_t* snapshot_blocks, size_t n_snapshots, float* left, float* right,
                              std::string& err) {
    if (n_blocks && (!left || !right)) {
        err = "synth state: left and right are needed";
        return PVQ_ERR_INVALID_ARG;
    }
    last_plan_.clear();
    if (pvq_status st = plan(events, n_blocks, snapshot_blocks, n_snapshots, 0, last_plan_, err)) return st;
    if (effects_ && !fx_) {
        err = "synth state: a state made for planning alone has no effect state to render with";
        return PVQ_ERR_INVALID_ARG;
    }
    synth_replay(*bank_, last_plan_, n_blocks, lanes_, lane_desc_, left, right, fx_.get(), master_volume_);
    return PVQ_OK;
}

pvq_status synth_plan_streams(SynthState* const* states, const SynthEvents* events, const size_t* n_blocks, size_t n, const uint32_t* snapshot_blocks,
                              size_t n_snapshots, SynthPlan* plans, std::string& err) {
    std::vector<pvq_status> status(n, PVQ_OK);
    std::vector<std::string> texts(n);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t s = next.fetch_add(1); s < n; s = next.fetch_add(1)) {
            plans[s].clear();
            status[s] = states[s]->plan(events[s], n_blocks[s], snapshot_blocks, n_snapshots, static_cast<uint32_t>(s), plans[s], texts[s]);
        }
    };
    const size_t n_threads = std::min<size_t>({n, 16, std::max(1u, std::thread::hardware_concurrency())});   // never the machine's core count
    if (n_threads <= 1) {
        work();
    } else {
        std::vector<std::thread> threads;
        for (size_t t = 0; t < n_threads; ++t) threads.emplace_back(work);
        for (std::thread& t : threads) t.join();
    }
    for (size_t s = 0; s < n; ++s)
        if (status[s] != PVQ_OK) {
            err = texts[s];
            return status[s];
        }
    return PVQ_OK;
}

}  // namespace pvq
