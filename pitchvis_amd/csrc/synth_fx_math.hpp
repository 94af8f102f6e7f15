// synth_fx_math.hpp — the one copy of the synthesizer's effect arithmetic (rustysynth_fork/src/reverb.rs, chorus.rs,
// synthesizer.rs:393-475), for the host replay (synth_host.cpp, g++) and the device replay (synth_batch.hip): the buffer lengths and
// their layout, the comb and all-pass steps with their flushes, the chorus interpolation, the wet mix with its condition, the final
// sum.  As in synth_math.hpp: every f32 / f64 expression is the reference's in the written order, FMA contraction off on both
// sides, no libm call (the chorus delay table, which needs sin, is made on the host: synth_host.hpp), f32 subnormals kept.
//
// What recurs and what does not.  Every buffer position read in a block was written before the block began: the shortest comb is
// 405 samples and the shortest all-pass 82 (both at 16 kHz), a block is 64.  So the comb OUTPUTS, the all-pass chain and — since it
// has no feedback: its ring holds inputs only — the chorus are functions of values older than the block and of the block's inputs:
// a lane per sample.  Only the comb's filter_store is a recurrence from sample to sample, with a flush in it: a lane per comb.
#pragma once

#include "synth_math.hpp"

namespace pvq {
namespace synth {

// One record's effect gains, parallel to the plan's records (include/pvq.h: pvq_synth_sends).  The mix gains in them are NOT times
// master_volume (synthesizer.rs:404-415, 449-454), so they cannot be read from Record::gain.
struct Sends {
    float chorus[4];   // previous left, current left, previous right, current right: send * mix gain
    float reverb[2];   // previous, current: (0.015 * send) * (mix gain left + mix gain right)
    uint32_t pad[2];
};
static_assert(sizeof(Sends) == 32, "two 16-byte pieces");

constexpr int FX_COMBS = 8, FX_ALLPASSES = 4;                // per channel (reverb.rs:61-95)
constexpr int FX_BUFFERS = 2 * (FX_COMBS + FX_ALLPASSES);    // comb c * 8 + i, then all-pass 16 + c * 4 + k; c = 0 left, 1 right
constexpr int FX_FIRST_ALLPASS = 2 * FX_COMBS;
constexpr float FX_FLUSH = 1.0e-6f;                          // reverb.rs:298, 303, 372
constexpr float FX_REVERB_GAIN = 0.015f;                     // Reverb::FIXED_GAIN
constexpr float FX_ALLPASS_FEEDBACK = 0.5f;                  // reverb.rs:98
constexpr double FX_CHORUS_DELAY = 0.002, FX_CHORUS_DEPTH = 0.0019, FX_CHORUS_FREQUENCY = 0.4;   // synthesizer.rs:124

// f64 `round() as usize` of a positive value, without libm
PVQ_SYNTH_FLAT uint32_t fx_round(double v) {
    const uint32_t f = static_cast<uint32_t>(v);
    return v - static_cast<double>(f) >= 0.5 ? f + 1 : f;
}

struct FxLayout {
    uint32_t len[FX_BUFFERS];   // Reverb::scale_tuning (reverb.rs:147-149)
    uint32_t off[FX_BUFFERS];   // where a buffer starts in a stream's reverb state
    uint32_t total;             // floats of a stream's reverb state
    uint32_t ring;              // Chorus::new: ((sample_rate * (delay + depth)) as usize) + 2, per channel
    uint32_t table;             // entries of the delay table: round(sample_rate / frequency)
    uint32_t pad;
};
PVQ_SYNTH_FLAT FxLayout fx_layout(int32_t sample_rate) {
    constexpr uint32_t comb[FX_COMBS] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}, allpass[FX_ALLPASSES] = {556, 441, 341, 225}, spread = 23;
    FxLayout l{};
    const double sr = static_cast<double>(sample_rate);
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < FX_COMBS; ++i) l.len[c * FX_COMBS + i] = fx_round(sr / 44100.0 * static_cast<double>(comb[i] + c * spread));
        for (int k = 0; k < FX_ALLPASSES; ++k)
            l.len[FX_FIRST_ALLPASS + c * FX_ALLPASSES + k] = fx_round(sr / 44100.0 * static_cast<double>(allpass[k] + c * spread));
    }
    for (int i = 0; i < FX_BUFFERS; ++i) {
        l.off[i] = l.total;
        l.total += l.len[i];
    }
    l.ring = static_cast<uint32_t>(sr * (FX_CHORUS_DELAY + FX_CHORUS_DEPTH)) + 2;
    l.table = fx_round(sr / FX_CHORUS_FREQUENCY);
    return l;
}

// Reverb::new's setters (reverb.rs:121-124, 195-236) in f32: feedback 0.84, damp1 0.2, damp2 0.8, wet1 1, wet2 0
struct ReverbConstants {
    float feedback, damp1, damp2, wet1, wet2;
};
PVQ_SYNTH_FLAT ReverbConstants reverb_constants() {
    PVQ_FP_STRICT
    const float scale_wet = 3.0f, initial_wet = 1.0f / scale_wet, width = 1.0f;
    const float wet = initial_wet * scale_wet;
    const float room_size = 0.5f * 0.28f + 0.7f, damp = 0.5f * 0.4f;
    return ReverbConstants{room_size, damp, 1.0f - damp, wet * (width / 2.0f + 0.5f), wet * ((1.0f - width) / 2.0f)};
}

PVQ_SYNTH_FLAT float fx_flush(float v) { return (v < 0.0f ? -v : v) < FX_FLUSH ? 0.0f : v; }

// the sum of the eight comb outputs onto 0, in comb order (reverb.rs:161-170, 298-300, 308): value(i) = the buffer's value at this sample
template <class Value>
PVQ_SYNTH_FLAT float comb_output_sum(Value&& value) {
    PVQ_FP_STRICT
    float acc = 0.0f;
    PVQ_SYNTH_UNROLL
    for (int i = 0; i < FX_COMBS; ++i) acc += fx_flush(value(i));
    return acc;
}

// one sample of a comb's state (reverb.rs:297-307): the value the buffer takes at this position
PVQ_SYNTH_FLAT float comb_step(float buffer_value, float input, float& filter_store, const ReverbConstants& k) {
    PVQ_FP_STRICT
    const float output = fx_flush(buffer_value);
    filter_store = fx_flush((output * k.damp2) + (filter_store * k.damp1));
    return input + (filter_store * k.feedback);
}

// one sample of an all-pass (reverb.rs:369-377): returns its output, `buffer_value` becomes what the buffer takes
PVQ_SYNTH_FLAT float allpass_step(float& buffer_value, float input) {
    PVQ_FP_STRICT
    const float bufout = fx_flush(buffer_value);
    buffer_value = input + (bufout * FX_ALLPASS_FEEDBACK);
    return bufout - input;
}

// the final width mix and its condition (reverb.rs:185-192)
PVQ_SYNTH_FLAT void reverb_wet_mix(float& left, float& right, const ReverbConstants& k) {
    PVQ_FP_STRICT
    if (1.0f - k.wet1 > 1.0e-3f || k.wet2 > 1.0e-3f) {
        const float l = left, r = right;
        left = l * k.wet1 + r * k.wet2;
        right = r * k.wet1 + l * k.wet2;
    }
}

// One chorus sample (chorus.rs:60-75): where it reads, from the RING index (so that position - index1 has the reference's bits).
// 1 <= delay < ring - 1 (checked when the table is made) keeps index1 inside the ring.
struct ChorusTap {
    uint32_t index1, index2;
    double a;
};
PVQ_SYNTH_FLAT ChorusTap chorus_tap(uint32_t ring_index, float delay, uint32_t ring) {
    PVQ_FP_STRICT
    double position = static_cast<double>(ring_index) - static_cast<double>(delay);
    if (position < 0.0) position += static_cast<double>(ring);
    const uint32_t index1 = static_cast<uint32_t>(position);
    const uint32_t index2 = index1 + 1 == ring ? 0 : index1 + 1;
    return ChorusTap{index1, index2, position - static_cast<double>(index1)};
}
PVQ_SYNTH_FLAT float chorus_mix(const ChorusTap& tap, float x1, float x2) {
    PVQ_FP_STRICT
    const double d1 = static_cast<double>(x1), d2 = static_cast<double>(x2);
    return static_cast<float>(d1 + tap.a * (d2 - d1));
}

// dry + master_volume * chorus output, then + master_volume * reverb output (synthesizer.rs:430-439, 465-474; array_math.rs:8-13)
PVQ_SYNTH_FLAT float fx_final(float dry, float chorus_out, float reverb_out, float master_volume) {
    PVQ_FP_STRICT
    float v = dry;
    v += master_volume * chorus_out;
    v += master_volume * reverb_out;
    return v;
}

// the three effect inputs' gains of a record beside its two dry ones, in the order the tiles and sums use: dry left, dry right,
// chorus left, chorus right, reverb
constexpr int FX_CHANNELS = 5;
PVQ_SYNTH_FLAT void fx_gains(const Record& r, const Sends& s, MixGain (&g)[FX_CHANNELS]) {
    g[0] = mix_gain(r.gain[0], r.gain[1]);
    g[1] = mix_gain(r.gain[2], r.gain[3]);
    g[2] = mix_gain(s.chorus[0], s.chorus[1]);
    g[3] = mix_gain(s.chorus[2], s.chorus[3]);
    g[4] = mix_gain(s.reverb[0], s.reverb[1]);
}

}  // namespace synth
}  // namespace pvq
