// synth_math.hpp — the one copy of the synthesizer's audio-rate arithmetic, for the host replay (synth_host.cpp, g++) and the device
// replay (synth_batch.hip): rustysynth_fork/src/oscillator.rs:112-176 (the fixed-point linear interpolation, looping and not),
// bi_quad_filter.rs:77-99 (the recurrence and the inactive branch's state copy), synthesizer.rs:478-495 with array_math.rs:8-24
// (the gain decision of write_block and the products it adds).
//
// Integer arithmetic is the reference's i64 arithmetic; every f32 expression is the reference's, operation for operation, in the
// written order, FMA contraction off on both sides (the host unit is built with -ffp-contract=off), no libm call, f32 subnormals
// kept (the default mode of a kernel, and of the host), as condition_batch.hip's header says for the AGC.  All that a block needs
// besides the samples is a Record of the plan (synth_host.hpp): nothing here decides which voices exist.
#pragma once

#include "color_math.hpp"

#define PVQ_SYNTH_FLAT PVQ_HD __attribute__((always_inline))
#if defined(__clang__)
#define PVQ_SYNTH_UNROLL _Pragma("unroll")
#else
#define PVQ_SYNTH_UNROLL _Pragma("GCC unroll 8")
#endif

namespace pvq {
namespace synth {

constexpr int BLOCK = 64;                                    // SynthesizerSettings::DEFAULT_BLOCK_SIZE
constexpr int FRAC_BITS = 24;                                // oscillator.rs:33
constexpr int64_t FRAC_UNIT = int64_t{1} << FRAC_BITS;       // oscillator.rs:34
constexpr float FP_TO_SAMPLE = 1.0f / 549755813888.0f;       // oscillator.rs:35: 1 / (32768 * FRAC_UNIT) = 2^-39
constexpr float NON_AUDIBLE = 1.0e-3f;                       // soundfont_math.rs:11
constexpr float INVERSE_BLOCK_SIZE = 1.0f / 64.0f;           // synthesizer.rs:96

// flags of a record
constexpr uint32_t F_START = 1u;    // Voice::start ran since the voice's last record: position = start, filter memory cleared
constexpr uint32_t F_LOOP = 2u;     // Oscillator::looping
constexpr uint32_t F_FILTER = 4u;   // BiQuadFilter::active
constexpr uint32_t F_ENDS = 8u;     // a sample without a loop reaches its end inside this block: zeros from there on

// One sounding voice in one block: all that the audio rate needs.  64 bytes, four 16-byte pieces.
struct Record {
    uint32_t voice;               // the voice object, 0 .. maximum_polyphony - 1: whose position and filter memory this block continues
    uint32_t flags;
    uint32_t ratio_lo, ratio_hi;  // pitch_ratio_fp (i64, oscillator.rs:103)
    float a[5];                   // BiQuadFilter a0 .. a4 (bi_quad_filter.rs:101-107)
    float gain[4];                // previous left, current left, previous right, current right: already times master_volume
    uint32_t desc;                // the sample descriptor (a record with F_START alone reads it)
    int32_t key;                  // Voice::key
    uint32_t stage;               // the volume envelope's stage after this block's step (envelope_stage.rs)
};
static_assert(sizeof(Record) == 64, "four 16-byte pieces");

// RegionPair::get_sample_start / _end / _start_loop / _end_loop (region_pair.rs:23-37): indices into wave_data
struct SampleDesc {
    int32_t start, end, start_loop, end_loop;
};

// what a voice object carries from block to block
struct Lane {
    int64_t position_fp = 0;                          // oscillator.rs:29
    float x1 = 0.0f, x2 = 0.0f, y1 = 0.0f, y2 = 0.0f;   // bi_quad_filter.rs:19-22
};

constexpr int MIX_SKIP = 0, MIX_CONST = 1, MIX_SLOPE = 2;
struct MixGain {
    float a, step;
    int mode;
};
// write_block's decision (synthesizer.rs:485-494)
PVQ_SYNTH_FLAT MixGain mix_gain(float previous_gain, float current_gain) {
    PVQ_FP_STRICT
    const float m = previous_gain > current_gain ? previous_gain : current_gain;   // SoundFontMath::max
    if (m < NON_AUDIBLE) return MixGain{0.0f, 0.0f, MIX_SKIP};
    const float diff = current_gain - previous_gain;
    if ((diff < 0.0f ? -diff : diff) < 1.0e-3f) return MixGain{current_gain, 0.0f, MIX_CONST};
    return MixGain{previous_gain, INVERSE_BLOCK_SIZE * diff, MIX_SLOPE};
}

// one sample of the interpolation (oscillator.rs:129-133 / 166-170)
PVQ_SYNTH_FLAT float osc_value(int32_t x1, int32_t x2, int64_t a_fp) {
    PVQ_FP_STRICT
    return FP_TO_SAMPLE * static_cast<float>(static_cast<int64_t>(x1) * FRAC_UNIT + a_fp * static_cast<int64_t>(x2 - x1));   // (x1 << 24: x1 may be negative)
}

// one step of the recurrence (bi_quad_filter.rs:82-89)
PVQ_SYNTH_FLAT float biquad_step(const float a[5], Lane& s, float input) {
    PVQ_FP_STRICT
    const float output = a[0] * input + a[1] * s.x1 + a[2] * s.x2 - a[3] * s.y1 - a[4] * s.y2;
    s.x2 = s.x1;
    s.x1 = input;
    s.y2 = s.y1;
    s.y1 = output;
    return output;
}

// A record's walk in pieces, for a caller that cannot hold a whole block's products at once (synth_batch.hip's effects kernel walks
// half a block at a time): walk_begin, walk_span over [t_begin, t_end) (multiples of 8) with N gains, walk_end.  What passes from
// span to span is the Walk and the gains, which walk_span steps by the reference's repeated addition (array_math.rs:16-24).
struct Walk {
    int64_t pos;
    float in1, in2;   // the block's last and last but one oscillator samples
};
PVQ_SYNTH_FLAT Walk walk_begin(const Record& r, const SampleDesc& d, Lane& s) {
    if (r.flags & F_START) {   // region_ex.rs:15-39 -> oscillator.rs:87; voice.rs:167
        s.position_fp = static_cast<int64_t>(d.start) << FRAC_BITS;
        s.x1 = s.x2 = s.y1 = s.y2 = 0.0f;
    }
    return Walk{s.position_fp, 0.0f, 0.0f};
}
// sink(t, products[N]): products[c] = gain c * the voice's sample; a channel whose mode is MIX_SKIP is not to be added.  The reads
// of eight samples are issued before the first of them enters the filter chain: positions do not depend on data.
template <int N, class Sink>
PVQ_SYNTH_FLAT void walk_span(const Record& r, const SampleDesc& d, const int16_t* wave, Lane& s, Walk& w, MixGain (&g)[N], int t_begin, int t_end,
                              Sink&& sink) {
    PVQ_FP_STRICT
    const int64_t ratio_fp = static_cast<int64_t>((static_cast<uint64_t>(r.ratio_hi) << 32) | r.ratio_lo);
    const bool looping = (r.flags & F_LOOP) != 0, active = (r.flags & F_FILTER) != 0;
    const int64_t end_loop_fp = static_cast<int64_t>(d.end_loop) << FRAC_BITS;
    const int64_t loop_length = static_cast<int64_t>(d.end_loop) - d.start_loop, loop_length_fp = loop_length * FRAC_UNIT;
    int64_t pos = w.pos;
    float in1 = w.in1, in2 = w.in2;
    for (int t0 = t_begin; t0 < t_end; t0 += 8) {
        int32_t w1[8], w2[8];
        int64_t a_fp[8];
        PVQ_SYNTH_UNROLL
        for (int k = 0; k < 8; ++k) {
            if (looping) {   // oscillator.rs:155-172
                if (pos >= end_loop_fp) pos -= loop_length_fp;
                const int64_t index1 = pos >> FRAC_BITS;
                int64_t index2 = index1 + 1;
                if (index2 >= d.end_loop) index2 -= loop_length;
                w1[k] = wave[index1];
                w2[k] = wave[index2];
                a_fp[k] = pos & (FRAC_UNIT - 1);
                pos += ratio_fp;
            } else {         // oscillator.rs:116-135; past the end the block is filled with zeros and the position stays
                const int64_t index = pos >> FRAC_BITS;
                const bool live = index < d.end;
                w1[k] = live ? wave[index] : 0;
                w2[k] = live ? wave[index + 1] : 0;
                a_fp[k] = live ? pos & (FRAC_UNIT - 1) : 0;
                pos += live ? ratio_fp : 0;
            }
        }
        PVQ_SYNTH_UNROLL
        for (int k = 0; k < 8; ++k) {
            const float x = osc_value(w1[k], w2[k], a_fp[k]);
            in2 = in1;
            in1 = x;
            const float y = active ? biquad_step(r.a, s, x) : x;
            float p[N];
            PVQ_SYNTH_UNROLL
            for (int c = 0; c < N; ++c) {
                p[c] = g[c].a * y;
                g[c].a += g[c].step;
            }
            sink(t0 + k, p);
        }
    }
    w.pos = pos;
    w.in1 = in1;
    w.in2 = in2;
}
PVQ_SYNTH_FLAT void walk_end(const Record& r, Lane& s, const Walk& w) {
    s.position_fp = w.pos;
    if (!(r.flags & F_FILTER)) {   // bi_quad_filter.rs:93-98
        s.x2 = w.in2;
        s.x1 = w.in1;
        s.y2 = s.x2;
        s.y1 = s.x1;
    }
}

// A record's 64 samples: oscillator, filter, and the two products a_left * x and a_right * x that write_block adds.
// sink(t, left product, right product).
template <class Sink>
PVQ_SYNTH_FLAT void walk_block(const Record& r, const SampleDesc& d, const int16_t* wave, Lane& s, MixGain gl, MixGain gr, Sink&& sink) {
    MixGain g[2] = {gl, gr};
    Walk w = walk_begin(r, d, s);
    walk_span<2>(r, d, wave, s, w, g, 0, BLOCK, [&](int t, const float (&p)[2]) { sink(t, p[0], p[1]); });
    walk_end(r, s, w);
}

}  // namespace synth
}  // namespace pvq
