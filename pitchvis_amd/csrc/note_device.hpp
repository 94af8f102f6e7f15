// note_device.hpp — the device pieces the note units share (note_model.hip, note_model_half.hip, note_trainer.hip,
// note_trainer_half.hip): the conv pair behind a pooled feature, the count of the conv values, and the epilogue of the trainer's
// products.  Inline device code only: nothing here is a kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "note_model_plan.hpp"
#include "note_trainer_plan.hpp"

namespace pvq {

constexpr int NOTE_CONV_VALUES = NM_CH * NM_KW + NM_CH;   // 96 conv values or gradients: weights [16][5], then bias [16]

// the two conv positions a pooled position covers (train.py:89-90), as nm_conv_fc1 evaluates them: bias first, taps in order, fused
__device__ __forceinline__ void conv_pair(const float* w5, float cb, const float* x, float& e, float& o) {
    e = cb;
    o = cb;
#pragma unroll
    for (int j = 0; j < NM_KW; ++j) {
        e = fmaf(w5[j], x[j], e);
        o = fmaf(w5[j], x[2 + j], o);
    }
}

// what happens to an element of a product before it is stored; G: the type the gate is stored in (float, or the 16-bit activation)
enum { E_RAW = 0, E_BIAS = 1, E_HIDDEN = 2, E_GATE = 3 };
template <class G>
struct NoteEpi {
    int kind;            // E_RAW: nothing.  E_BIAS: + bias[col].  E_HIDDEN: ReLU(+ bias[col]), then dropout.  E_GATE: * (gate > 0 ? scale : 0)
    const float* bias;   // [N]
    const G* gate;       // E_GATE: [M][ldg], the activation this gradient flows back through (as stored: after ReLU and dropout)
    uint32_t ldg;        //   its row length
    float scale;         // 1 / (1 - p) where dropout applies, else 1
    int drop;            // E_HIDDEN: apply the mask
    uint32_t threshold;  // keep when the 24-bit draw >= threshold
    uint64_t key;        // nt_layer_key(seed, step, layer)
};
template <class G>
__device__ __forceinline__ float epi_apply(const NoteEpi<G>& e, float v, uint32_t row, uint32_t col) {
    if (e.kind == E_BIAS) return v + e.bias[col];
    if (e.kind == E_HIDDEN) {
        v = fmaxf(v + e.bias[col], 0.0f);
        if (e.drop) v = nt_keep(e.key, row, col, e.threshold) ? v * e.scale : 0.0f;
        return v;
    }
    if (e.kind == E_GATE) return static_cast<float>(e.gate[static_cast<size_t>(row) * e.ldg + col]) > 0.0f ? v * e.scale : 0.0f;
    return v;
}

}  // namespace pvq
