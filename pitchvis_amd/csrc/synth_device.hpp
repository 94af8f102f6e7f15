// synth_device.hpp — what the two replay units (synth_batch.hip: the dry kernel and the handle; synth_fx_batch.hip: the effects
// kernel) share: the argument blocks of the kernels.  Private to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "synth_fx_math.hpp"
#include "synth_math.hpp"

namespace pvq {

constexpr int LDT = synth::BLOCK + 1;   // dwords of a tile row

struct SynthStream {
    float* left;
    float* right;
    uint32_t n_blocks;
    uint32_t ptr_base;   // the stream's first entry of block_ptr
};

struct SynthArgs {
    const SynthStream* tab;         // [gridDim.x]
    const uint32_t* block_ptr;      // per stream [n_blocks + 1]: indices into records
    const uint4* records;           // four pieces a record
    const int16_t* wave;
    const synth::SampleDesc* descs;
    uint4* lanes;                   // [gridDim.x][2][64]
};

struct SynthFxArgs {
    SynthArgs dry;
    const uint4* sends;         // two pieces a record
    const uint32_t* layout;     // synth::FxLayout
    const float* table;         // [layout.table]
    float* reverb;              // [gridDim.x][layout.total]
    float* store;               // [gridDim.x][16]
    float* ring;                // [gridDim.x][2][layout.ring]
    unsigned long long* count;  // [gridDim.x]
    float master_volume;
};

// synth_replay_fx over n_streams workgroups of one wavefront (synth_fx_batch.hip); the caller checks hipGetLastError
void launch_synth_replay_fx(const SynthFxArgs& args, uint32_t n_streams, hipStream_t stream);

}  // namespace pvq
