// note_epoch.hpp — the one kernel an epoch of the note trainer adds to the step's (note_trainer.hpp): the whole epoch's gathered
// order, d_order[j] = d_idx[order(j)] with the order of note_epoch_math.hpp, one element per thread.  NoteTrainer::epoch copies a
// batch's slice of d_order into the step's index array, device to device, and runs the step's own launches on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pvq {

// d_idx, d_order: n entries each, 1 <= n <= 2^25 (note_trainer_check_epoch).  Queues only.
void note_epoch_gather(const uint32_t* d_idx, uint32_t* d_order, uint32_t n, uint64_t seed, uint64_t epoch, hipStream_t stream);

}  // namespace pvq
