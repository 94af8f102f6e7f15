// note_epoch.hip — see note_epoch.hpp.
#include "note_epoch.hpp"

#include "note_epoch_math.hpp"

namespace pvq {

namespace {
constexpr int NE_THREADS = 256;

// Thread j walks its own cycle (a few passes of four hashes each; the longest walk grows with log n) and reads one entry of d_idx:
// order(j) < n by the walk's own condition, so no read leaves d_idx.
__global__ __launch_bounds__(NE_THREADS) void ne_gather(const uint32_t* __restrict__ idx, uint32_t* __restrict__ order, const NoteEpochKeys k) {
    const uint32_t j = blockIdx.x * NE_THREADS + threadIdx.x;
    if (j >= k.n) return;
    order[j] = idx[ne_order(k, j)];
}
}  // namespace

void note_epoch_gather(const uint32_t* d_idx, uint32_t* d_order, uint32_t n, uint64_t seed, uint64_t epoch, hipStream_t stream) {
    const NoteEpochKeys k = ne_keys(seed, epoch, n);
    hipLaunchKernelGGL(ne_gather, dim3((n + NE_THREADS - 1) / NE_THREADS), dim3(NE_THREADS), 0, stream, d_idx, d_order, k);
}

}  // namespace pvq
