// backdrop_device.hpp — device side of what the backdrop's two units share (backdrop_batch.hip: the list kernel, the one-sample tile
// kernel and the dispatch; backdrop_msaa.hip: the four-sample tile kernel): the kernels' argument block, the walk over a list of
// finished records for one lane's pixel, templated on the sample count, and the launcher of the four-sample kernel.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "backdrop_math.hpp"
#include "stage_device.hpp"

namespace pvq {

constexpr uint32_t BACKDROP_WORDS = sizeof(backdrop::Tri) / 16;   // 16-byte words a record

struct BackdropArgs {
    const uint32_t* bass_lit;    // [rows] or null
    const float* bass_rgba;      // [rows][4]
    const float *line_pos, *line_rgba, *disc_pos, *disc_rgba, *hist_pos, *hist_rgba, *graph_pos, *graph_rgba;
    const uint32_t* peak_count;
    uint32_t max_peaks, line_quads, graph_quads;
    float t_spec[4], t_hist[4], t_graph[4];
    const float* background;     // [H][W][4] or null
    const float* bass_quads;     // [n_bass][4][2]
    const uint4* net;            // [n_net] records
    uint32_t n_bass, n_net;
    uint32_t n_streams, n_frames, f0, pf;   // the call's frames; this piece is frames f0 .. f0 + pf
    uint32_t cap;                // records a row of the workspace holds
    uint32_t W, H;
    float vh;
    float clear[4];
    uint4* list;                 // [n_streams * pf][cap] records
    uint32_t* counts;            // [n_streams * pf]
    float* image;                // [n_streams][n_frames][H][W][4]
};

// backdrop_tiles_msaa over a piece whose lists backdrop_lists has finished on `stream`: the grid of backdrop_tiles (a workgroup per
// tile, gridDim.y rows with a stride), 256 lanes.  Defined in backdrop_msaa.hip.
void launch_backdrop_tiles_msaa(const BackdropArgs& a, dim3 grid, hipStream_t stream);

namespace backdrop {

// m records, in order, over the S sample positions (wx[k], wy[k]) of one pixel of the wave's block at (bx0, by0); dst + 4 k is
// sample k's destination.  A wave that hits nothing — most waves, most of the time: the layers are thin lines — waits for one
// load per round, so a round takes the box words of DEPTH x 64 records at once.  A record's box holds every pixel with a covered
// sample (backdrop_math.hpp, at tri_box), so the box test is the same for every S.
// The instantiation for 1 is held to the machine code the one-sample kernel had before there was a template: plain pointers and
// no loop over its one sample (with references to arrays, or a loop of one trip, the compiler allocates its registers otherwise).
template <uint32_t S>
__device__ __forceinline__ void walk(const uint4* list, uint32_t m, uint32_t lane, uint32_t bx0, uint32_t by0, const float* wx,
                                     const float* wy, float* dst) {
#pragma clang fp contract(off)
    constexpr uint32_t DEPTH = 4;
    constexpr uint32_t WORDS = BACKDROP_WORDS;
    for (uint32_t c0 = 0; c0 < m; c0 += 64u * DEPTH) {   // (m is the wave's)
        unsigned long long masks[DEPTH];
#pragma unroll
        for (uint32_t d = 0; d < DEPTH; ++d) {
            const uint32_t idx = c0 + 64u * d + lane;
            bool hit = false;
            if (idx < m) {
                const uint4 b = list[static_cast<size_t>(idx) * WORDS];
                hit = !((b.x & 0xFFFFu) > bx0 + 7u || (b.x >> 16) < bx0 || (b.y & 0xFFFFu) > by0 + 7u || (b.y >> 16) < by0);
            }
            masks[d] = __ballot(hit);
        }
#pragma unroll
        for (uint32_t d = 0; d < DEPTH; ++d) {
            unsigned long long mask = masks[d];
            while (mask) {
                const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(mask));        // ascending: the list's order
                mask &= mask - 1ull;
                const uint4* rec = list + static_cast<size_t>(c0 + 64u * d + k) * WORDS;   // wave-uniform, < m
                const uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3], q4 = rec[4];
                backdrop::Tri t;
                t.positive = q0.z;
                t.edge[0][0] = __uint_as_float(q1.x); t.edge[0][1] = __uint_as_float(q1.y); t.edge[0][2] = __uint_as_float(q1.z); t.edge[0][3] = __uint_as_float(q1.w);
                t.edge[1][0] = __uint_as_float(q2.x); t.edge[1][1] = __uint_as_float(q2.y); t.edge[1][2] = __uint_as_float(q2.z); t.edge[1][3] = __uint_as_float(q2.w);
                t.edge[2][0] = __uint_as_float(q3.x); t.edge[2][1] = __uint_as_float(q3.y); t.edge[2][2] = __uint_as_float(q3.z); t.edge[2][3] = __uint_as_float(q3.w);
                if constexpr (S == 1u) {
                    if (backdrop::covers(t, wx[0], wy[0])) {
                        const float src[4] = {__uint_as_float(q4.x), __uint_as_float(q4.y), __uint_as_float(q4.z), __uint_as_float(q4.w)};
                        raster::blend(src, dst);
                    }
                } else {
                    const float src[4] = {__uint_as_float(q4.x), __uint_as_float(q4.y), __uint_as_float(q4.z), __uint_as_float(q4.w)};
#pragma unroll
                    for (uint32_t s = 0; s < S; ++s)
                        if (backdrop::covers(t, wx[s], wy[s])) raster::blend(src, dst + 4 * s);
                }
            }
        }
    }
}

}  // namespace backdrop
}  // namespace pvq
