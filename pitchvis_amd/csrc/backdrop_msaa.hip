// backdrop_msaa.hip — the backdrop's tile kernel with four samples a pixel (backdrop_math.hpp has the rule; backdrop_batch.hip the
// list kernel, whose records do not depend on the sample count, and the dispatch).
//
// backdrop_tiles_msaa keeps the shape of backdrop_tiles: a workgroup per (row, 16 x 16 pixels), a wave per 8 x 8 block, a lane per
// pixel; the same 64-record ballot box test against the wave's block, the set bits visited in ascending order with the record at a
// wave-uniform address (backdrop_device.hpp, walk<4>).  A lane keeps its pixel's four destinations (16 registers) and four sample
// positions (8); per hit it evaluates the three edges at the four positions and blends the covered samples; at the end it resolves
// and issues the one 16-byte store of the one-sample kernel.  No LDS, no scratch, and no per-sample image leaves the kernel.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#include "backdrop_device.hpp"

namespace pvq {

namespace {
__global__ __launch_bounds__(256) __attribute__((flatten)) void backdrop_tiles_msaa(BackdropArgs a) {
#pragma clang fp contract(off)
    constexpr uint32_t S = 4;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const stage::TilePixel px = stage::tile_pixel(wave, lane, a.W, a.H, a.vh);
    float wx[S], wy[S];
#pragma unroll
    for (uint32_t k = 0; k < S; ++k) {
        float fx, fy;
        backdrop::sample_fraction(S, k, fx, fy);
        backdrop::sample_world(px.bx0 + (lane & 7u), px.by0 + (lane >> 3), a.W, a.H, a.vh, fx, fy, wx[k], wy[k]);
    }
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        float4 first = make_float4(a.clear[0], a.clear[1], a.clear[2], a.clear[3]);
        if (a.background && px.inside) first = reinterpret_cast<const float4*>(a.background)[px.pixel];
        float dst[4 * S];
#pragma unroll
        for (uint32_t k = 0; k < S; ++k) {   // every sample starts from the pixel
            dst[4 * k] = first.x; dst[4 * k + 1] = first.y; dst[4 * k + 2] = first.z; dst[4 * k + 3] = first.w;
        }
        backdrop::walk<S>(a.net, a.n_net, lane, px.bx0, px.by0, wx, wy, dst);
        backdrop::walk<S>(a.list + static_cast<size_t>(r) * a.cap * BACKDROP_WORDS, a.counts[r], lane, px.bx0, px.by0, wx, wy, dst);
        if (px.inside)
            reinterpret_cast<float4*>(a.image)[g * a.W * a.H + px.pixel] =
                make_float4(backdrop::resolve4(dst[0], dst[4], dst[8], dst[12]), backdrop::resolve4(dst[1], dst[5], dst[9], dst[13]),
                            backdrop::resolve4(dst[2], dst[6], dst[10], dst[14]), backdrop::resolve4(dst[3], dst[7], dst[11], dst[15]));
    }
}
}  // namespace

void launch_backdrop_tiles_msaa(const BackdropArgs& a, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL(backdrop_tiles_msaa, grid, dim3(256), 0, stream, a);
}

}  // namespace pvq
