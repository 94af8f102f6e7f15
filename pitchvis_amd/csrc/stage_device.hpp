// stage_device.hpp — device side of what the batch stages' kernels share (raster_batch.hip, backdrop_batch.hip, scene_batch.hip,
// overlay_batch.hip): how a row of a piece of a call maps to the call's rows, and a lane's pixel in the 16 x 16 tile kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "raster_math.hpp"

namespace pvq {
namespace stage {

constexpr int TILE = 16;   // pixels a side of a workgroup's tile: 2 x 2 waves of 8 x 8

// A piece holds frames f0 .. f0 + pf of every stream, stream by stream: its row r is the call's row stream * n_frames + frame.
__device__ __forceinline__ size_t piece_row(uint32_t r, uint32_t pf, uint32_t n_frames, uint32_t f0) {
    return static_cast<size_t>(r / pf) * n_frames + f0 + r % pf;
}

// Workgroup blockIdx.x is a tile of the W x H image, row-major; wave `wave` of its four takes the 8 x 8 block at (bx0, by0), lane
// `lane` the pixel (lane & 7, lane >> 3) of that block.
struct TilePixel {
    uint32_t bx0, by0;
    bool inside;     // the pixel lies on the image
    float wx, wy;    // its world position
    size_t pixel;    // its index in a [H][W] image
};
__device__ __forceinline__ TilePixel tile_pixel(uint32_t wave, uint32_t lane, uint32_t W, uint32_t H, float vh) {
#pragma clang fp contract(off)
    TilePixel p;
    const uint32_t tiles_x = (W + TILE - 1) / TILE;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    p.bx0 = tx * TILE + (wave & 1u) * 8u;
    p.by0 = ty * TILE + (wave >> 1) * 8u;
    const uint32_t i = p.bx0 + (lane & 7u), j = p.by0 + (lane >> 3);
    p.inside = i < W && j < H;
    raster::pixel_world(i, j, W, H, vh, p.wx, p.wy);
    p.pixel = static_cast<size_t>(j) * W + i;
    return p;
}
// The same for a kernel launched over a list of tiles (overlay_batch.hip): `tile` is the workgroup's row-major tile number.
__device__ __forceinline__ TilePixel tile_pixel_of(uint32_t tile, uint32_t wave, uint32_t lane, uint32_t W, uint32_t H, float vh, uint32_t& i,
                                                   uint32_t& j) {
#pragma clang fp contract(off)
    TilePixel p;
    const uint32_t tiles_x = (W + TILE - 1) / TILE;
    p.bx0 = (tile % tiles_x) * TILE + (wave & 1u) * 8u;
    p.by0 = (tile / tiles_x) * TILE + (wave >> 1) * 8u;
    i = p.bx0 + (lane & 7u);
    j = p.by0 + (lane >> 3);
    p.inside = i < W && j < H;
    raster::pixel_world(i, j, W, H, vh, p.wx, p.wy);
    p.pixel = static_cast<size_t>(j) * W + i;
    return p;
}

}  // namespace stage
}  // namespace pvq
