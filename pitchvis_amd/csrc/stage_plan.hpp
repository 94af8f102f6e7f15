// stage_plan.hpp — host side of what the batch stages (scene, panels, raster, backdrop) and their one-frame host faces share: the
// checks on image, visuals mode and frame count, and the cut of a call into pieces whose rows fit a workspace.  Plain data in, plain
// data out: no HIP, no device pointer, no environment (the blockdft_plan.cpp pattern).  A check that fails returns false and leaves
// the text, which begins with the caller's `who`, in err.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace pvq {

// width and height 1 .. raster::MAX_IMAGE, then viewport_height 0 (the viewer's) or positive and finite
bool stage_image_ok(const char* who, uint32_t width, uint32_t height, float viewport_height, std::string& err);
bool stage_mode_ok(const char* who, int visuals_mode, std::string& err);   // scene::FULL .. scene::GALAXY
// n_frames and the call's rows, n_frames * n_streams, are at most 2^31 - 1: the kernels count both in 32 bits
bool stage_frames_ok(const char* who, size_t n_frames, uint32_t n_streams, std::string& err);
// Frames of every stream in a piece of a call, 1 .. n_frames, so that a piece's rows (per_row bytes each) stay within `limit` bytes
// wherever one frame of all streams does.
size_t stage_piece_frames(size_t n_frames, uint32_t n_streams, size_t per_row, size_t limit);

}  // namespace pvq
