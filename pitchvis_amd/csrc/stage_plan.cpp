// stage_plan.cpp — see stage_plan.hpp.
#include "stage_plan.hpp"

#include <algorithm>

#include "raster_math.hpp"

namespace pvq {

bool stage_image_ok(const char* who, uint32_t width, uint32_t height, float viewport_height, std::string& err) {
    if (width == 0 || height == 0 || width > raster::MAX_IMAGE || height > raster::MAX_IMAGE) {
        err = std::string(who) + ": width and height are 1 .. 4096";
        return false;
    }
    if (!(viewport_height >= 0.0f) || !raster::finite_f(viewport_height)) {
        err = std::string(who) + ": viewport_height is 0 (the viewer's) or positive and finite";
        return false;
    }
    return true;
}

bool stage_mode_ok(const char* who, int visuals_mode, std::string& err) {
    if (visuals_mode >= scene::FULL && visuals_mode <= scene::GALAXY) return true;
    err = std::string(who) + ": unknown visuals mode";
    return false;
}

bool stage_frames_ok(const char* who, size_t n_frames, uint32_t n_streams, std::string& err) {
    if (n_frames <= 0x7FFFFFFFull && n_frames * n_streams <= 0x7FFFFFFFull) return true;
    err = std::string(who) + ": too many frames in one call";
    return false;
}

size_t stage_piece_frames(size_t n_frames, uint32_t n_streams, size_t per_row, size_t limit) {
    return std::min<size_t>(n_frames, std::max<size_t>(1, limit / (per_row * n_streams)));
}

}  // namespace pvq
