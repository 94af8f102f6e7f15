// present_host.hpp — the present stage for ONE picture on the host: bloom over the mip pyramid, the display transform and the sRGB
// encode of a linear HDR image [H][W][4] (present_math.hpp has the arithmetic, include/pvq.h the rule).  The one-image face and
// second reference of PresentBatch (present_batch.hpp), and the host planning that the device stage shares: the settings' checks,
// the mip chain's layout in a workspace and the cut of a call's rows into pieces.  Plain data in, plain data out: no HIP.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "present_math.hpp"

namespace pvq {

// Every field finite, high_pass_frequency > 0, the two enums in range, max_mip_dimension 0 (512) or 4 .. 4096.  false leaves the
// text, which begins with `who`, in err (as stage_plan.hpp's checks do).
bool present_settings_ok(const char* who, const present::Settings& s, std::string& err);
// max_mip_dimension 0 resolved to 512
present::Settings present_resolved(const present::Settings& s);

// A row's mip chain in a workspace of 16-byte texels: mip k at texel offset[k], `texels` in all.
struct PresentPlan {
    present::Mips mips;
    size_t offset[present::MAX_MIPS];
    size_t texels;
};
// false (a picture so much wider than high that mip 0 would pass 16384 texels a side) leaves the text in err
bool present_plan(const char* who, uint32_t W, uint32_t H, uint32_t max_mip_dimension, PresentPlan& out, std::string& err);
// Rows in a piece of a call, 1 .. n_rows, so that the pieces' mip chains stay within `limit` bytes wherever one row's does.
size_t present_piece_rows(size_t n_rows, const PresentPlan& plan, size_t limit);

// B_0 .. B_{n_mips - 1} at this intensity; n_mips 1 .. MAX_MIPS
void present_blend_factors(const present::Settings& s, float intensity, uint32_t n_mips, float* out);

// image [H][W][4] -> out_rgba8 [H][W][4] bytes and, where out_hdr is not null, the bloomed linear picture [H][W][4] before the
// display transform (it may be `image`).  The settings are resolved and checked; plan: present_plan's of W, H and the settings.
void present_frame(const present::Settings& s, const PresentPlan& plan, uint32_t W, uint32_t H, const float* image, float intensity, uint8_t* out_rgba8, float* out_hdr);

}  // namespace pvq
