// readout_batch.hip — the tuning-drift readout for many rows (readout_batch.hpp).
//
// readout_atlas (once per handle, at create; a workgroup per 16 x 16 tile of a glyph's cell, text_coverage's shape: a wave per 8 x 8
// block, a lane per pixel): the glyph's chords are staged through LDS in chunks of text::CHUNK, one 16-byte load a thread, and every
// lane reads the same chord (a 16-byte LDS broadcast) and adds text::segment_area in list order — the host face's sum, so the atlas
// has the host face's bits.
// readout_draw (per call; a workgroup per (tile, row) over the tiles the widest admissible box and its glyph cells can meet, rows on
// gridDim.y with a stride loop past the grid cap as text_blend): the workgroup's first wave formats the row's value and lays the
// string out, a lane per glyph slot — every lane runs the sequential pen fold up to the end, so the pen has the host's bits — and
// leaves the placed cells in LDS; then a lane per pixel blends the box and the glyphs in string order.  A pixel that neither covers
// is neither loaded nor stored; a drawn pixel costs one 16-byte load and one 16-byte store.  Formatting and drawing are one kernel:
// see DESIGN.md 6k.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#include "readout_batch.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "stage_device.hpp"
#include "stage_plan.hpp"

namespace pvq {

namespace {
static_assert(stage::TILE * stage::TILE == 256 && text::CHUNK == 256, "a thread per pixel, and per staged segment");
static_assert(readout::MAX_SLOTS <= 64, "a lane of the first wave per glyph slot");

struct AtlasArgs {
    const float4* segments;       // every glyph's list, one after the other
    const uint4* entries;         // [gridDim.x]: glyph, tile column and tile row within its cell, 0
    const readout::Cell* cells;   // [N_GLYPHS]
    const uint2* ranges;          // [N_GLYPHS]: the glyph's first segment, its segments
    float* atlas;
};

__global__ __launch_bounds__(256) void readout_atlas(AtlasArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 s_seg[text::CHUNK];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint4 e = a.entries[blockIdx.x];
    const readout::Cell cell = a.cells[e.x];
    const uint2 range = a.ranges[e.x];
    const uint32_t ci = e.y * stage::TILE + (wave & 1u) * 8u + (lane & 7u), cj = e.z * stage::TILE + (wave >> 1) * 8u + (lane >> 3);
    const bool in_cell = ci < cell.w && cj < cell.h;
    const float X = static_cast<float>(cell.x0 + static_cast<int32_t>(ci)), Y = static_cast<float>(cell.y0 + static_cast<int32_t>(cj));
    float sum = 0.0f;
    for (uint32_t base = 0; base < range.y; base += text::CHUNK) {   // range.y is the workgroup's: every thread takes every barrier
        const uint32_t m = min(text::CHUNK, range.y - base);
        __syncthreads();                                              // the chunk before has been read
        if (tid < m) s_seg[tid] = a.segments[static_cast<size_t>(range.x) + base + tid];
        __syncthreads();
        if (in_cell)
            for (uint32_t k = 0; k < m; ++k) {
                const float4 s = s_seg[k];
                sum += text::segment_area(text::Segment{s.x, s.y, s.z, s.w}, X, Y);
            }
    }
    if (in_cell) a.atlas[static_cast<size_t>(cell.offset) + static_cast<size_t>(cj) * cell.w + ci] = text::coverage_of(sum);
}

struct DrawArgs {
    float* image;                 // [rows][H][W][4]
    const float* values;          // [rows]
    const float* atlas;
    const readout::Cell* cells;   // [N_GLYPHS]
    uint32_t W, H, rows;
    uint32_t tx0, ty0, tiles_x;   // the grid's tiles: columns tx0 .. tx0 + tiles_x - 1, rows from ty0
    float font_px, baseline;
};

__global__ __launch_bounds__(256) void readout_draw(DrawArgs a) {
#pragma clang fp contract(off)
    __shared__ float s_advance[readout::N_GLYPHS];
    __shared__ int4 s_cell[readout::N_GLYPHS];      // x0, y0, w, h
    __shared__ uint32_t s_offset[readout::N_GLYPHS];
    __shared__ int4 s_place[readout::MAX_SLOTS];    // a slot's cell on the image: first column, first row, w, h
    __shared__ uint2 s_source[readout::MAX_SLOTS];  // its coverages' offset in the atlas; 1: the value's colour, 0: white
    __shared__ float s_row[8];                      // xl, xr, yt, yb, the value's linear colour
    __shared__ uint32_t s_slots;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    if (tid < readout::N_GLYPHS) {
        const readout::Cell c = a.cells[tid];
        s_advance[tid] = c.advance;
        s_cell[tid] = make_int4(c.x0, c.y0, static_cast<int>(c.w), static_cast<int>(c.h));
        s_offset[tid] = c.offset;
    }
    const uint32_t i = (a.tx0 + blockIdx.x % a.tiles_x) * stage::TILE + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t j = (a.ty0 + blockIdx.x / a.tiles_x) * stage::TILE + (wave >> 1) * 8u + (lane >> 3);
    const bool inside = i < a.W && j < a.H;
    const size_t per_row = static_cast<size_t>(a.W) * a.H, pixel = static_cast<size_t>(j) * a.W + i;
    for (uint32_t r = blockIdx.y; r < a.rows; r += gridDim.y) {   // a.rows is the grid's: every thread takes every barrier
        __syncthreads();                                           // the cells are staged; the row before has been drawn
        if (tid < readout::MAX_SLOTS) {
            uint64_t text;
            float rounded, pen;
            const uint32_t n = readout::N_PREFIX + readout::value_glyphs(a.values[r], text, rounded);
            const float text_w = readout::pen_fold(s_advance, text, n, tid, pen);
            const readout::Box box = readout::box_of(a.W, a.H, text_w, a.font_px);
            if (tid < n) {
                const uint32_t g = readout::slot_glyph(text, tid);
                const int4 c = s_cell[g];
                const int ox = static_cast<int>(readout::origin_column(box, pen)), by = static_cast<int>(readout::baseline_row(box, a.baseline));
                s_place[tid] = make_int4(ox + c.x, by + c.y, c.z, c.w);
                s_source[tid] = make_uint2(s_offset[g], tid >= readout::N_PREFIX ? 1u : 0u);
            }
            if (tid == 0) {
                float srgb[3];
                readout::value_srgb(rounded, srgb);
                s_row[0] = box.xl, s_row[1] = box.xr, s_row[2] = box.yt, s_row[3] = box.yb;
                s_row[4] = scene::srgb_to_linear(srgb[0]);
                s_row[5] = scene::srgb_to_linear(srgb[1]);
                s_row[6] = scene::srgb_to_linear(srgb[2]);
                s_slots = n;
            }
        }
        __syncthreads();
        if (!inside) continue;
        const readout::Box box{s_row[0], s_row[1], s_row[2], s_row[3]};
        float4* at = reinterpret_cast<float4*>(a.image) + (static_cast<size_t>(r) * per_row + pixel);
        float dst[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool have = false;
        if (readout::in_box(box, i, j)) {
            const float4 c = *at;
            dst[0] = c.x, dst[1] = c.y, dst[2] = c.z, dst[3] = c.w;
            have = true;
            readout::blend_box(dst);
        }
        const uint32_t n = s_slots;
        for (uint32_t s = 0; s < n; ++s) {
            const int4 p = s_place[s];
            const int dx = static_cast<int>(i) - p.x, dy = static_cast<int>(j) - p.y;
            if (dx < 0 || dy < 0 || dx >= p.z || dy >= p.w) continue;
            const uint2 src = s_source[s];
            const float cov = a.atlas[static_cast<size_t>(src.x) + static_cast<size_t>(dy) * static_cast<size_t>(p.z) + static_cast<size_t>(dx)];
            if (cov == 0.0f) continue;
            if (!have) {
                const float4 c = *at;
                dst[0] = c.x, dst[1] = c.y, dst[2] = c.z, dst[3] = c.w;
                have = true;
            }
            const float rgb[3] = {src.y ? s_row[4] : 1.0f, src.y ? s_row[5] : 1.0f, src.y ? s_row[6] : 1.0f};
            text::blend_label(rgb, cov, dst);
        }
        if (have) *at = make_float4(dst[0], dst[1], dst[2], dst[3]);
    }
}
}  // namespace

pvq_status ReadoutBatch::create(int device_id, TextFont& font, uint32_t width, uint32_t height, float ui_scale, std::unique_ptr<ReadoutBatch>& out) {
    out.reset();
    std::string err;
    std::unique_ptr<ReadoutBatch> b(new ReadoutBatch());
    if (pvq_status s = readout_plan("readout batch", font, width, height, ui_scale, b->plan_, err)) {
        set_last_error(err);
        return s;
    }
    const ReadoutPlan& plan = b->plan_;
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_tiles_ = plan.any ? (plan.tx1 - plan.tx0 + 1) * (plan.ty1 - plan.ty0 + 1) : 0;
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        std::vector<uint32_t> entries, ranges;
        for (uint32_t g = 0; g < readout::N_GLYPHS; ++g) {
            const readout::Cell& c = plan.cells[g];
            ranges.insert(ranges.end(), {plan.first_segment[g], plan.n_segments[g]});
            for (uint32_t ty = 0; ty * stage::TILE < c.h; ++ty)
                for (uint32_t tx = 0; tx * stage::TILE < c.w; ++tx) entries.insert(entries.end(), {g, tx, ty, 0u});
        }
        if (pvq_status s = b->cells_.upload(plan.cells, sizeof(plan.cells))) return s;
        if (pvq_status s = b->atlas_.reserve(std::max<size_t>(plan.atlas_floats, 1) * sizeof(float))) return s;
        if (!entries.empty()) {
            DeviceBuffer d_segments, d_entries, d_ranges;   // needed by readout_atlas only
            if (pvq_status s = d_segments.upload(plan.segments.data(), plan.segments.size() * sizeof(text::Segment))) return s;
            if (pvq_status s = d_entries.upload(entries.data(), entries.size() * sizeof(uint32_t))) return s;
            if (pvq_status s = d_ranges.upload(ranges.data(), ranges.size() * sizeof(uint32_t))) return s;
            AtlasArgs a{};
            a.segments = d_segments.as<float4>();
            a.entries = d_entries.as<uint4>();
            a.cells = b->cells_.as<readout::Cell>();
            a.ranges = d_ranges.as<uint2>();
            a.atlas = b->atlas_.as<float>();
            hipLaunchKernelGGL(readout_atlas, dim3(static_cast<unsigned>(entries.size() / 4)), dim3(256), 0, nullptr, a);
            PVQ_HIP(hipGetLastError());
            PVQ_HIP(hipDeviceSynchronize());   // the atlas is ready for any stream, and the kernel's inputs may go
        }
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status ReadoutBatch::rows_device(size_t n_rows, const float* d_values, float* d_image, hipStream_t stream) {
    if (!d_values || !d_image) {
        set_last_error("readout batch: d_values and d_image_inout are needed");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(d_image) & 15) || (reinterpret_cast<uintptr_t>(d_values) & 3)) {
        set_last_error("readout batch: d_image_inout must be 16-byte aligned, d_values 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("readout batch", n_rows, 1, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched readout stage runs on a GPU; this handle has none (pvq_readout_frame is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_rows == 0 || n_tiles_ == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    DrawArgs a{};
    a.image = d_image;
    a.values = d_values;
    a.atlas = atlas_.as<float>();
    a.cells = cells_.as<readout::Cell>();
    a.W = plan_.width;
    a.H = plan_.height;
    a.rows = static_cast<uint32_t>(n_rows);
    a.tx0 = plan_.tx0;
    a.ty0 = plan_.ty0;
    a.tiles_x = plan_.tx1 - plan_.tx0 + 1;
    a.font_px = plan_.font_px;
    a.baseline = plan_.baseline;
    hipLaunchKernelGGL(readout_draw, dim3(n_tiles_, static_cast<unsigned>(std::min<size_t>(n_rows, 65535))), dim3(256), 0, stream, a);
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status ReadoutBatch::get_atlas(uint32_t codepoint, int32_t* x0, int32_t* y0, uint32_t* w, uint32_t* h, float* advance, size_t cap_floats,
                                   float* out) {
    const uint32_t g = readout::glyph_of(codepoint);
    if (g == readout::N_GLYPHS) {
        set_last_error("readout batch: the codepoint is none the readout emits (\"Tuning drift: \", 0-9, '-', \"NaN\", \"inf\")");
        return PVQ_ERR_INVALID_ARG;
    }
    const readout::Cell& c = plan_.cells[g];
    if (x0) *x0 = c.x0;
    if (y0) *y0 = c.y0;
    if (w) *w = c.w;
    if (h) *h = c.h;
    if (advance) *advance = c.advance;
    const size_t n = static_cast<size_t>(c.w) * c.h;
    if (!out || n == 0) return PVQ_OK;
    if (cap_floats < n) {
        set_last_error("readout batch: out is smaller than the cell; ask for its size first");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {   // the host face's atlas, made when first asked for
        if (plan_.coverage.size() != plan_.atlas_floats) readout_cover(plan_);
        std::copy_n(plan_.coverage.begin() + c.offset, n, out);
        return PVQ_OK;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    PVQ_HIP(hipMemcpy(out, atlas_.as<float>() + c.offset, n * sizeof(float), hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
