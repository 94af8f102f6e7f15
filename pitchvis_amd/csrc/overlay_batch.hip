// overlay_batch.hip — the spectrogram quad and the chroma boxes for many streams (overlay_batch.hpp).
//
// overlay_draw (frame-parallel with a halo, the tile kernels' shape: a workgroup per (row, 16 x 16 pixels), a wave per 8 x 8
// block, a lane per pixel; launched over the static list of tiles that the quad's or the boxes' pixel box meets): a frame's
// picture depends on the rows of the h - 2 frames before it only, so frame f of a call reads the row `age` frames back from the
// call's own rows where f - age >= 0 and from the handle's ring otherwise, and nothing where that frame never was or the age is
// that of the zeroed row.  A lane loads one texel (4 bytes: lanes along x read one bin of neighbouring frames' rows, lanes along
// y neighbouring bins), and only a pixel that a texel with alpha or a lit box covers is loaded (16 bytes), blended and stored (16
// bytes).  The decode tables (2.2 KB) are staged in LDS once per workgroup.
// overlay_keep (after the draw, never before: later frames of a call would overwrite ring rows that earlier frames still read):
// the call's last min(n_frames, h) rows go to their ring rows.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#include "overlay_batch.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "stage_device.hpp"
#include "stage_plan.hpp"

namespace pvq {

namespace {
constexpr uint32_t TABLE_WORDS = sizeof(overlay::Tables) / sizeof(float);
constexpr uint32_t LINEAR_AT = 0, ALPHA_AT = 256, BOX_AT = 512;
static_assert(offsetof(overlay::Tables, alpha) == ALPHA_AT * 4 && offsetof(overlay::Tables, box) == BOX_AT * 4, "table layout");

struct OverlayArgs {
    const uint32_t* rows;    // [n_streams][n_frames][n_bins] texels, or null
    const float* chroma;     // [n_streams][n_frames][12], or null
    float* image;            // [n_streams][n_frames][H][W][4]
    const uint32_t* ring;    // [n_streams][h][n_bins] texels
    const float* tables;     // overlay::Tables
    const uint32_t* tiles;   // [gridDim.x]
    uint32_t n_streams, n_frames, n_bins, h, W, H;
    uint32_t w0;             // write index of the call's first frame: frames seen % h
    uint32_t seen;           // min(frames seen, h)
    uint32_t active;         // QUAD_TILE | BOX_TILE: the layers this call draws
    float vh, ui_scale;
    float quad[4];
};

__global__ __launch_bounds__(256) __attribute__((flatten)) void overlay_draw(OverlayArgs a) {
#pragma clang fp contract(off)
    __shared__ float s_tab[TABLE_WORDS];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    for (uint32_t k = tid; k < TABLE_WORDS; k += 256u) s_tab[k] = a.tables[k];
    __syncthreads();
    const uint32_t entry = a.tiles[blockIdx.x];
    const uint32_t layers = entry & a.active;   // the workgroup's
    if (!layers) return;
    uint32_t i, j;
    const stage::TilePixel px = stage::tile_pixel_of(entry & TILE_MASK, wave, lane, a.W, a.H, a.vh, i, j);
    if (!px.inside) return;
    const bool with_quad = (layers & QUAD_TILE) != 0u;
    const uint32_t pc = (layers & BOX_TILE) ? overlay::box_at(i, j, a.H, a.ui_scale) : overlay::BOXES;
    const uint32_t rows = a.n_streams * a.n_frames;
    for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const uint32_t s = r / a.n_frames, f = r % a.n_frames;
        uint32_t texel = 0u;
        if (with_quad) {
            const uint32_t w = (a.w0 + f) % a.h, next = w + 1u == a.h ? 0u : w + 1u;
            uint32_t tx, ty;
            if (overlay::quad_texel(a.quad, a.n_bins, a.h, overlay::scroll_of(next, a.h), px.wx, px.wy, tx, ty)) {   // tx < n_bins
                const uint32_t age = overlay::age_of(ty, next, a.h);                                               // < h
                if (age != a.h - 1u) {
                    if (age <= f) {
                        texel = a.rows[(static_cast<size_t>(r) - age) * a.n_bins + tx];        // row r - age is frame f - age of stream s
                    } else if (age - f <= a.seen) {
                        const uint32_t k = w + a.h - age;                                      // 0 < k < 2 h
                        texel = a.ring[(static_cast<size_t>(s) * a.h + (k >= a.h ? k - a.h : k)) * a.n_bins + tx];
                    }
                }
            }
        }
        float strength = 0.0f;
        if (pc < overlay::BOXES) strength = a.chroma[static_cast<size_t>(r) * overlay::BOXES + pc];
        const bool quad_draws = overlay::texel_draws(texel), box_draws = overlay::strength_draws(strength);
        if (!quad_draws && !box_draws) continue;
        float4* at = reinterpret_cast<float4*>(a.image) + (static_cast<size_t>(r) * a.W * a.H + px.pixel);
        const float4 c = *at;
        float dst[4] = {c.x, c.y, c.z, c.w};
        if (quad_draws) overlay::blend_texel(s_tab + LINEAR_AT, s_tab + ALPHA_AT, texel, dst);
        if (box_draws) overlay::blend_box(s_tab + BOX_AT + 3u * pc, strength, dst);
        *at = make_float4(dst[0], dst[1], dst[2], dst[3]);
    }
}

// rows f_first .. f_first + m of every stream's n_frames go to ring rows (w_first + k) % h
__global__ __launch_bounds__(256) void overlay_keep(const uint32_t* rows, uint32_t* ring, uint32_t n_streams, uint32_t n_frames, uint32_t n_bins,
                                                    uint32_t h, uint32_t f_first, uint32_t m, uint32_t w_first) {
    const size_t per_stream = static_cast<size_t>(m) * n_bins, total = per_stream * n_streams;
    for (size_t idx = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; idx < total; idx += static_cast<size_t>(gridDim.x) * 256u) {
        const size_t s = idx / per_stream, rem = idx % per_stream;
        const uint32_t k = static_cast<uint32_t>(rem / n_bins), bin = static_cast<uint32_t>(rem % n_bins);
        ring[(s * h + (w_first + k) % h) * n_bins + bin] = rows[(s * n_frames + f_first + k) * n_bins + bin];
    }
}
}  // namespace

pvq_status OverlayBatch::create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, uint32_t history_rows, float viewport_height,
                                float ui_scale, const float* quad, const float* colors, uint32_t n_streams, uint32_t width, uint32_t height,
                                std::unique_ptr<OverlayBatch>& out) {
    out.reset();
    if (octaves == 0 || buckets_per_octave == 0 || n_streams == 0) {
        set_last_error("overlay batch: octaves, buckets_per_octave and n_streams must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_image_ok("overlay batch", width, height, viewport_height, err) || !overlay_args_ok("overlay batch", history_rows, ui_scale, quad, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (n < overlay::MIN_BINS || n > overlay::MAX_BINS) {
        set_last_error("unsupported: the batched overlay takes 3 .. 1024 bins");
        return PVQ_ERR_UNSUPPORTED;
    }
    if (static_cast<uint64_t>(n_streams) * n > 0x7FFFFFFFull) {
        set_last_error("overlay batch: too many streams");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<OverlayBatch> b(new OverlayBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_streams_ = n_streams;
    b->n_bins_ = static_cast<uint32_t>(n);
    b->h_ = history_rows == 0 ? overlay::HISTORY_ROWS : history_rows;
    b->width_ = width;
    b->height_ = height;
    b->vh_ = viewport_height == 0.0f ? raster::VIEWPORT_HEIGHT : viewport_height;
    b->ui_scale_ = ui_scale == 0.0f ? 1.0f : ui_scale;
    if (quad) std::copy(quad, quad + 4, b->quad_);
    else overlay::reference_quad(b->n_bins_, b->h_, b->quad_);
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        overlay::Tables tables;
        overlay_tables(colors, tables);
        if (pvq_status s = b->tables_.upload(&tables, sizeof(tables))) return s;
        const std::vector<uint32_t> tiles = overlay_tiles(width, height, b->vh_, b->ui_scale_, b->quad_);
        b->n_tiles_ = static_cast<uint32_t>(tiles.size());
        if (b->n_tiles_)
            if (pvq_status s = b->tiles_.upload(tiles.data(), tiles.size() * sizeof(uint32_t))) return s;
        const size_t ring_bytes = static_cast<size_t>(n_streams) * b->h_ * b->n_bins_ * 4;
        if (pvq_status s = b->ring_.reserve(ring_bytes)) return s;
        PVQ_HIP(hipMemset(b->ring_.as<void>(), 0, ring_bytes));
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status OverlayBatch::frames_device(size_t n_frames, const uint8_t* d_rows, const float* d_chroma, float* d_image, hipStream_t stream) {
    if (!d_image || (!d_rows && !d_chroma)) {
        set_last_error("overlay batch: d_image_inout is needed, and d_rows or d_chroma");
        return PVQ_ERR_INVALID_ARG;
    }
    if (reinterpret_cast<uintptr_t>(d_image) & 15) {
        set_last_error("overlay batch: d_image_inout must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_chroma)) & 3) {
        set_last_error("overlay batch: d_rows and d_chroma must be 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("overlay batch", n_frames, n_streams_, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched overlay runs on a GPU; this handle has none (pvq_overlay_frame is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_frames == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));

    OverlayArgs a{};
    a.rows = reinterpret_cast<const uint32_t*>(d_rows);
    a.chroma = d_chroma;
    a.image = d_image;
    a.ring = ring_.as<uint32_t>();
    a.tables = tables_.as<float>();
    a.tiles = tiles_.as<uint32_t>();
    a.n_streams = n_streams_;
    a.n_frames = static_cast<uint32_t>(n_frames);
    a.n_bins = n_bins_;
    a.h = h_;
    a.W = width_;
    a.H = height_;
    a.w0 = static_cast<uint32_t>(seen_ % h_);
    a.seen = static_cast<uint32_t>(std::min<uint64_t>(seen_, h_));
    a.active = (d_rows ? QUAD_TILE : 0u) | (d_chroma ? BOX_TILE : 0u);
    a.vh = vh_;
    a.ui_scale = ui_scale_;
    std::copy(quad_, quad_ + 4, a.quad);
    const size_t rows = static_cast<size_t>(n_streams_) * n_frames;
    if (n_tiles_) hipLaunchKernelGGL(overlay_draw, dim3(n_tiles_, static_cast<unsigned>(std::min<size_t>(rows, 65535))), dim3(256), 0, stream, a);
    if (d_rows) {
        const uint32_t m = static_cast<uint32_t>(std::min<size_t>(n_frames, h_)), f_first = a.n_frames - m;
        const size_t texels = static_cast<size_t>(n_streams_) * m * n_bins_;
        hipLaunchKernelGGL(overlay_keep, dim3(static_cast<unsigned>(std::min<size_t>((texels + 255) / 256, 256 * 32))), dim3(256), 0, stream, a.rows,
                           ring_.as<uint32_t>(), n_streams_, a.n_frames, n_bins_, h_, f_first, m, static_cast<uint32_t>((seen_ + f_first) % h_));
        seen_ += n_frames;
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status OverlayBatch::get_texture(uint32_t stream_index, uint8_t* out, uint32_t* write_index) {
    if (stream_index >= n_streams_ || !out) {
        set_last_error("overlay batch: stream_index out of range or a null array");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched overlay runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    const size_t row = static_cast<size_t>(n_bins_) * 4;
    std::vector<uint8_t> ring(row * h_);
    PVQ_HIP(hipMemcpy(ring.data(), ring_.as<uint8_t>() + static_cast<size_t>(stream_index) * h_ * row, ring.size(), hipMemcpyDeviceToHost));
    // the texture holds ring row k at row h - 1 - k, and the row of the next write index zeroed
    const uint32_t next = static_cast<uint32_t>(seen_ % h_);
    for (uint32_t k = 0; k < h_; ++k) {
        uint8_t* dst = out + static_cast<size_t>(h_ - 1u - k) * row;
        if (k == next) std::fill_n(dst, row, uint8_t{0});
        else std::copy(ring.begin() + k * row, ring.begin() + (k + 1) * row, dst);
    }
    if (write_index) *write_index = next;
    return PVQ_OK;
}

}  // namespace pvq
