// text_batch.hip — the pitch-name labels for many rows (text_batch.hpp).
//
// text_coverage (once per handle, at create; a workgroup per (tile, label) entry of the layer, the tile kernels' shape: a wave per
// 8 x 8 block, a lane per pixel): the label's segments are staged through LDS in chunks of text::CHUNK, one 16-byte load a thread,
// and every lane reads the same segment (a 16-byte LDS broadcast) and adds text::segment_area in list order — the host face's sum,
// so the layer has the host face's bits.
// text_blend (per call; a workgroup per (touched tile, row), rows on gridDim.y with a stride loop past the grid cap as
// overlay_draw): a workgroup walks its tile's entries in label order; a lane whose pixel no label covers leaves at once, a covered
// pixel costs one 16-byte load and one 16-byte store a row.  The layer (1 KB an entry) is shared by every row.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#include "text_batch.hpp"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "stage_device.hpp"
#include "stage_plan.hpp"

namespace pvq {

namespace {
constexpr uint32_t TILE_PIXELS = stage::TILE * stage::TILE;
constexpr size_t MAX_LAYER_BYTES = size_t{1} << 28;
static_assert(TILE_PIXELS == 256 && text::CHUNK == 256, "a thread per pixel, and per staged segment");

// thread tid's pixel of row-major tile `tile`: wave tid / 64 takes an 8 x 8 block, lane tid % 64 a pixel of it (stage_device.hpp)
__host__ __device__ inline void pixel_of(uint32_t tile, uint32_t tid, uint32_t W, uint32_t& i, uint32_t& j) {
    const uint32_t tiles_x = (W + stage::TILE - 1) / stage::TILE, wave = tid >> 6, lane = tid & 63u;
    i = (tile % tiles_x) * stage::TILE + (wave & 1u) * 8u + (lane & 7u);
    j = (tile / tiles_x) * stage::TILE + (wave >> 1) * 8u + (lane >> 3);
}

struct CoverageArgs {
    const float4* segments;   // every label's list, one after the other
    const uint4* entries;     // [gridDim.x]: tile, label, the label's first segment, its segments
    const uint4* boxes;       // [n_labels]: x0, y0, x1, y1, on the image
    float* layer;             // [gridDim.x][256]
    uint32_t W;
};

__global__ __launch_bounds__(256) void text_coverage(CoverageArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 s_seg[text::CHUNK];
    const uint32_t tid = threadIdx.x;
    const uint4 e = a.entries[blockIdx.x];
    const uint4 box = a.boxes[e.y];
    uint32_t i, j;
    pixel_of(e.x, tid, a.W, i, j);
    const bool in_box = i >= box.x && i <= box.z && j >= box.y && j <= box.w;
    const float X = static_cast<float>(i), Y = static_cast<float>(j);
    float sum = 0.0f;
    for (uint32_t base = 0; base < e.w; base += text::CHUNK) {   // e.w is the workgroup's: every thread takes every barrier
        const uint32_t m = min(text::CHUNK, e.w - base);
        __syncthreads();                                          // the chunk before has been read
        if (tid < m) s_seg[tid] = a.segments[static_cast<size_t>(e.z) + base + tid];
        __syncthreads();
        if (in_box)
            for (uint32_t k = 0; k < m; ++k) {
                const float4 s = s_seg[k];
                sum += text::segment_area(text::Segment{s.x, s.y, s.z, s.w}, X, Y);
            }
    }
    a.layer[static_cast<size_t>(blockIdx.x) * TILE_PIXELS + tid] = in_box ? text::coverage_of(sum) : 0.0f;
}

struct BlendArgs {
    float* image;                  // [rows][H][W][4]
    const float* layer;            // [n_entries][256]
    const uint4* tiles;            // [gridDim.x]: tile, first entry, entries, 0
    const uint32_t* entry_labels;  // [n_entries]
    const float4* colors;          // [n_labels] linear RGB
    uint32_t W, H, rows;
};

__global__ __launch_bounds__(256) void text_blend(BlendArgs a) {
#pragma clang fp contract(off)
    const uint32_t tid = threadIdx.x;
    const uint4 t = a.tiles[blockIdx.x];
    uint32_t i, j;
    pixel_of(t.x, tid, a.W, i, j);
    if (i >= a.W || j >= a.H) return;
    const float* lay = a.layer + static_cast<size_t>(t.y) * TILE_PIXELS + tid;
    const float c_first = lay[0];                                   // most tiles have one entry: its coverage stays in a register
    bool any = c_first != 0.0f;
    for (uint32_t e = 1; e < t.z; ++e) any = any || lay[static_cast<size_t>(e) * TILE_PIXELS] != 0.0f;
    if (!any) return;
    const float4 col_first = a.colors[a.entry_labels[t.y]];
    const size_t per_row = static_cast<size_t>(a.W) * a.H, pixel = static_cast<size_t>(j) * a.W + i;
    for (uint32_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
        float4* at = reinterpret_cast<float4*>(a.image) + (static_cast<size_t>(r) * per_row + pixel);
        const float4 c = *at;
        float dst[4] = {c.x, c.y, c.z, c.w};
        if (c_first != 0.0f) {
            const float rgb[3] = {col_first.x, col_first.y, col_first.z};
            text::blend_label(rgb, c_first, dst);
        }
        for (uint32_t e = 1; e < t.z; ++e) {
            const float cov = lay[static_cast<size_t>(e) * TILE_PIXELS];
            if (cov == 0.0f) continue;
            const float4 col = a.colors[a.entry_labels[t.y + e]];
            const float rgb[3] = {col.x, col.y, col.z};
            text::blend_label(rgb, cov, dst);
        }
        *at = make_float4(dst[0], dst[1], dst[2], dst[3]);
    }
}
}  // namespace

pvq_status TextBatch::create(int device_id, TextFont& font, const pvq_text_label* labels, uint32_t n, float viewport_height, uint32_t width,
                             uint32_t height, std::unique_ptr<TextBatch>& out) {
    out.reset();
    std::string err;
    if (!stage_image_ok("text batch", width, height, viewport_height, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    std::vector<TextLabelPlan> plans;
    if (pvq_status s = text_plan("text batch", font, labels, n, width, height, viewport_height == 0.0f ? raster::VIEWPORT_HEIGHT : viewport_height,
                                 plans, err)) {
        set_last_error(err);
        return s;
    }
    // the layer's index: (tile, label) sorted by tile, then label
    const uint32_t tiles_x = (width + stage::TILE - 1) / stage::TILE;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    size_t n_pairs = 0;
    for (const TextLabelPlan& p : plans) n_pairs += p.n_tiles();
    if (n_pairs * TILE_PIXELS * sizeof(float) > MAX_LAYER_BYTES) {
        set_last_error("unsupported: the labels' boxes meet more tiles than a coverage layer of 256 MiB holds");
        return PVQ_ERR_UNSUPPORTED;
    }
    pairs.reserve(n_pairs);
    for (uint32_t l = 0; l < n; ++l) {
        const TextLabelPlan& p = plans[l];
        if (!p.on_image) continue;
        for (uint32_t ty = p.y0 / stage::TILE; ty <= p.y1 / stage::TILE; ++ty)
            for (uint32_t tx = p.x0 / stage::TILE; tx <= p.x1 / stage::TILE; ++tx) pairs.emplace_back(ty * tiles_x + tx, l);
    }
    std::sort(pairs.begin(), pairs.end());
    std::unique_ptr<TextBatch> b(new TextBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_labels_ = n;
    b->width_ = width;
    b->height_ = height;
    std::vector<uint32_t> first_segment(n, 0u), tiles, entry_labels;
    std::vector<text::Segment> segments;
    for (uint32_t l = 0; l < n; ++l) {
        first_segment[l] = static_cast<uint32_t>(segments.size());
        if (plans[l].on_image) segments.insert(segments.end(), plans[l].segments.begin(), plans[l].segments.end());
    }
    std::vector<uint32_t> entries;   // [n_entries][4] for the kernel
    for (size_t k = 0; k < pairs.size(); ++k) {
        const uint32_t tile = pairs[k].first, l = pairs[k].second;
        if (k == 0 || pairs[k - 1].first != tile) tiles.insert(tiles.end(), {tile, static_cast<uint32_t>(k), 0u, 0u});
        ++tiles[tiles.size() - 2];
        entries.insert(entries.end(), {tile, l, first_segment[l], static_cast<uint32_t>(plans[l].segments.size())});
        entry_labels.push_back(l);
        b->entries_.insert(b->entries_.end(), {tile, l});
    }
    b->n_tiles_ = static_cast<uint32_t>(tiles.size() / 4);
    if (device_id >= 0 && !pairs.empty()) {
        PVQ_HIP(hipSetDevice(device_id));
        std::vector<uint32_t> boxes(static_cast<size_t>(n) * 4, 0u);
        std::vector<float> colors(static_cast<size_t>(n) * 4, 0.0f);
        for (uint32_t l = 0; l < n; ++l) {
            const TextLabelPlan& p = plans[l];
            const uint32_t box[4] = {p.x0, p.y0, p.x1, p.y1};
            std::copy(box, box + 4, boxes.begin() + 4 * l);
            std::copy(p.linear_rgb, p.linear_rgb + 3, colors.begin() + 4 * l);
        }
        DeviceBuffer d_segments, d_entries, d_boxes;   // needed by text_coverage only
        if (pvq_status s = d_segments.upload(segments.data(), segments.size() * sizeof(text::Segment))) return s;
        if (pvq_status s = d_entries.upload(entries.data(), entries.size() * sizeof(uint32_t))) return s;
        if (pvq_status s = d_boxes.upload(boxes.data(), boxes.size() * sizeof(uint32_t))) return s;
        if (pvq_status s = b->colors_.upload(colors.data(), colors.size() * sizeof(float))) return s;
        if (pvq_status s = b->tiles_.upload(tiles.data(), tiles.size() * sizeof(uint32_t))) return s;
        if (pvq_status s = b->entry_labels_.upload(entry_labels.data(), entry_labels.size() * sizeof(uint32_t))) return s;
        if (pvq_status s = b->layer_.reserve(pairs.size() * TILE_PIXELS * sizeof(float))) return s;
        CoverageArgs a{};
        a.segments = d_segments.as<float4>();
        a.entries = d_entries.as<uint4>();
        a.boxes = d_boxes.as<uint4>();
        a.layer = b->layer_.as<float>();
        a.W = width;
        hipLaunchKernelGGL(text_coverage, dim3(static_cast<unsigned>(pairs.size())), dim3(256), 0, nullptr, a);
        PVQ_HIP(hipGetLastError());
        PVQ_HIP(hipDeviceSynchronize());   // the layer is ready for any stream, and the kernel's inputs may go
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status TextBatch::rows_device(size_t n_rows, float* d_image, hipStream_t stream) {
    if (!d_image) {
        set_last_error("text batch: d_image_inout is needed");
        return PVQ_ERR_INVALID_ARG;
    }
    if (reinterpret_cast<uintptr_t>(d_image) & 15) {
        set_last_error("text batch: d_image_inout must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("text batch", n_rows, 1, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched text stage runs on a GPU; this handle has none (pvq_text_frame is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_rows == 0 || n_tiles_ == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    BlendArgs a{};
    a.image = d_image;
    a.layer = layer_.as<float>();
    a.tiles = tiles_.as<uint4>();
    a.entry_labels = entry_labels_.as<uint32_t>();
    a.colors = colors_.as<float4>();
    a.W = width_;
    a.H = height_;
    a.rows = static_cast<uint32_t>(n_rows);
    hipLaunchKernelGGL(text_blend, dim3(n_tiles_, static_cast<unsigned>(std::min<size_t>(n_rows, 65535))), dim3(256), 0, stream, a);
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status TextBatch::get_coverage(int label, float* out) {
    if (!out || label < -1 || label >= static_cast<int>(n_labels_)) {
        set_last_error("text batch: label is -1 or 0 .. n - 1, and out is needed");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched text stage runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    std::fill_n(out, static_cast<size_t>(width_) * height_, 0.0f);
    const size_t n_entries = entries_.size() / 2;
    if (n_entries == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    std::vector<float> layer(n_entries * TILE_PIXELS);
    PVQ_HIP(hipMemcpy(layer.data(), layer_.as<float>(), layer.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n_entries; ++e) {
        if (label >= 0 && entries_[2 * e + 1] != static_cast<uint32_t>(label)) continue;
        for (uint32_t tid = 0; tid < TILE_PIXELS; ++tid) {
            uint32_t i, j;
            pixel_of(entries_[2 * e], tid, width_, i, j);
            if (i >= width_ || j >= height_) continue;
            float& o = out[static_cast<size_t>(j) * width_ + i];
            o = std::max(o, layer[e * TILE_PIXELS + tid]);
        }
    }
    return PVQ_OK;
}

}  // namespace pvq
