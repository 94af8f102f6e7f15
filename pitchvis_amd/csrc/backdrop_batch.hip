// backdrop_batch.hip — the picture behind the pitch balls for many streams (backdrop_batch.hpp).
//
// backdrop_lists (frame-parallel, a workgroup per (stream, frame) row): the row's dynamic triangles — spectrum line, peak discs,
// graph, histogram, lit bass segments, in draw order — become finished backdrop::Tri records in the workspace: a lane places its
// triangle's vertices, builds the canonical edge data, converts the colour and computes the pixel box; a triangle that draws
// nothing on this image is dropped, and a prefix count over the workgroup (a ballot per wave, the waves' sums through LDS) keeps
// the order.  The static net's records are built once at create, on the host, and shared by all rows.
// backdrop_tiles (frame-parallel, the raster stage's tile shape: a workgroup per (row, 16 x 16 pixels), a wave per 8 x 8 block, a
// lane per pixel): per 64 records each lane loads one record's box word (16 bytes, a record apart; four such loads in flight) and
// tests it against the wave's block; a ballot gives the hit mask, the wave visits the set bits in ascending order — the list's
// order — reading the record at a wave-uniform address, and every lane evaluates the rule for its pixel and blends.  The colour
// stays in four registers and leaves in one 16-byte store.  The kernels' argument block and the walk over a list are
// backdrop_device.hpp's, shared with the four-sample tile kernel of backdrop_msaa.hip, which frames_device launches in this
// kernel's place for a handle made with samples = 4.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#include "backdrop_batch.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "backdrop_device.hpp"
#include "stage_device.hpp"
#include "stage_plan.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
constexpr uint32_t MAX_BINS = 1024;
constexpr size_t WORKSPACE_LIMIT = 256ull << 20;   // the lists of one piece of a call
constexpr int LIST_THREADS = 256;
constexpr int TILE = stage::TILE;
constexpr uint32_t WORDS = BACKDROP_WORDS;

__global__ __launch_bounds__(LIST_THREADS) __attribute__((flatten)) void backdrop_lists(BackdropArgs a) {
#pragma clang fp contract(off)
    __shared__ uint32_t s_wave[LIST_THREADS / 64];
    __shared__ uint32_t s_base;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        if (tid == 0) s_base = 0u;
        __syncthreads();
        // the row's layers, in draw order: [0, e_line) line, [.., e_disc) discs, [.., e_graph) graph, [.., e_hist) histogram, bass
        const uint32_t e_line = a.line_pos ? 2u * a.line_quads : 0u;
        const uint32_t e_disc = e_line + (a.disc_pos ? panels::DISC_SEGMENTS * min(a.peak_count[g], a.max_peaks) : 0u);
        const uint32_t e_graph = e_disc + (a.graph_pos ? 2u * a.graph_quads : 0u);
        const uint32_t e_hist = e_graph + (a.hist_pos ? 2u * a.line_quads : 0u);
        const uint32_t total = e_hist + (a.bass_lit ? 2u * min(a.bass_lit[g], a.n_bass) : 0u);   // <= cap
        uint4* out = a.list + static_cast<size_t>(r) * a.cap * WORDS;
        for (uint32_t t0 = 0; t0 < total; t0 += LIST_THREADS) {   // (total is the workgroup's: every wave meets every barrier)
            const uint32_t t = t0 + tid;
            bool keep = false;
            backdrop::Tri q;
            if (t < total) {
                float v[6], rgba[4];
                uint32_t va, vb, vc, base;
                if (t >= e_hist) {
                    backdrop::quad_triangle(t - e_hist, va, vb, vc, base);   // vertex numbers < 4 n_bass
                    v[0] = a.bass_quads[2u * va]; v[1] = a.bass_quads[2u * va + 1u];
                    v[2] = a.bass_quads[2u * vb]; v[3] = a.bass_quads[2u * vb + 1u];
                    v[4] = a.bass_quads[2u * vc]; v[5] = a.bass_quads[2u * vc + 1u];
                    const float4 c = reinterpret_cast<const float4*>(a.bass_rgba)[g];
                    const float srgba[4] = {c.x, c.y, c.z, c.w};
                    backdrop::bass_color(srgba, rgba);
                } else {
                    const bool is_line = t < e_line, is_disc = !is_line && t < e_disc, is_graph = !is_line && !is_disc && t < e_graph;
                    const float* pos;
                    const float* col;
                    size_t row_vertices;
                    if (is_disc) {
                        backdrop::disc_triangle(t - e_line, va, vb, vc, base);   // disc < min(count, max_peaks)
                        pos = a.disc_pos;
                        col = a.disc_rgba;
                        row_vertices = static_cast<size_t>(panels::DISC_VERTICES) * a.max_peaks;
                    } else {
                        backdrop::quad_triangle(is_line ? t : (is_graph ? t - e_disc : t - e_graph), va, vb, vc, base);
                        pos = is_line ? a.line_pos : (is_graph ? a.graph_pos : a.hist_pos);
                        col = is_line ? a.line_rgba : (is_graph ? a.graph_rgba : a.hist_rgba);
                        row_vertices = 4u * static_cast<size_t>(is_graph ? a.graph_quads : a.line_quads);
                    }
                    const bool spec = is_line || is_disc;
                    const float tr[4] = {spec ? a.t_spec[0] : (is_graph ? a.t_graph[0] : a.t_hist[0]),
                                         spec ? a.t_spec[1] : (is_graph ? a.t_graph[1] : a.t_hist[1]),
                                         spec ? a.t_spec[2] : (is_graph ? a.t_graph[2] : a.t_hist[2]),
                                         spec ? a.t_spec[3] : (is_graph ? a.t_graph[3] : a.t_hist[3])};
                    const float* p = pos + g * row_vertices * 3u;
                    backdrop::place(tr, p[3u * va], p[3u * va + 1u], v[0], v[1]);
                    backdrop::place(tr, p[3u * vb], p[3u * vb + 1u], v[2], v[3]);
                    backdrop::place(tr, p[3u * vc], p[3u * vc + 1u], v[4], v[5]);
                    const float4 c = reinterpret_cast<const float4*>(col)[g * row_vertices + base];
                    rgba[0] = c.x; rgba[1] = c.y; rgba[2] = c.z; rgba[3] = c.w;
                }
                keep = backdrop::make_tri(v, rgba, a.W, a.H, a.vh, q);
            }
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__popcll(mask));
            __syncthreads();
            uint32_t at = s_base + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
            for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
            if (keep) {   // at < total <= cap
                uint4* dst = out + static_cast<size_t>(at) * WORDS;
                dst[0] = make_uint4(q.box_x, q.box_y, q.positive, 0u);
                dst[1] = make_uint4(__float_as_uint(q.edge[0][0]), __float_as_uint(q.edge[0][1]), __float_as_uint(q.edge[0][2]), __float_as_uint(q.edge[0][3]));
                dst[2] = make_uint4(__float_as_uint(q.edge[1][0]), __float_as_uint(q.edge[1][1]), __float_as_uint(q.edge[1][2]), __float_as_uint(q.edge[1][3]));
                dst[3] = make_uint4(__float_as_uint(q.edge[2][0]), __float_as_uint(q.edge[2][1]), __float_as_uint(q.edge[2][2]), __float_as_uint(q.edge[2][3]));
                dst[4] = make_uint4(__float_as_uint(q.rgba[0]), __float_as_uint(q.rgba[1]), __float_as_uint(q.rgba[2]), __float_as_uint(q.rgba[3]));
            }
            __syncthreads();   // s_base and s_wave have been read
            if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            __syncthreads();
        }
        if (tid == 0) a.counts[r] = s_base;
        __syncthreads();   // s_base is the next row's
    }
}

__global__ __launch_bounds__(256) __attribute__((flatten)) void backdrop_tiles(BackdropArgs a) {
#pragma clang fp contract(off)
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const stage::TilePixel px = stage::tile_pixel(wave, lane, a.W, a.H, a.vh);
    const float wx[1] = {px.wx}, wy[1] = {px.wy};   // one sample, at the centre
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        float dst[4] = {a.clear[0], a.clear[1], a.clear[2], a.clear[3]};
        if (a.background && px.inside) {
            const float4 bg = reinterpret_cast<const float4*>(a.background)[px.pixel];
            dst[0] = bg.x; dst[1] = bg.y; dst[2] = bg.z; dst[3] = bg.w;
        }
        backdrop::walk<1>(a.net, a.n_net, lane, px.bx0, px.by0, wx, wy, dst);
        backdrop::walk<1>(a.list + static_cast<size_t>(r) * a.cap * WORDS, a.counts[r], lane, px.bx0, px.by0, wx, wy, dst);
        if (px.inside) reinterpret_cast<float4*>(a.image)[g * a.W * a.H + px.pixel] = make_float4(dst[0], dst[1], dst[2], dst[3]);
    }
}
}  // namespace

pvq_status BackdropBatch::create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                                 uint32_t n_streams, uint32_t width, uint32_t height, std::unique_ptr<BackdropBatch>& out, uint32_t samples) {
    out.reset();
    if (!backdrop::samples_ok(samples)) {
        set_last_error("backdrop batch: samples is 1 or 4");
        return PVQ_ERR_INVALID_ARG;
    }
    if (octaves == 0 || buckets_per_octave == 0 || n_streams == 0) {
        set_last_error("backdrop batch: octaves, buckets_per_octave and n_streams must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_mode_ok("backdrop batch", visuals_mode, err) || !stage_image_ok("backdrop batch", width, height, viewport_height, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (n < 3 || n > MAX_BINS) {
        set_last_error("unsupported: the batched backdrop takes 3 .. 1024 bins");
        return PVQ_ERR_UNSUPPORTED;
    }
    if (static_cast<uint64_t>(n_streams) * n > 0x7FFFFFFFull) {
        set_last_error("backdrop batch: too many streams");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<BackdropBatch> b(new BackdropBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_streams_ = n_streams;
    b->n_bins_ = static_cast<uint32_t>(n);
    b->width_ = width;
    b->height_ = height;
    b->vh_ = viewport_height == 0.0f ? raster::VIEWPORT_HEIGHT : viewport_height;
    b->galaxy_ = visuals_mode == scene::GALAXY;
    b->samples_ = samples;
    raster::clear_color(visuals_mode, b->clear_);
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        if (!b->galaxy_) {   // update.rs:888-895: no net and no bass spiral in Galaxy mode
            std::vector<backdrop::Tri> net;
            float gray[4];
            backdrop::net_color(gray);
            for (int what : {backdrop::NET_SPIRAL, backdrop::NET_RAYS}) {
                const std::vector<float> quads = backdrop_geometry(octaves, what);
                for (uint32_t t = 0; t < 2u * backdrop::geometry_count(octaves, what); ++t) {
                    uint32_t va, vb, vc, base;
                    backdrop::quad_triangle(t, va, vb, vc, base);
                    const float v[6] = {quads[2 * va], quads[2 * va + 1], quads[2 * vb], quads[2 * vb + 1], quads[2 * vc], quads[2 * vc + 1]};
                    backdrop::Tri q;
                    if (backdrop::make_tri(v, gray, width, height, b->vh_, q)) net.push_back(q);
                }
            }
            b->n_net_ = static_cast<uint32_t>(net.size());
            if (b->n_net_)
                if (pvq_status s = b->net_.upload(net.data(), net.size() * sizeof(backdrop::Tri))) return s;
            const std::vector<float> bass = backdrop_geometry(octaves, backdrop::BASS);
            b->n_bass_ = backdrop::geometry_count(octaves, backdrop::BASS);
            if (pvq_status s = b->bass_.upload(bass.data(), bass.size() * sizeof(float))) return s;
        }
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status BackdropBatch::frames_device(size_t n_frames, const pvq_backdrop_inputs& in, float* d_image, hipStream_t stream) {
    if (!d_image) {
        set_last_error("backdrop batch: d_image is needed");
        return PVQ_ERR_INVALID_ARG;
    }
    if (!in.line_pos != !in.line_rgba || !in.hist_pos != !in.hist_rgba || !in.graph_pos != !in.graph_rgba || !in.disc_pos != !in.disc_rgba ||
        !in.bass_lit != !in.bass_rgba) {
        set_last_error("backdrop batch: a mesh needs its positions and its colours, bass_lit needs bass_rgba");
        return PVQ_ERR_INVALID_ARG;
    }
    if (in.disc_pos && (!in.peak_count || in.max_peaks == 0)) {
        set_last_error("backdrop batch: the discs need peak_count and max_peaks > 0");
        return PVQ_ERR_INVALID_ARG;
    }
    if (in.graph_pos && (in.graph_capacity < 2 || in.graph_capacity > 1024)) {
        set_last_error("backdrop batch: the graph needs its graph_capacity, 2 .. 1024");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(in.bass_rgba) | reinterpret_cast<uintptr_t>(in.line_rgba) | reinterpret_cast<uintptr_t>(in.disc_rgba) |
         reinterpret_cast<uintptr_t>(in.hist_rgba) | reinterpret_cast<uintptr_t>(in.graph_rgba) | reinterpret_cast<uintptr_t>(in.background) |
         reinterpret_cast<uintptr_t>(d_image)) & 15) {
        set_last_error("backdrop batch: the rgba arrays, bass_rgba, background and d_image must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(in.bass_lit) | reinterpret_cast<uintptr_t>(in.line_pos) | reinterpret_cast<uintptr_t>(in.disc_pos) |
         reinterpret_cast<uintptr_t>(in.hist_pos) | reinterpret_cast<uintptr_t>(in.graph_pos) | reinterpret_cast<uintptr_t>(in.peak_count)) & 3) {
        set_last_error("backdrop batch: the position and count arrays must be 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if (in.max_peaks > 0x00FFFFFFu) {
        set_last_error("backdrop batch: max_peaks is too large");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("backdrop batch", n_frames, n_streams_, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched backdrop runs on a GPU; this handle has none (pvq_backdrop_frame is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_frames == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));

    BackdropArgs a{};
    a.bass_lit = n_bass_ ? in.bass_lit : nullptr;
    a.bass_rgba = in.bass_rgba;
    a.line_pos = in.line_pos; a.line_rgba = in.line_rgba;
    a.disc_pos = in.disc_pos; a.disc_rgba = in.disc_rgba;
    a.hist_pos = in.hist_pos; a.hist_rgba = in.hist_rgba;
    a.graph_pos = in.graph_pos; a.graph_rgba = in.graph_rgba;
    a.peak_count = in.peak_count;
    a.max_peaks = in.max_peaks;
    a.line_quads = n_bins_ - 1u;
    a.graph_quads = in.graph_pos ? in.graph_capacity - 1u : 0u;
    for (int i = 0; i < 4; ++i) {
        a.t_spec[i] = in.spectrum_transform[i];
        a.t_hist[i] = in.histogram_transform[i];
        a.t_graph[i] = in.graph_transform[i];
        a.clear[i] = clear_[i];
    }
    a.background = in.background;
    a.bass_quads = bass_.as<float>();
    a.net = net_.as<uint4>();
    a.n_bass = n_bass_;
    a.n_net = n_net_;
    a.n_streams = n_streams_;
    a.n_frames = static_cast<uint32_t>(n_frames);
    a.W = width_;
    a.H = height_;
    a.vh = vh_;
    a.image = d_image;
    // the most records a row can have: backdrop_lists' `total` with every count at its maximum
    const uint64_t cap = (in.line_pos ? 2ull * a.line_quads : 0ull) + (in.disc_pos ? static_cast<uint64_t>(panels::DISC_SEGMENTS) * in.max_peaks : 0ull) +
                         2ull * a.graph_quads + (in.hist_pos ? 2ull * a.line_quads : 0ull) + (a.bass_lit ? 2ull * n_bass_ : 0ull);
    a.cap = static_cast<uint32_t>(cap);   // < 2^32: max_peaks < 2^24

    // the lists of a piece of the call's frames fit the workspace
    const size_t per_row = static_cast<size_t>(cap) * sizeof(backdrop::Tri) + sizeof(uint32_t);
    const size_t limit = static_cast<size_t>(std::max(1, dev_knob("PVQ_BACKDROP_WS_KB", static_cast<int>(WORKSPACE_LIMIT >> 10)))) << 10;
    const size_t pf = stage_piece_frames(n_frames, n_streams_, per_row, limit);
    const size_t rows_max = static_cast<size_t>(n_streams_) * pf;
    if (pvq_status s = ws_.reserve(per_row * rows_max)) return s;
    a.list = ws_.as<uint4>();   // the 80-byte records first: the workspace is 256-byte aligned
    a.counts = reinterpret_cast<uint32_t*>(a.list + rows_max * cap * WORDS);
    const uint32_t tiles = ((width_ + TILE - 1) / TILE) * ((height_ + TILE - 1) / TILE);
    for (size_t f0 = 0; f0 < n_frames; f0 += pf) {
        a.f0 = static_cast<uint32_t>(f0);
        a.pf = static_cast<uint32_t>(std::min(pf, n_frames - f0));
        const size_t rows_here = static_cast<size_t>(n_streams_) * a.pf;
        hipLaunchKernelGGL(backdrop_lists, dim3(static_cast<unsigned>(std::min<size_t>(rows_here, 256 * 32))), dim3(LIST_THREADS), 0, stream, a);
        const dim3 grid(tiles, static_cast<unsigned>(std::min<size_t>(rows_here, 65535)));
        if (samples_ == 4u) launch_backdrop_tiles_msaa(a, grid, stream);
        else hipLaunchKernelGGL(backdrop_tiles, grid, dim3(256), 0, stream, a);
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

}  // namespace pvq
