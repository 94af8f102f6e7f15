// raster_batch.hip — the pitch balls as pixels for many streams (raster_batch.hpp), split by what recurs.
//
// raster_marks (frame-parallel, a wavefront per (stream, frame) row): the row's peak list ORs the key bins into a bin mask.
// raster_times (a lane per (stream, bin), frames in order): the only recurrence — a marked bin takes the frame's clock, the others
// carry theirs; the per-frame times go to the workspace (and to d_ball_time), the last one back to the handle.
// raster_lists (frame-parallel, a workgroup per row): the drawable balls whose pixel box meets the image are keyed by (z, bin) into
// LDS, each entry is ranked against all others — keys are distinct, so the ranks are the sorted positions; 1024 entries are
// 1024 x 1024 / 256 broadcast LDS reads a lane, and a row seldom has a tenth of that — and its finished raster::Ball (the two
// pulses, the cube, the star's brightness: all the per-ball libm) lands at its rank in the workspace.
// raster_tiles (frame-parallel, a workgroup per (row, 16 x 16 pixels), a wave per 8 x 8 block, a lane per pixel): the row's list
// goes through LDS in chunks of 64 balls (one 16-byte load a lane); the box-against-block test reads LDS at a wave-uniform address
// and branches the whole wave; the pixel's colour stays in registers across all balls and leaves in one 16-byte store.  The
// colour starts as the clear colour, the shared background, or — drawing over a backdrop — what the image holds for that row.
//
// FMA contraction is off and `/` and sqrt are the correctly rounded ones, as in scene_batch.hip.
#include "raster_batch.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "stage_device.hpp"
#include "stage_plan.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
constexpr uint32_t MAX_BINS = 1024;
constexpr size_t WORKSPACE_LIMIT = 256ull << 20;   // the lists of one piece of a call
constexpr int LIST_THREADS = 256;
constexpr int CHUNK = 64;                           // balls staged through LDS at a time: 64 x 64 bytes, 16 bytes a lane of 256
constexpr int TILE = stage::TILE;

struct RasterArgs {
    const float* xyzs;          // [n_streams][n_frames][n_bins][4]
    const float* rgba;
    const float* params;        // [..][n_bins][3]
    const uint32_t* visible;    // [..][words]
    const float* center;        // [..][max_peaks]
    const uint32_t* peak_count;
    const float* background;    // [H][W][4] or null
    size_t bg_row;              // pixels from a row's background to the next row's: 0, one picture shared by all rows
    const float* elapsed;       // [n_frames]
    uint32_t max_peaks, n_streams, n_bins, words;
    uint32_t n_frames, f0, pf;  // the call's frames; this piece is frames f0 .. f0 + pf
    uint32_t W, H;
    float vh;
    float clear[4];
    float* state;               // [n_streams][n_bins]
    raster::Ball* list;         // [n_streams * pf][n_bins]
    float* times;               // [n_streams * pf][n_bins]
    uint32_t* marks;            // [n_streams * pf][words]
    uint32_t* counts;           // [n_streams * pf]
    float* out_time;            // [n_streams][n_frames][n_bins] or null
    float* image;               // [n_streams][n_frames][H][W][4]
};

__global__ __launch_bounds__(64) void raster_marks(RasterArgs a) {
    __shared__ uint32_t s_mask[MAX_BINS / 32];
    const int lane = threadIdx.x;
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        if (lane < static_cast<int>(MAX_BINS / 32)) s_mask[lane] = 0u;
        __syncthreads();
        const uint32_t cnt = min(a.peak_count[g], a.max_peaks);
        const float* c_row = a.center + g * a.max_peaks;
        for (uint32_t p = lane; p < cnt; p += 64) {
            const uint32_t key = scene::sat_u32(truncf(c_row[p]));   // as scene::peak_record takes it
            if (key < a.n_bins) atomicOr(&s_mask[key >> 5], 1u << (key & 31u));
        }
        __syncthreads();
        if (lane < static_cast<int>(a.words)) a.marks[static_cast<size_t>(r) * a.words + lane] = s_mask[lane];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void raster_times(RasterArgs a) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.n_streams * a.n_bins) return;
    const uint32_t s = idx / a.n_bins, bin = idx - s * a.n_bins;
    float t = a.state[idx];
    for (uint32_t fi = 0; fi < a.pf; ++fi) {
        const size_t r = static_cast<size_t>(s) * a.pf + fi;
        if ((a.marks[r * a.words + (bin >> 5)] >> (bin & 31u)) & 1u) t = a.elapsed[a.f0 + fi];
        a.times[r * a.n_bins + bin] = t;
        if (a.out_time) a.out_time[(static_cast<size_t>(s) * a.n_frames + a.f0 + fi) * a.n_bins + bin] = t;
    }
    a.state[idx] = t;
}

// the row's inputs of one bin; false: not drawn
__device__ __forceinline__ bool load_ball(const RasterArgs& a, size_t g, size_t r, uint32_t bin, float xyzs[4], float rgba[4], float params[3],
                                          float& time) {
    const float4 q0 = reinterpret_cast<const float4*>(a.xyzs)[g * a.n_bins + bin];
    const float4 q1 = reinterpret_cast<const float4*>(a.rgba)[g * a.n_bins + bin];
    const float* pp = a.params + (g * a.n_bins + bin) * 3;
    xyzs[0] = q0.x; xyzs[1] = q0.y; xyzs[2] = q0.z; xyzs[3] = q0.w;
    rgba[0] = q1.x; rgba[1] = q1.y; rgba[2] = q1.z; rgba[3] = q1.w;
    params[0] = pp[0]; params[1] = pp[1]; params[2] = pp[2];
    time = a.times[r * a.n_bins + bin];
    const bool vis = (a.visible[g * a.words + (bin >> 5)] >> (bin & 31u)) & 1u;
    return raster::drawable(xyzs, rgba, params, time, vis);
}

__global__ __launch_bounds__(LIST_THREADS) __attribute__((flatten)) void raster_lists(RasterArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_key[MAX_BINS];
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x;
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        if (tid == 0) s_n = 0u;
        __syncthreads();
        for (uint32_t bin = tid; bin < a.n_bins; bin += LIST_THREADS) {
            float xyzs[4], rgba[4], params[3], time;
            uint32_t bx, by;
            if (load_ball(a, g, r, bin, xyzs, rgba, params, time) &&
                raster::pixel_box(xyzs[0], xyzs[1], raster::BALL_SIDE * xyzs[3], a.W, a.H, a.vh, bx, by))
                s_key[atomicAdd(&s_n, 1u)] = raster::order_key(xyzs[2], bin);   // (at most n_bins <= 1024 entries)
        }
        __syncthreads();
        const uint32_t m = s_n;
        for (uint32_t e = tid; e < m; e += LIST_THREADS) {
            const unsigned long long key = s_key[e];
            uint32_t rank = 0u;
            for (uint32_t i = 0; i < m; ++i) rank += s_key[i] < key ? 1u : 0u;   // (the same address on every lane: a broadcast)
            const uint32_t bin = static_cast<uint32_t>(key & 0xFFFFFFFFull);
            float xyzs[4], rgba[4], params[3], time;
            (void)load_ball(a, g, r, bin, xyzs, rgba, params, time);
            raster::Ball q;
            raster::make_ball(xyzs, rgba, params, time, q);
            (void)raster::pixel_box(q.x, q.y, q.side, a.W, a.H, a.vh, q.box_x, q.box_y);
            uint4* dst = reinterpret_cast<uint4*>(a.list + static_cast<size_t>(r) * a.n_bins + rank);   // rank < m <= n_bins
            dst[0] = make_uint4(__float_as_uint(q.x), __float_as_uint(q.y), __float_as_uint(q.side), __float_as_uint(q.noise_z));
            dst[1] = make_uint4(__float_as_uint(q.r), __float_as_uint(q.g), __float_as_uint(q.b), __float_as_uint(q.a));
            dst[2] = make_uint4(__float_as_uint(q.calmness), __float_as_uint(q.ring_strength), __float_as_uint(q.dot_factor),
                                __float_as_uint(q.dot_pulse));
            dst[3] = make_uint4(__float_as_uint(q.spiral), __float_as_uint(q.star_brightness), q.box_x, q.box_y);
        }
        if (tid == 0) a.counts[r] = m;
        __syncthreads();   // s_key / s_n are the next row's
    }
}

__global__ __launch_bounds__(256) __attribute__((flatten)) void raster_tiles(RasterArgs a) {
#pragma clang fp contract(off)
    __shared__ uint4 s_ball[CHUNK * 4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const stage::TilePixel px = stage::tile_pixel(wave, lane, a.W, a.H, a.vh);
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        float dst[4] = {a.clear[0], a.clear[1], a.clear[2], a.clear[3]};
        if (a.background && px.inside) {
            const float4 bg = reinterpret_cast<const float4*>(a.background)[g * a.bg_row + px.pixel];
            dst[0] = bg.x; dst[1] = bg.y; dst[2] = bg.z; dst[3] = bg.w;
        }
        const uint32_t m = a.counts[r];
        const uint4* list = reinterpret_cast<const uint4*>(a.list + static_cast<size_t>(r) * a.n_bins);
        for (uint32_t c0 = 0; c0 < m; c0 += CHUNK) {   // (m is the workgroup's: every wave meets every barrier)
            const uint32_t here = min(static_cast<uint32_t>(CHUNK), m - c0);
            __syncthreads();   // the chunk before has been read
            if (tid < here * 4u) s_ball[tid] = list[static_cast<size_t>(c0) * 4 + tid];
            __syncthreads();
            for (uint32_t k = 0; k < here; ++k) {
                const uint4 q3 = s_ball[k * 4 + 3];   // wave-uniform address
                const uint32_t bx = __builtin_amdgcn_readfirstlane(q3.z), by = __builtin_amdgcn_readfirstlane(q3.w);
                if ((bx & 0xFFFFu) > px.bx0 + 7u || (bx >> 16) < px.bx0 || (by & 0xFFFFu) > px.by0 + 7u || (by >> 16) < px.by0) continue;
                const uint4 q0 = s_ball[k * 4], q1 = s_ball[k * 4 + 1], q2 = s_ball[k * 4 + 2];
                raster::Ball q;
                q.x = __uint_as_float(q0.x); q.y = __uint_as_float(q0.y); q.side = __uint_as_float(q0.z); q.noise_z = __uint_as_float(q0.w);
                q.r = __uint_as_float(q1.x); q.g = __uint_as_float(q1.y); q.b = __uint_as_float(q1.z); q.a = __uint_as_float(q1.w);
                q.calmness = __uint_as_float(q2.x); q.ring_strength = __uint_as_float(q2.y);
                q.dot_factor = __uint_as_float(q2.z); q.dot_pulse = __uint_as_float(q2.w);
                q.spiral = __uint_as_float(q3.x); q.star_brightness = __uint_as_float(q3.y);
                q.box_x = bx; q.box_y = by;
                raster::compose_ball(q, px.wx, px.wy, dst);
            }
        }
        if (px.inside) reinterpret_cast<float4*>(a.image)[g * a.W * a.H + px.pixel] = make_float4(dst[0], dst[1], dst[2], dst[3]);
    }
}
}  // namespace

pvq_status RasterBatch::create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, int visuals_mode, float viewport_height,
                               uint32_t n_streams, uint32_t width, uint32_t height, std::unique_ptr<RasterBatch>& out) {
    out.reset();
    if (octaves == 0 || buckets_per_octave == 0 || n_streams == 0) {
        set_last_error("raster batch: octaves, buckets_per_octave and n_streams must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_mode_ok("raster batch", visuals_mode, err) || !stage_image_ok("raster batch", width, height, viewport_height, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (n < 3 || n > MAX_BINS) {
        set_last_error("unsupported: the batched raster takes 3 .. 1024 bins");
        return PVQ_ERR_UNSUPPORTED;
    }
    if (static_cast<uint64_t>(n_streams) * n > 0x7FFFFFFFull) {
        set_last_error("raster batch: too many streams");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<RasterBatch> b(new RasterBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_streams_ = n_streams;
    b->n_bins_ = static_cast<uint32_t>(n);
    b->width_ = width;
    b->height_ = height;
    b->vh_ = viewport_height == 0.0f ? raster::VIEWPORT_HEIGHT : viewport_height;
    raster::clear_color(visuals_mode, b->clear_);
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        const size_t bytes = static_cast<size_t>(n_streams) * n * sizeof(float);
        if (pvq_status s = b->time_.reserve(bytes)) return s;
        PVQ_HIP(hipMemset(b->time_.as<float>(), 0, bytes));   // Params::default()
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status RasterBatch::frames_device(size_t n_frames, const pvq_raster_inputs& in, const float* elapsed_s, float* d_image,
                                      float* d_ball_time, hipStream_t stream, bool over) {
    if (over && (in.background || !d_image)) {
        set_last_error("raster batch: drawing over the image takes no background and needs d_image");
        return PVQ_ERR_INVALID_ARG;
    }
    if (!in.center || !in.peak_count || in.max_peaks == 0) {
        set_last_error("raster batch: center and peak_count are needed, with max_peaks > 0");
        return PVQ_ERR_INVALID_ARG;
    }
    if (d_image && (!in.ball_xyzs || !in.ball_rgba || !in.ball_params || !in.ball_visible)) {
        set_last_error("raster batch: an image needs ball_xyzs, ball_rgba, ball_params and ball_visible");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(in.ball_xyzs) | reinterpret_cast<uintptr_t>(in.ball_rgba) | reinterpret_cast<uintptr_t>(in.background) |
         reinterpret_cast<uintptr_t>(d_image)) & 15) {
        set_last_error("raster batch: ball_xyzs, ball_rgba, background and d_image must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("raster batch", n_frames, n_streams_, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_frames && !elapsed_s) {
        set_last_error("raster batch: elapsed_s is needed, one clock value per frame");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched raster runs on a GPU; this handle has none (pvq_raster_frame is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_frames == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    const uint32_t n = n_bins_, words = (n + 31u) / 32u;

    if (pvq_status s = elapsed_.reserve(n_frames * sizeof(float))) return s;
    // stream-ordered behind the call before, which may still read the buffer; the host array is the caller's again on return
    PVQ_HIP(hipMemcpyAsync(elapsed_.as<float>(), elapsed_s, n_frames * sizeof(float), hipMemcpyHostToDevice, stream));
    PVQ_HIP(hipStreamSynchronize(stream));

    // the lists of a piece of the call's frames fit the workspace
    const size_t per_row = static_cast<size_t>(n) * (sizeof(raster::Ball) + sizeof(float)) + (words + 1u) * sizeof(uint32_t);
    const size_t limit = static_cast<size_t>(std::max(1, dev_knob("PVQ_RASTER_WS_KB", static_cast<int>(WORKSPACE_LIMIT >> 10)))) << 10;
    const size_t pf = stage_piece_frames(n_frames, n_streams_, per_row, limit);
    const size_t rows_max = static_cast<size_t>(n_streams_) * pf;
    if (pvq_status s = ws_.reserve(per_row * rows_max)) return s;
    RasterArgs a{};
    a.xyzs = in.ball_xyzs;
    a.rgba = in.ball_rgba;
    a.params = in.ball_params;
    a.visible = in.ball_visible;
    a.center = in.center;
    a.peak_count = in.peak_count;
    a.background = over ? d_image : in.background;   // in place: a lane reads its pixel before it writes it
    a.bg_row = over ? static_cast<size_t>(width_) * height_ : 0;
    a.elapsed = elapsed_.as<float>();
    a.max_peaks = in.max_peaks;
    a.n_streams = n_streams_;
    a.n_bins = n;
    a.words = words;
    a.n_frames = static_cast<uint32_t>(n_frames);
    a.W = width_;
    a.H = height_;
    a.vh = vh_;
    for (int i = 0; i < 4; ++i) a.clear[i] = clear_[i];
    a.state = time_.as<float>();
    a.list = ws_.as<raster::Ball>();   // the 64-byte records first: the workspace is 256-byte aligned
    a.times = reinterpret_cast<float*>(a.list + rows_max * n);
    a.marks = reinterpret_cast<uint32_t*>(a.times + rows_max * n);
    a.counts = a.marks + rows_max * words;
    a.out_time = d_ball_time;
    a.image = d_image;
    const uint32_t tiles = ((width_ + TILE - 1) / TILE) * ((height_ + TILE - 1) / TILE);
    for (size_t f0 = 0; f0 < n_frames; f0 += pf) {
        a.f0 = static_cast<uint32_t>(f0);
        a.pf = static_cast<uint32_t>(std::min(pf, n_frames - f0));
        const size_t rows_here = static_cast<size_t>(n_streams_) * a.pf;
        const unsigned row_grid = static_cast<unsigned>(std::min<size_t>(rows_here, 256 * 32));
        hipLaunchKernelGGL(raster_marks, dim3(row_grid), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(raster_times, dim3((n_streams_ * n + 255u) / 256u), dim3(256), 0, stream, a);
        if (d_image) {
            hipLaunchKernelGGL(raster_lists, dim3(row_grid), dim3(LIST_THREADS), 0, stream, a);
            hipLaunchKernelGGL(raster_tiles, dim3(tiles, static_cast<unsigned>(std::min<size_t>(rows_here, 65535))), dim3(256), 0, stream, a);
        }
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status RasterBatch::get_times(uint32_t stream_index, float* out) {
    if (stream_index >= n_streams_ || !out) {
        set_last_error("raster batch: stream index out of range, or no output");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched raster runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    PVQ_HIP(hipMemcpy(out, time_.as<float>() + static_cast<size_t>(stream_index) * n_bins_, n_bins_ * sizeof(float), hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
