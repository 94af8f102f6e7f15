// panels_batch.hip — the debug panels for many rows, a wavefront per row (panels_batch.hpp).
//
// Every arithmetic step is panels_math.hpp's — the very source the host face (panels_host.cpp) compiles — with FMA contraction off,
// the correctly rounded fp32 division and square root hipcc emits for `/` and sqrtf, and the double-precision sqrt of the segment
// length.  No kernel evaluates any other libm function: the bucket colours and the twelve disc angles come from the host once.
//
// The stage writes far more than it reads (112 bytes per segment against 4 to 8 read), so the kernels are shaped by their stores:
//   * panels_rows<NK>: one 64-lane workgroup walks rows blockIdx.x, + gridDim.x, ...; lane l owns segments l, l + 64, ... of the row
//     (NK of them: an instantiation knows its bin count's 64-chunk).  util::arg_max of the row is a wave reduction over (value, bin).
//     A lane writes its segment's 48 bytes of positions and 64 bytes of colours as whole 16-byte stores; a wave's stores cover one
//     contiguous run.  The histogram goes the same way.  A disc's 156 bytes are only 4-byte aligned, so discs go through LDS: a lane
//     per peak (in chunks of 64, any max_peaks) leaves centre and colour entry there, then the lanes walk the chunk's dwords in
//     order, so the row's disc block goes out as contiguous dwords; slots beyond the row's count are zeros.
//   * panels_graph: a wavefront per emitted (stream, frame); segment i reads entries f + 1 + i and f + 2 + i of [history | the call's
//     values] and is written like a row's segment.
//   * panels_history: entry i of a stream's next history is entry n_frames + i of the same concatenation, into the other buffer.
#include "panels_batch.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "panels_host.hpp"
#include "panels_math.hpp"
#include "stage_plan.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
constexpr uint32_t MAX_BINS = 1024;
constexpr uint32_t MAX_CAPACITY = 1024;
constexpr uint32_t POS_PER_DISC = panels::DISC_VERTICES * 3;    // 39 dwords
constexpr uint32_t RGBA_PER_DISC = panels::DISC_VERTICES * 4;   // 52 dwords

// built by the host at create, read-only afterwards
struct PanelTables {
    float rgb[MAX_BINS * 3];   // panel_color_table: entry k < bpo
    float cs[24];              // panel_disc_table
};

struct RowsArgs {
    const float* x;
    const float* center;
    const float* size;
    const uint32_t* peak_count;
    const float* calmness;
    uint32_t max_peaks, n_rows;
    int n_bins;
    uint32_t bpo;
    const PanelTables* tab;
    float* line_pos;
    float* line_rgba;
    float* disc_pos;
    float* disc_rgba;
    float* hist_pos;
    float* hist_rgba;
};

struct GraphArgs {
    const float* hist;     // [n_streams][capacity]
    const float* vals;     // [n_streams][n_frames]
    float* hist_next;      // [n_streams][capacity]
    uint32_t n_streams, n_frames, first, capacity;
    float* pos;
    float* rgba;
};

// one 16-byte store each: a vector type, which the compiler neither splits nor regroups (as four float members it regrouped a quad's
// 48 bytes into four 12-byte stores, three of them off the 16-byte grid)
typedef float vec4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_quad(float* pos, size_t seg, const float q[12]) {   // 48 bytes, 16-byte aligned
    vec4* o = reinterpret_cast<vec4*>(pos + 12 * seg);
    o[0] = vec4{q[0], q[1], q[2], q[3]};
    o[1] = vec4{q[4], q[5], q[6], q[7]};
    o[2] = vec4{q[8], q[9], q[10], q[11]};
}
__device__ __forceinline__ void store_rgba(float* rgba, size_t seg, float r, float g, float b, float al) {   // four vertices, 64 bytes
    vec4* o = reinterpret_cast<vec4*>(rgba + 16 * seg);
    const vec4 c = {r, g, b, al};
    o[0] = c;
    o[1] = c;
    o[2] = c;
    o[3] = c;
}

template <int NK>   // 64 (NK - 1) < n_bins <= 64 NK (the host's promise: the chunk tests fold away)
__global__ __launch_bounds__(64) void panels_rows(RowsArgs a) {
#pragma clang fp contract(off)
    constexpr int NB = 64 * NK;
    __builtin_assume(a.n_bins > 64 * (NK - 1) && a.n_bins <= NB);
    __shared__ float s_rgb[3 * NB];   // the colour of every bin's bucket: entry bin % bpo of the table (bpo <= n_bins: also the table itself)
    __shared__ float s_cs[24];
    __shared__ float s_cx[64], s_cy[64];
    __shared__ uint32_t s_at[64];

    const int lane = threadIdx.x;
    const int n = a.n_bins;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int bin = lane + 64 * k;
        if (bin < n) {
            const uint32_t e = static_cast<uint32_t>(bin) % a.bpo;
            s_rgb[3 * bin] = a.tab->rgb[3 * e];
            s_rgb[3 * bin + 1] = a.tab->rgb[3 * e + 1];
            s_rgb[3 * bin + 2] = a.tab->rgb[3 * e + 2];
        }
    }
    if (lane < 24) s_cs[lane] = a.tab->cs[lane];
    __syncthreads();

    const bool do_line = a.line_pos || a.line_rgba;
    const bool do_hist = a.hist_pos || a.hist_rgba;
    const bool do_disc = a.disc_pos || a.disc_rgba;
    const size_t segs = static_cast<size_t>(n - 1);

    for (uint32_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
        if (do_line) {   // update.rs:506-579
            const float* xr = a.x + static_cast<size_t>(row) * n;
            // util::arg_max (util.rs:48-57): the FIRST maximum; with both signs of zero in the row the first one's sign is the value,
            // so every lane carries (value, bin) and ends with the same pair
            float best = scene::F32_MIN;
            uint32_t best_at = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int bin = lane + 64 * k;
                const float v = bin < n ? xr[bin] : 0.0f;
                if (bin < n && v > best) {
                    best = v;
                    best_at = static_cast<uint32_t>(bin);
                }
            }
            for (int o = 32; o; o >>= 1) {
                const float other = __shfl_xor(best, o);
                const uint32_t other_at = __shfl_xor(best_at, o);
                if (other > best || (!(other < best) && other_at < best_at)) {   // (a NaN never gets into `best`)
                    best = other;
                    best_at = other_at;
                }
            }
            const float max_size = best_at != 0xFFFFFFFFu ? best : xr[0];   // update.rs:512-513
            // (the row is read again, from cache: a segment's 28 store registers are live one or two segments at a time, not NK)
#pragma unroll 2
            for (int k = 0; k < NK; ++k) {
                const int seg = lane + 64 * k;
                if (seg < n - 1) {
                    const size_t at = static_cast<size_t>(row) * segs + seg;
                    const float x0 = xr[seg], x1 = xr[seg + 1];
                    if (a.line_pos) {
                        float q[12];
                        panels::spectrum_quad(static_cast<uint32_t>(seg), x0, x1, q);
                        store_quad(a.line_pos, at, q);
                    }
                    if (a.line_rgba)
                        store_rgba(a.line_rgba, at, s_rgb[3 * seg], s_rgb[3 * seg + 1], s_rgb[3 * seg + 2], panels::spectrum_alpha(x0, max_size));
                }
            }
        }
        if (do_hist) {   // update.rs:787-845
            const float* cr = a.calmness + static_cast<size_t>(row) * n;
#pragma unroll 2
            for (int k = 0; k < NK; ++k) {
                const int seg = lane + 64 * k;
                if (seg < n - 1) {
                    const size_t at = static_cast<size_t>(row) * segs + seg;
                    const float c0 = cr[seg], c1 = cr[seg + 1];
                    if (a.hist_pos) {
                        float q[12];
                        panels::histogram_quad(static_cast<uint32_t>(seg), c0, c1, q);
                        store_quad(a.hist_pos, at, q);
                    }
                    if (a.hist_rgba) {
                        float r, g, b;
                        panels::calmness_to_color(panels::histogram_class_value(c0, c1), r, g, b);
                        store_rgba(a.hist_rgba, at, r, g, b, 1.0f);
                    }
                }
            }
        }
        if (do_disc) {   // update.rs:582-615
            const uint32_t cnt = min(a.peak_count[row], a.max_peaks);
            const float* c_row = a.center + static_cast<size_t>(row) * a.max_peaks;
            const float* z_row = a.size + static_cast<size_t>(row) * a.max_peaks;
            for (uint32_t base = 0; base < a.max_peaks; base += 64) {
                const uint32_t slots = min(64u, a.max_peaks - base);        // of the arrays
                const uint32_t live = cnt > base ? min(cnt - base, 64u) : 0u;   // of the list: entries beyond the count are never read
                __syncthreads();   // the previous chunk's readers are done
                if (static_cast<uint32_t>(lane) < live) {
                    float cx, cy;
                    uint32_t at;
                    panels::disc_of_peak(a.bpo, c_row[base + lane], z_row[base + lane], cx, cy, at);
                    s_cx[lane] = cx;
                    s_cy[lane] = cy;
                    s_at[lane] = at;
                }
                __syncthreads();
                const size_t first = static_cast<size_t>(row) * a.max_peaks + base;
                if (a.disc_pos) {
                    float* o = a.disc_pos + first * POS_PER_DISC;
                    for (uint32_t d = lane; d < slots * POS_PER_DISC; d += 64) {
                        const uint32_t pk = d / POS_PER_DISC, rem = d - pk * POS_PER_DISC;
                        const uint32_t vtx = rem / 3u, comp = rem - 3u * vtx;
                        o[d] = pk < live ? panels::disc_coordinate(s_cx[pk], s_cy[pk], s_cs, vtx, comp) : 0.0f;
                    }
                }
                if (a.disc_rgba) {
                    float* o = a.disc_rgba + first * RGBA_PER_DISC;
                    for (uint32_t d = lane; d < slots * RGBA_PER_DISC; d += 64) {
                        const uint32_t pk = d / RGBA_PER_DISC, comp = d & 3u;
                        float val = 0.0f;
                        if (pk < live) val = comp == 3u ? panels::DISC_ALPHA : s_rgb[3 * s_at[pk] + comp];
                        o[d] = val;
                    }
                }
            }
            __syncthreads();   // s_cx, s_cy and s_at are the next row's
        }
    }
}

__global__ __launch_bounds__(64) void panels_graph(GraphArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x;
    const uint32_t cap = a.capacity;
    const uint32_t emitted = a.n_frames - a.first;
    const uint32_t rows = a.n_streams * emitted;
    const size_t segs = cap - 1u;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t s = r / emitted, f = a.first + r % emitted;
        const float* h = a.hist + static_cast<size_t>(s) * cap;
        const float* v = a.vals + static_cast<size_t>(s) * a.n_frames;
        for (uint32_t seg = lane; seg + 1u < cap; seg += 64) {
            // the window after frame f's push: entry i is entry f + 1 + i of [history | values] (update.rs:656-666)
            const uint32_t j0 = f + 1u + seg, j1 = j0 + 1u;   // j1 <= f + cap <= n_frames - 1 + cap
            const float h0 = j0 < cap ? h[j0] : v[j0 - cap];
            const float h1 = j1 < cap ? h[j1] : v[j1 - cap];
            const size_t at = static_cast<size_t>(r) * segs + seg;
            if (a.pos) {
                float q[12];
                panels::graph_quad(seg, cap, h0, h1, q);
                store_quad(a.pos, at, q);
            }
            if (a.rgba) {
                float cr, cg, cb;
                panels::calmness_to_color(h0, cr, cg, cb);   // update.rs:680-682
                store_rgba(a.rgba, at, cr, cg, cb, 1.0f);
            }
        }
    }
}

__global__ __launch_bounds__(256) void panels_history(GraphArgs a) {
    const size_t total = static_cast<size_t>(a.n_streams) * a.capacity;
    for (size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; t < total; t += static_cast<size_t>(gridDim.x) * 256) {
        const size_t s = t / a.capacity, i = t - s * a.capacity;
        const size_t j = static_cast<size_t>(a.n_frames) + i;   // of [history | values]
        a.hist_next[t] = j < a.capacity ? a.hist[s * a.capacity + j] : a.vals[s * a.n_frames + (j - a.capacity)];
    }
}

template <int NK>
void launch_nk(int nk, const RowsArgs& a, dim3 grid, hipStream_t stream) {
    if constexpr (NK > 16) {
        return;
    } else {
        if (nk == NK)
            hipLaunchKernelGGL(panels_rows<NK>, grid, dim3(64), 0, stream, a);
        else
            launch_nk<NK + 1>(nk, a, grid, stream);
    }
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
}  // namespace

pvq_status PanelsBatch::create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const float* colors, float gray_level,
                               uint32_t n_streams, uint32_t graph_capacity, std::unique_ptr<PanelsBatch>& out) {
    out.reset();
    if (octaves == 0 || buckets_per_octave == 0 || n_streams == 0) {
        set_last_error("panels batch: octaves, buckets_per_octave and n_streams must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (n < 3 || n > MAX_BINS) {
        set_last_error("unsupported: the batched panels take 3 .. 1024 bins");
        return PVQ_ERR_UNSUPPORTED;
    }
    const uint32_t cap = graph_capacity ? graph_capacity : panels::DEFAULT_GRAPH_CAPACITY;
    if (cap < 2 || cap > MAX_CAPACITY) {
        set_last_error("panels batch: graph_capacity must be 2 .. 1024 (0: 300)");
        return PVQ_ERR_INVALID_ARG;
    }
    if (static_cast<uint64_t>(n_streams) * cap > 0x7FFFFFFFull) {
        set_last_error("panels batch: too many streams");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<PanelsBatch> b(new PanelsBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_bins_ = static_cast<uint32_t>(n);
    b->bpo_ = buckets_per_octave;
    b->n_streams_ = n_streams;
    b->capacity_ = cap;
    if (device_id >= 0) {
        std::vector<PanelTables> host(1);
        PanelTables& t = host[0];
        std::fill(reinterpret_cast<char*>(&t), reinterpret_cast<char*>(&t + 1), 0);
        panel_color_table(buckets_per_octave, colors, gray_level, t.rgb);
        panel_disc_table(t.cs);
        const size_t hist_bytes = 2 * static_cast<size_t>(n_streams) * cap * sizeof(float);
        PVQ_HIP(hipSetDevice(device_id));
        if (pvq_status s = b->tab_.upload(&t, sizeof(PanelTables))) return s;
        if (pvq_status s = b->hist_.reserve(hist_bytes)) return s;
        PVQ_HIP(hipMemset(b->hist_.as<float>(), 0, hist_bytes));   // SceneCalmnessHistory::new (mod.rs:125-132)
        PVQ_HIP(hipDeviceSynchronize());
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status PanelsBatch::rows_device(size_t n_rows, const float* d_x_vqt_smoothed, const float* d_center, const float* d_size,
                                    const uint32_t* d_peak_count, uint32_t max_peaks, const float* d_calmness, const pvq_panels_outputs& outs,
                                    hipStream_t stream) {
    if ((outs.line_pos || outs.line_rgba) && !d_x_vqt_smoothed) {
        set_last_error("panels batch: line_pos and line_rgba read x_vqt_smoothed, which is null");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((outs.disc_pos || outs.disc_rgba) && (!d_center || !d_size || !d_peak_count || max_peaks == 0)) {
        set_last_error("panels batch: disc_pos and disc_rgba read center, size and peak_count, with max_peaks > 0");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((outs.hist_pos || outs.hist_rgba) && !d_calmness) {
        set_last_error("panels batch: hist_pos and hist_rgba read calmness, which is null");
        return PVQ_ERR_INVALID_ARG;
    }
    if (misaligned16(outs.line_pos) || misaligned16(outs.line_rgba) || misaligned16(outs.hist_pos) || misaligned16(outs.hist_rgba)) {
        set_last_error("panels batch: a line or histogram output must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(outs.disc_pos) | reinterpret_cast<uintptr_t>(outs.disc_rgba)) & 3) {
        set_last_error("panels batch: a disc output must be 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_rows > 0x7FFFFFFFull) {
        set_last_error("panels batch: too many rows in one call");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched panels run on a GPU; this handle has none (pvq_spectrum_mesh and pvq_calmness_histogram_mesh are the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_rows == 0 || !(outs.line_pos || outs.line_rgba || outs.disc_pos || outs.disc_rgba || outs.hist_pos || outs.hist_rgba)) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    RowsArgs a{};
    a.x = d_x_vqt_smoothed;
    a.center = d_center;
    a.size = d_size;
    a.peak_count = d_peak_count;
    a.calmness = d_calmness;
    a.max_peaks = max_peaks;
    a.n_rows = static_cast<uint32_t>(n_rows);
    a.n_bins = static_cast<int>(n_bins_);
    a.bpo = bpo_;
    a.tab = tab_.as<PanelTables>();
    a.line_pos = outs.line_pos;
    a.line_rgba = outs.line_rgba;
    a.disc_pos = outs.disc_pos;
    a.disc_rgba = outs.disc_rgba;
    a.hist_pos = outs.hist_pos;
    a.hist_rgba = outs.hist_rgba;
    // a wave per row, rows strided over at most 32 resident waves per CU of a 256-CU chip: the tables reach LDS once per workgroup
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(n_rows, 256 * 32)));
    launch_nk<1>(static_cast<int>((n_bins_ + 63) / 64), a, grid, stream);
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status PanelsBatch::graph_device(size_t n_frames, const float* d_scene_calmness, size_t first_emitted, float* graph_pos, float* graph_rgba,
                                     hipStream_t stream) {
    if (n_frames && !d_scene_calmness) {
        set_last_error("panels batch: the graph reads scene_calmness, which is null");
        return PVQ_ERR_INVALID_ARG;
    }
    if (first_emitted > n_frames) {
        set_last_error("panels batch: first_emitted lies beyond n_frames");
        return PVQ_ERR_INVALID_ARG;
    }
    if (misaligned16(graph_pos) || misaligned16(graph_rgba)) {
        set_last_error("panels batch: a graph output must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("panels batch", n_frames, n_streams_, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched panels run on a GPU; this handle has none (pvq_calmness_graph_* is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_frames == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    const size_t half = static_cast<size_t>(n_streams_) * capacity_;
    GraphArgs a{};
    a.hist = hist_.as<float>() + cur_ * half;
    a.hist_next = hist_.as<float>() + (1 - cur_) * half;
    a.vals = d_scene_calmness;
    a.n_streams = n_streams_;
    a.n_frames = static_cast<uint32_t>(n_frames);
    a.first = static_cast<uint32_t>(first_emitted);
    a.capacity = capacity_;
    a.pos = graph_pos;
    a.rgba = graph_rgba;
    const size_t rows = static_cast<size_t>(n_streams_) * (n_frames - first_emitted);
    if (rows && (graph_pos || graph_rgba)) {
        hipLaunchKernelGGL(panels_graph, dim3(static_cast<unsigned>(std::min<size_t>(rows, 256 * 32))), dim3(64), 0, stream, a);
        PVQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(panels_history, dim3(static_cast<unsigned>(std::min<size_t>((half + 255) / 256, 2048))), dim3(256), 0, stream, a);
    PVQ_HIP(hipGetLastError());
    cur_ = 1 - cur_;   // both kernels read the old half and are ordered on `stream` before the next call's
    return PVQ_OK;
}

pvq_status PanelsBatch::get_history(uint32_t stream_index, float* out) {
    if (stream_index >= n_streams_ || !out) {
        set_last_error("panels batch: stream_index out of range or a null array");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched panels run on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    const size_t half = static_cast<size_t>(n_streams_) * capacity_;
    PVQ_HIP(hipMemcpy(out, hist_.as<float>() + cur_ * half + static_cast<size_t>(stream_index) * capacity_, capacity_ * sizeof(float), hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
