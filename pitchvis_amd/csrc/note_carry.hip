// note_carry.hip — see note_carry.hpp.
//
// The three kernels move a few frames per stream; none of them is near any limit of the device, so they are written for being
// plainly right: a workgroup column per stream (blockIdx.x), the floats or rows of that stream strided over the threads of its
// blockIdx.y workgroups.  A stream that gets no frame in the call (n == 0) is left alone by all three.
#include "note_carry.hpp"

#include <algorithm>
#include <string>

namespace pvq {

namespace {
constexpr int NC_THREADS = 256;
constexpr uint32_t NC_MAX_Y = 64;   // workgroups per stream at most; beyond, a thread takes several elements
static_assert(sizeof(NcStream) == 32 && sizeof(NmRow) == 16, "read by the kernels as laid out in note_model_plan.hpp and note_model_half.hpp");

struct NcArgs {
    const NcStream* desc;   // [n_streams]
    const float* db;        // [n_streams][stride_frames][n_bins]
    float* tail;            // [n_streams][lead][n_bins]
    float* stitch;          // [n_streams][2 lead][n_bins]
    NmRow* rows;            // [tiles * 128]
    NmTile* tiles;          // [tiles]
    size_t stride_frames;
    uint32_t n_bins, t_frames;
    uint32_t lead;          // t_frames - 1
    uint32_t total_rows;
};

// stitch[s] = tail[s] (lead frames), then the call's first min(n, lead) frames
__global__ __launch_bounds__(NC_THREADS) void nc_stitch(const NcArgs a) {
    const uint32_t s = blockIdx.x;
    const NcStream st = a.desc[s];
    if (st.n == 0u) return;
    const size_t half = static_cast<size_t>(a.lead) * a.n_bins;
    const size_t fresh = static_cast<size_t>(min(st.n, a.lead)) * a.n_bins;
    const float* tail = a.tail + s * half;
    const float* db = a.db + static_cast<size_t>(s) * a.stride_frames * a.n_bins;
    float* dst = a.stitch + 2 * half * s;
    for (size_t i = static_cast<size_t>(blockIdx.y) * NC_THREADS + threadIdx.x; i < half + fresh; i += static_cast<size_t>(gridDim.y) * NC_THREADS)
        dst[i] = i < half ? tail[i] : db[i - half];
}

// the row table and the tile list from the descriptors (note_carry_row is the one copy of the rule)
__global__ __launch_bounds__(NC_THREADS) void nc_rows(const NcArgs a) {
    const uint32_t s = blockIdx.x;
    const NcStream st = a.desc[s];
    const float* stitched = a.stitch + 2 * static_cast<size_t>(s) * a.lead * a.n_bins;
    for (uint32_t i = blockIdx.y * NC_THREADS + threadIdx.x; i < st.rows; i += gridDim.y * NC_THREADS) {
        const NcRow r = note_carry_row(st, s, i, a.t_frames, a.n_bins, a.stride_frames);
        const uint32_t at = st.first_row + i;
        NmRow out;
        out.x = (r.in_stitch ? stitched : a.db) + r.at;
        out.out_row = r.out_row;
        a.rows[at] = out;
        if (at % NM_BM == 0u) a.tiles[at / NM_BM] = NmTile{0u, 0u, min(static_cast<uint32_t>(NM_BM), a.total_rows - at), 0u};
    }
}

// tail[s] = the last `lead` frames of (old tail, the call's n frames): from d_db when the call alone holds them, else from the
// stitched buffer, where they are frames n .. n + lead - 1
__global__ __launch_bounds__(NC_THREADS) void nc_tail_save(const NcArgs a) {
    const uint32_t s = blockIdx.x;
    const NcStream st = a.desc[s];
    if (st.n == 0u) return;
    const size_t half = static_cast<size_t>(a.lead) * a.n_bins;
    const float* src = st.n >= a.lead ? a.db + (static_cast<size_t>(s) * a.stride_frames + (st.n - a.lead)) * a.n_bins
                                      : a.stitch + 2 * half * s + static_cast<size_t>(st.n) * a.n_bins;
    float* dst = a.tail + s * half;
    for (size_t i = static_cast<size_t>(blockIdx.y) * NC_THREADS + threadIdx.x; i < half; i += static_cast<size_t>(gridDim.y) * NC_THREADS) dst[i] = src[i];
}

uint32_t y_blocks(size_t elements) { return static_cast<uint32_t>(std::min<size_t>(NC_MAX_Y, std::max<size_t>(1, (elements + NC_THREADS - 1) / NC_THREADS))); }
}  // namespace

NoteCarry::~NoteCarry() {
    if (device_id_ < 0) return;
    (void)hipSetDevice(device_id_);   // the buffers go after this body, with their device set
    for (int i = 0; i < NC_RING; ++i)
        if (copied_[i]) {
            if (in_flight_[i]) (void)hipEventSynchronize(copied_[i]);   // the pinned slots are freed below
            (void)hipEventDestroy(copied_[i]);
        }
    if (staged_) (void)hipHostFree(staged_);
}

pvq_status NoteCarry::create(const NoteModelDims& d, int device_id, uint32_t n_streams, std::unique_ptr<NoteCarry>& out) {
    out.reset();
    if (n_streams == 0) {
        set_last_error("note carry: n_streams must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<NoteCarry> c(new NoteCarry());
    c->device_id_ = device_id < 0 ? -1 : device_id;
    c->n_streams_ = n_streams;
    c->n_bins_ = d.n_bins;
    c->t_frames_ = d.t_frames;
    c->seen_.assign(n_streams, 0u);
    c->plan_.streams.resize(n_streams);
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        if (pvq_status s = c->desc_.reserve(static_cast<size_t>(n_streams) * sizeof(NcStream))) return s;
        PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->staged_), static_cast<size_t>(NC_RING) * n_streams * sizeof(NcStream), hipHostMallocDefault));
        for (int i = 0; i < NC_RING; ++i) PVQ_HIP(hipEventCreateWithFlags(&c->copied_[i], hipEventDisableTiming));
        const size_t half = static_cast<size_t>(n_streams) * (d.t_frames - 1u) * d.n_bins * sizeof(float);
        if (half) {   // (t_frames == 1: nothing is carried)
            if (pvq_status s = c->tail_.reserve(half)) return s;
            if (pvq_status s = c->stitch_.reserve(2 * half)) return s;
            PVQ_HIP(hipMemset(c->tail_.as<char>(), 0, half));
            PVQ_HIP(hipMemset(c->stitch_.as<char>(), 0, 2 * half));
        }
    }
    out = std::move(c);
    return PVQ_OK;
}

pvq_status NoteCarry::reset(int64_t stream_index, hipStream_t stream) {
    if (stream_index >= static_cast<int64_t>(n_streams_)) {
        set_last_error("note carry: stream index out of range");
        return PVQ_ERR_INVALID_ARG;
    }
    const size_t per = static_cast<size_t>(t_frames_ - 1u) * n_bins_ * sizeof(float);
    if (stream_index < 0) std::fill(seen_.begin(), seen_.end(), 0u);
    else seen_[static_cast<size_t>(stream_index)] = 0u;
    if (device_id_ >= 0 && per) {
        PVQ_HIP(hipSetDevice(device_id_));
        if (stream_index < 0) PVQ_HIP(hipMemsetAsync(tail_.as<char>(), 0, per * n_streams_, stream));
        else PVQ_HIP(hipMemsetAsync(tail_.as<char>() + per * static_cast<size_t>(stream_index), 0, per, stream));
    }
    return PVQ_OK;
}

pvq_status NoteCarry::frames_seen(uint32_t stream_index, uint64_t* out) const {
    if (!out || stream_index >= n_streams_) {
        set_last_error("note carry: stream index out of range or null output");
        return PVQ_ERR_INVALID_ARG;
    }
    *out = seen_[stream_index];
    return PVQ_OK;
}

pvq_status NoteCarry::plan(const NoteModelDims& d, const size_t* n_frames, size_t stride_frames) {
    std::string err;
    const pvq_status st = note_carry_plan(d, seen_.data(), n_frames, n_streams_, stride_frames, plan_, err);
    if (st != PVQ_OK) set_last_error(err);
    return st;
}

pvq_status NoteCarry::stage(const float* d_db, size_t stride_frames, NmTile* d_tiles, hipStream_t stream) {
    if (pvq_status s = rows_.reserve(std::max<size_t>(1, plan_.tiles) * NM_BM * sizeof(NmRow))) return s;
    // the descriptors through this call's pinned slot: the copy is queued like the kernels, the plan may change as soon as this returns
    const int slot = static_cast<int>(calls_++ % NC_RING);
    if (in_flight_[slot]) PVQ_HIP(hipEventSynchronize(copied_[slot]));   // (only NC_RING calls ahead of the device)
    NcStream* src = staged_ + static_cast<size_t>(slot) * n_streams_;
    std::copy(plan_.streams.begin(), plan_.streams.end(), src);
    PVQ_HIP(hipMemcpyAsync(desc_.as<NcStream>(), src, static_cast<size_t>(n_streams_) * sizeof(NcStream), hipMemcpyHostToDevice, stream));
    PVQ_HIP(hipEventRecord(copied_[slot], stream));
    in_flight_[slot] = true;
    NcArgs a{};
    a.desc = desc_.as<NcStream>();
    a.db = d_db;
    a.tail = tail_.as<float>();
    a.stitch = stitch_.as<float>();
    a.rows = rows_.as<NmRow>();
    a.tiles = d_tiles;
    a.stride_frames = stride_frames;
    a.n_bins = n_bins_;
    a.t_frames = t_frames_;
    a.lead = t_frames_ - 1u;
    a.total_rows = static_cast<uint32_t>(plan_.total_rows);
    if (a.lead && plan_.max_n)
        hipLaunchKernelGGL(nc_stitch, dim3(n_streams_, y_blocks(2 * static_cast<size_t>(a.lead) * n_bins_)), dim3(NC_THREADS), 0, stream, a);
    if (plan_.total_rows) hipLaunchKernelGGL(nc_rows, dim3(n_streams_, y_blocks(plan_.max_rows)), dim3(NC_THREADS), 0, stream, a);
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status NoteCarry::commit(const float* d_db, size_t stride_frames, hipStream_t stream) {
    NcArgs a{};
    a.desc = desc_.as<NcStream>();
    a.db = d_db;
    a.tail = tail_.as<float>();
    a.stitch = stitch_.as<float>();
    a.stride_frames = stride_frames;
    a.n_bins = n_bins_;
    a.t_frames = t_frames_;
    a.lead = t_frames_ - 1u;
    if (a.lead && plan_.max_n) {
        hipLaunchKernelGGL(nc_tail_save, dim3(n_streams_, y_blocks(static_cast<size_t>(a.lead) * n_bins_)), dim3(NC_THREADS), 0, stream, a);
        PVQ_HIP(hipGetLastError());
    }
    for (uint32_t s = 0; s < n_streams_; ++s) seen_[s] += plan_.streams[s].n;
    return PVQ_OK;
}

}  // namespace pvq
