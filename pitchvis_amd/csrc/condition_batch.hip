// condition_batch.hip — the trainer's stream conditioning for many streams, a lane per stream (condition_batch.hpp).
//
// Every arithmetic step below is train_condition_stream's / MonoAgc::process's (consumers_host.cpp, itself the reference's f32
// expressions, file:line cited there) with FMA contraction off, the correctly rounded fp32 division hipcc emits for a plain `/`, and
// fp32 subnormals kept (the default kernel mode) — so every sample and every gain carries the host's bits.
//
// Two kernels, because the gate of a chunk needs the chunk's whole sum before the chunk's first sample is scaled:
//   cond_gate        a lane per (stream, chunk): m = (l + r) / 2 written to the output row, sq += m * m in sample order (train.rs:286-293)
//   cond_recurrence  a lane per stream: the gain in a register, the output rows scaled in place, the gain after each chunk (lib.rs:76-86)
// A lane that walked its own row in memory would gather 4 bytes per lane and instruction.  Both kernels therefore move [64 rows] x
// [TS samples] tiles through LDS: a row's TS samples are contiguous in memory, so the wave loads them 16 bytes per lane, 16 lanes per
// row; in LDS a row is TS + 4 dwords long, which puts the 16-byte reads of the 16 lanes of a ds_read_b128 lane group on 16 distinct
// 4-bank slots (row r starts at bank 4 r mod 64), so the per-lane walk is free of bank conflicts.  The recurrence kernel holds the
// next tile in registers while it walks this one: its loads are in flight under the serial chain.
#include "condition_batch.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "consumers_host.hpp"
#include "vqt_engine.hpp"

namespace pvq {

struct CondStream {
    const float* left;
    const float* right;   // null: mono
    float* out;
    unsigned long long n_chunks;
};

struct CondArgs {
    const CondStream* tab;   // [n_streams]
    uint32_t n_streams, max_chunks;
    unsigned long long chunk;
    uint8_t* frozen;   // [max_chunks][n_streams]: 1 = the chunk's sum of squares is < 1e-6 (train.rs:293)
    float* gain;       // [n_streams] state
    float* gain_out;   // optional, [n_streams][gain_stride]
    unsigned long long gain_stride;
    float rms, d;
};

namespace {
constexpr int TS = 64;        // samples of a row per tile
constexpr int LDW = TS + 4;   // dwords of a row in LDS
constexpr int NQ = TS / 4;    // 16-byte pieces of a row = tile pieces per lane

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// elements [off, off + 4) of a row of `len` elements; zeros past its end (a row of length 0 is never dereferenced)
__device__ __forceinline__ float4 row_load4(const float* p, unsigned long long off, unsigned long long len) {
    const float* q = p + off;
    if (off + 4 <= len && aligned16(q)) return *reinterpret_cast<const float4*>(q);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (off < len) v.x = q[0];
    if (off + 1 < len) v.y = q[1];
    if (off + 2 < len) v.z = q[2];
    if (off + 3 < len) v.w = q[3];
    return v;
}
// nothing at or past `len` is written
__device__ __forceinline__ void row_store4(float* p, unsigned long long off, unsigned long long len, float4 v) {
    float* q = p + off;
    if (off + 4 <= len && aligned16(q)) {
        *reinterpret_cast<float4*>(q) = v;
        return;
    }
    if (off < len) q[0] = v.x;
    if (off + 1 < len) q[1] = v.y;
    if (off + 2 < len) q[2] = v.z;
    if (off + 3 < len) q[3] = v.w;
}

// The usual tile: every row either holds all TS samples of it on the 16-byte grid or none.  Its pieces then move without a branch — a
// piece of a row that is not there reads `spare` (16 valid bytes) and becomes zeros — so the 16 loads of a lane are in flight together;
// behind the branches of row_load4 each would wait for the one before.
__device__ __forceinline__ bool row_whole(const float* p, unsigned long long t0, unsigned long long len) {
    return t0 >= len || (t0 + TS <= len && aligned16(p + t0));
}
__device__ __forceinline__ float4 piece_load(const float* p, unsigned long long off, bool there, const void* spare) {
    const float4 v = *reinterpret_cast<const float4*>(there ? static_cast<const void*>(p + off) : spare);
    return there ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// train.rs:286-293 for one chunk per lane: piece k of the tile is row 4 k + lane / 16, samples 4 (lane % 16) .. + 3
__global__ __launch_bounds__(64) void cond_gate(CondArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float tile[64 * LDW];
    __shared__ const float* row_l[64];
    __shared__ const float* row_r[64];
    __shared__ float* row_o[64];
    const int lane = threadIdx.x;
    const unsigned long long item = (unsigned long long)blockIdx.x * 64 + lane;
    const unsigned long long s = item / a.max_chunks, c = item % a.max_chunks;
    bool valid = s < a.n_streams;
    if (valid) {
        const CondStream st = a.tab[s];
        valid = c < st.n_chunks;
        const unsigned long long o = c * a.chunk;
        row_l[lane] = valid ? st.left + o : nullptr;   // (a null left marks a row without a chunk)
        row_r[lane] = valid && st.right ? st.right + o : nullptr;
        row_o[lane] = valid ? st.out + o : nullptr;
    } else {
        row_l[lane] = nullptr;
        row_r[lane] = nullptr;
        row_o[lane] = nullptr;
    }
    __syncthreads();
    const int prow = lane >> 4, pcol = (lane & 15) * 4;
    float sq = 0.0f;
    for (unsigned long long t0 = 0; t0 < a.chunk; t0 += TS) {
        float4 m[NQ];   // every load of the tile before its first store: the output row may be the left row
        const bool whole = __all(row_whole(row_l[lane], t0, row_l[lane] ? a.chunk : 0) && row_whole(row_r[lane], t0, row_r[lane] ? a.chunk : 0) &&
                                 row_whole(row_o[lane], t0, row_o[lane] ? a.chunk : 0));
        if (whole) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int row = 4 * k + prow;
                const float* l = row_l[row];
                const float* r = row_r[row];
                m[k] = piece_load(l, t0 + pcol, l != nullptr, a.tab);
                const float4 q = piece_load(r, t0 + pcol, r != nullptr, a.tab);
                m[k].x = r ? (m[k].x + q.x) / 2.0f : m[k].x;   // train.rs:286-289
                m[k].y = r ? (m[k].y + q.y) / 2.0f : m[k].y;
                m[k].z = r ? (m[k].z + q.z) / 2.0f : m[k].z;
                m[k].w = r ? (m[k].w + q.w) / 2.0f : m[k].w;
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int row = 4 * k + prow;
                float* o = row_o[row];
                if (o) *reinterpret_cast<float4*>(o + t0 + pcol) = m[k];
                *reinterpret_cast<float4*>(&tile[row * LDW + pcol]) = m[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int row = 4 * k + prow;
                const float* l = row_l[row];
                const float* r = row_r[row];
                const unsigned long long len = l ? a.chunk : 0;
                m[k] = row_load4(l, t0 + pcol, len);
                if (r) {
                    const float4 q = row_load4(r, t0 + pcol, len);
                    m[k].x = (m[k].x + q.x) / 2.0f;
                    m[k].y = (m[k].y + q.y) / 2.0f;
                    m[k].z = (m[k].z + q.z) / 2.0f;
                    m[k].w = (m[k].w + q.w) / 2.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int row = 4 * k + prow;
                row_store4(row_o[row], t0 + pcol, row_l[row] ? a.chunk : 0, m[k]);
                *reinterpret_cast<float4*>(&tile[row * LDW + pcol]) = m[k];
            }
        }
        __syncthreads();
        const int n = (int)min((unsigned long long)TS, a.chunk - t0);
        for (int j = 0; j < n; j += 4) {   // train.rs:292, in sample order; past the chunk's end the tile holds zeros: sq + 0 = sq
            const float4 v = *reinterpret_cast<const float4*>(&tile[lane * LDW + j]);
            sq = sq + v.x * v.x;
            sq = sq + v.y * v.y;
            sq = sq + v.z * v.z;
            sq = sq + v.w * v.w;
        }
        __syncthreads();
    }
    if (valid) a.frozen[c * a.n_streams + s] = sq < 1e-6f ? 1 : 0;   // train.rs:293
}

// lib.rs:76-86 for one stream per lane over the rows cond_gate wrote.  Every stream starts at sample 0 and has the same chunk length, so
// the chunk boundaries are the same for all lanes (scalar branches); a lane past its stream's end keeps its gain and stores nothing.
// STEP: samples between two looks at the chunk boundary (4: chunk is a multiple of 4; 1: any chunk).
template <int STEP>
__global__ __launch_bounds__(64) void cond_recurrence(CondArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float tile[64 * LDW];
    __shared__ float* row_o[64];
    __shared__ unsigned long long row_len[64];
    const int lane = threadIdx.x;
    const unsigned long long s = (unsigned long long)blockIdx.x * 64 + lane;
    const bool valid = s < a.n_streams;
    uint32_t my_chunks = 0;
    float gain = 1.0f;
    float* out = nullptr;
    if (valid) {
        const CondStream st = a.tab[s];
        my_chunks = (uint32_t)st.n_chunks;
        out = st.out;
        gain = a.gain[s];
    }
    row_o[lane] = out;
    row_len[lane] = my_chunks * a.chunk;
    uint32_t wave_chunks = my_chunks;
    for (int o = 32; o; o >>= 1) wave_chunks = max(wave_chunks, (uint32_t)__shfl_xor((int)wave_chunks, o));
    const unsigned long long wave_len = wave_chunks * a.chunk;
    __syncthreads();
    const int prow = lane >> 4, pcol = (lane & 15) * 4;
    float4 next[NQ];   // the tile after the one in LDS
    auto load_tile = [&](unsigned long long t0) {
        if (__all(row_whole(out, t0, row_len[lane]))) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) next[k] = piece_load(row_o[4 * k + prow], t0 + pcol, t0 < row_len[4 * k + prow], a.tab);
        } else {
#pragma unroll
            for (int k = 0; k < NQ; ++k) next[k] = row_load4(row_o[4 * k + prow], t0 + pcol, row_len[4 * k + prow]);
        }
    };
    load_tile(0);
    uint32_t c = 0;               // the chunk the walk is in, and the position in it: the same for every lane
    unsigned long long pos = 0;
    bool update = false, active = false;
    uint8_t frozen_next = my_chunks ? a.frozen[s] : 1;
    for (unsigned long long t0 = 0; t0 < wave_len; t0 += TS) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) *reinterpret_cast<float4*>(&tile[(4 * k + prow) * LDW + pcol]) = next[k];
        __syncthreads();
        if (t0 + TS < wave_len) load_tile(t0 + TS);
        const int n = (int)min((unsigned long long)TS, wave_len - t0);
        float v[TS];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float4 f = *reinterpret_cast<const float4*>(&tile[lane * LDW + 4 * q]);
            v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
        }
#pragma unroll
        for (int j = 0; j < TS; j += STEP) {
            if (j < n) {
                if (pos == 0) {   // train.rs:293: the chunk's gate; the next chunk's is fetched a chunk ahead
                    active = c < my_chunks;
                    update = active && !frozen_next;
                    frozen_next = c + 1 < my_chunks ? a.frozen[(unsigned long long)(c + 1) * a.n_streams + s] : 1;
                }
#pragma unroll
                for (int k = 0; k < STEP; ++k) {   // lib.rs:77-85
                    const float x = v[j + k] * gain;
                    v[j + k] = x;
                    const float y = (x * x) / a.rms;
                    float g = 1.0f + (a.d * (1.0f - y));
                    g = fmaxf(g, a.d);   // f32::max: a NaN g yields d
                    gain = update ? gain * g : gain;
                }
                pos += STEP;
                if (pos == a.chunk) {
                    if (active && a.gain_out) a.gain_out[s * a.gain_stride + c] = gain;
                    ++c;
                    pos = 0;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            *reinterpret_cast<float4*>(&tile[lane * LDW + 4 * q]) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        __syncthreads();
        if (__all(row_whole(out, t0, row_len[lane]))) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int row = 4 * k + prow;
                if (t0 < row_len[row]) *reinterpret_cast<float4*>(row_o[row] + t0 + pcol) = *reinterpret_cast<const float4*>(&tile[row * LDW + pcol]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int row = 4 * k + prow;
                row_store4(row_o[row], t0 + pcol, row_len[row], *reinterpret_cast<const float4*>(&tile[row * LDW + pcol]));
            }
        }
        __syncthreads();
    }
    if (valid) a.gain[s] = gain;
}
}  // namespace

pvq_status AgcBatch::create(int device_id, uint32_t n_streams, float desired_output_rms, float distortion_factor, std::unique_ptr<AgcBatch>& out) {
    out.reset();
    std::string why;
    if (!MonoAgc::valid(desired_output_rms, distortion_factor, &why)) {   // lib.rs:36-49
        set_last_error(why);
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_streams == 0) {
        set_last_error("zero streams");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<AgcBatch> b(new AgcBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_streams_ = n_streams;
    b->desired_output_rms_ = desired_output_rms;
    b->distortion_factor_ = distortion_factor;
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        const std::vector<float> ones(n_streams, 1.0f);   // lib.rs:50: gain = 1
        if (pvq_status s = b->gain_.upload(ones.data(), n_streams * sizeof(float))) return s;
        if (pvq_status s = b->tab_.reserve(n_streams * sizeof(CondStream))) return s;
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status AgcBatch::condition_device(const float* const* d_left, const float* const* d_right, const size_t* n_chunks, size_t chunk,
                                      float* const* d_mono_out, float* d_gain_out, size_t gain_stride, hipStream_t stream) {
    if (chunk == 0 || !d_left || !n_chunks || !d_mono_out) {
        set_last_error("agc batch: chunk must be positive and the left, n_chunks and output tables non-null");
        return PVQ_ERR_INVALID_ARG;
    }
    std::vector<CondStream> tab(n_streams_);
    size_t max_chunks = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        if (n_chunks[s] && (!d_left[s] || !d_mono_out[s])) {
            set_last_error("agc batch: stream " + std::to_string(s) + " has a null left or output pointer");
            return PVQ_ERR_INVALID_ARG;
        }
        if (n_chunks[s] > 0x7fffffffull || (n_chunks[s] && chunk > (~0ull >> 1) / n_chunks[s])) {
            set_last_error("agc batch: stream " + std::to_string(s) + " is too long");
            return PVQ_ERR_INVALID_ARG;
        }
        if (d_gain_out && gain_stride < n_chunks[s]) {
            set_last_error("agc batch: gain_stride is smaller than the chunk count of stream " + std::to_string(s));
            return PVQ_ERR_INVALID_ARG;
        }
        tab[s] = CondStream{d_left[s], d_right ? d_right[s] : nullptr, d_mono_out[s], n_chunks[s]};
        max_chunks = std::max(max_chunks, n_chunks[s]);
    }
    const unsigned long long gate_blocks = ((unsigned long long)n_streams_ * max_chunks + 63) / 64;
    if (gate_blocks > 0x7fffffffull) {
        set_last_error("agc batch: more than 2^37 chunks in one call");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched conditioning runs on a GPU; this handle has none (pvq_train_condition_stream is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (max_chunks == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    if (pvq_status s = frozen_.reserve((size_t)n_streams_ * max_chunks)) return s;
    PVQ_HIP(hipMemcpyAsync(tab_.as<void>(), tab.data(), tab.size() * sizeof(CondStream), hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns)
    CondArgs a{};
    a.tab = tab_.as<CondStream>();
    a.n_streams = n_streams_;
    a.max_chunks = (uint32_t)max_chunks;
    a.chunk = chunk;
    a.frozen = frozen_.as<uint8_t>();
    a.gain = gain_.as<float>();
    a.gain_out = d_gain_out;
    a.gain_stride = gain_stride;
    a.rms = desired_output_rms_;
    a.d = distortion_factor_;
    hipLaunchKernelGGL(cond_gate, dim3((unsigned)gate_blocks), dim3(64), 0, stream, a);
    const dim3 waves((n_streams_ + 63) / 64);
    if (chunk % 4 == 0)
        hipLaunchKernelGGL(cond_recurrence<4>, waves, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(cond_recurrence<1>, waves, dim3(64), 0, stream, a);
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status AgcBatch::get_gains(float* gains) {
    if (!gains) {
        set_last_error("null output");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {   // nothing ever ran: lib.rs:50
        std::fill(gains, gains + n_streams_, 1.0f);
        return PVQ_OK;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    PVQ_HIP(hipMemcpy(gains, gain_.as<float>(), n_streams_ * sizeof(float), hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
