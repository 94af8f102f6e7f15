// note_model_half.hip — see note_model_half.hpp.
//
// nmh_features: a wave per row and 64 pooled positions.  A lane reads x[4 p .. 4 p + 6] of its row's window, runs the 16 channels'
// two conv positions as the fmaf chain of nm_conv_fc1 (from the bias, one fmaf per tap), takes max(e, o, 0), rounds the 16 values
// and stores them as two 16-byte words at k' = 16 p: a wave writes 2 KiB of one row in order.  Rows of a tile past its last valid
// one, up to the next multiple of 32 (what an active wave of nmh_dense reads), and the half chunk past an odd O_pool are zeros.
//
// nmh_dense: the tile scheme of note_model.hip — 4 waves own 128 rows x 64 columns, wave w rows 32 w .. 32 w + 31 and all 64
// columns, 8 accumulator tiles; K is walked in stages of NM_PC = 4 chunks of 32; the stage's packed weights (16 KiB) go global ->
// registers -> LDS one stage ahead, double buffered, one barrier per stage; the activations go from global memory into registers
// a stage ahead, 16 bytes per lane, row tile and chunk — with the operand roles swapped: the packed weights are the instruction's
// A operand (matrix row = output column) and the activations its B operand (matrix column = activation row).  Lane l then holds,
// in register r of strip s, activation row l & 15 and output column 16 (l >> 4) + 4 s + r of the column tile (the packing numbers
// the columns so): 16 consecutive columns of one row, stored as two 16-byte words of hidden activations or four float4 of logits.
// A row's result depends on its window alone: equal windows give equal bits wherever the row sits.
#include "note_model_half.hpp"

#include "note_device.hpp"

namespace pvq {

namespace {
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

constexpr int NMH_THREADS = 256;
constexpr int CHUNK_U4 = NM_BN * NM_KC16 * 2 / 16;   // 16-byte words of one chunk of the packed operand (4 strips x 64 lanes)
constexpr int STAGE_U4 = NM_PC * CHUNK_U4;           // ... of one stage
constexpr int STAGE_LD = STAGE_U4 / NMH_THREADS;     // words per thread per stage
static_assert(STAGE_U4 % NMH_THREADS == 0, "the stage copy is whole words per thread");
static_assert(sizeof(NmTile) == 16, "NmTile is read as laid out in note_model_plan.hpp");

// the two types: the element, eight of them as an operand, the instruction.  A plain cast rounds to nearest even.
template <int PREC>
struct Type16;
template <>
struct Type16<PVQ_NOTE_BF16> {
    using T = __bf16;
    using V8 = __attribute__((ext_vector_type(8))) __bf16;
    static __device__ __forceinline__ f32x4 mfma(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct Type16<PVQ_NOTE_F16> {
    using T = _Float16;
    using V8 = __attribute__((ext_vector_type(8))) _Float16;
    static __device__ __forceinline__ f32x4 mfma(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

struct NmhArgs {
    const NmTile* tiles;     // this launch's tiles
    const NmRow* rows;       // null, or the launch's row table as in note_model.hip's NmArgs
    const float* db;         // nmh_features: [n_streams][stride_frames][n_bins]
    const float* conv;       // nmh_features: conv weights [16][5], bias [16]
    const void* x_in;        // nmh_dense: [tiles * 128][k_pad], 16-bit
    const u32x4* w_packed;   // [column tiles][stages * NM_PC chunks][CHUNK_U4]
    const float* bias;       // [n], 16-byte aligned
    void* h_out;             // nmh_features: [tiles * 128][k_pad]; ACT 0: [tiles * 128][n_pad]; 16-bit
    float* prob;             // ACT 1: [n_streams][stride_frames][128], may be null
    float* logits;           //        the same
    uint32_t* mask;          //        [n_streams][stride_frames][4], may be null
    size_t stride_frames;
    uint32_t n_bins, t_frames, o_pool;
    uint32_t k_pad;          // row length of x_in (nmh_dense) or of h_out (nmh_features): whole chunks of 32
    uint32_t n, n_pad;       // columns of the product; row length of h_out
    uint32_t n_ct;           // column tiles
    uint32_t p_blocks;       // nmh_features: blocks of 64 pooled positions per row
};

template <int PREC>
__global__ __launch_bounds__(64) void nmh_features(const NmhArgs a) {
    using T = typename Type16<PREC>::T;
    using V8 = typename Type16<PREC>::V8;
    const uint32_t row_local = blockIdx.x / a.p_blocks, pb = blockIdx.x % a.p_blocks;
    const uint32_t tile_local = row_local / NM_BM, r = row_local % NM_BM;
    const NmTile tile = a.tiles[tile_local];
    if (r >= ((tile.n_valid + 31u) & ~31u)) return;   // (uniform) no wave of nmh_dense reads this row
    const uint32_t p = 64 * pb + threadIdx.x;
    if (p >= a.k_pad / NM_CH) return;
    V8 lo, hi;
#pragma unroll
    for (int c = 0; c < 8; ++c) lo[c] = hi[c] = static_cast<T>(0.0f);
    if (r < tile.n_valid && p < a.o_pool) {
        const float* xrow = (a.rows ? a.rows[row_local].x   // (uniform choice; row_local = 128 * tile_local + r)
                                    : a.db + (static_cast<size_t>(tile.stream) * a.stride_frames + tile.f0 + r - (a.t_frames - 1)) * a.n_bins) + 4 * p;
        float x[NM_KW + 2];
#pragma unroll
        for (int j = 0; j < NM_KW + 2; ++j) x[j] = xrow[j];   // 4 p + 6 <= L - 1 for p < o_pool
#pragma unroll
        for (int c = 0; c < NM_CH; ++c) {
            float e, o;   // conv positions 2 p and 2 p + 1
            conv_pair(a.conv + c * NM_KW, a.conv[NM_CH * NM_KW + c], x, e, o);
            const T v = static_cast<T>(fmaxf(fmaxf(e, o), 0.0f));
            if (c < 8) lo[c] = v;
            else hi[c - 8] = v;
        }
    }
    V8* dst = reinterpret_cast<V8*>(static_cast<T*>(a.h_out) + static_cast<size_t>(row_local) * a.k_pad + NM_CH * p);
    dst[0] = lo;
    dst[1] = hi;
}

__device__ __forceinline__ void stage_fetch(const u32x4* __restrict__ src, u32x4 (&r)[STAGE_LD]) {
#pragma unroll
    for (int j = 0; j < STAGE_LD; ++j) r[j] = src[threadIdx.x + NMH_THREADS * j];
}
__device__ __forceinline__ void stage_put(u32x4* dst, const u32x4 (&r)[STAGE_LD]) {
#pragma unroll
    for (int j = 0; j < STAGE_LD; ++j) dst[threadIdx.x + NMH_THREADS * j] = r[j];
}

// out = x_in * W^T + bias: ACT 0 -> ReLU -> rounded -> h_out; ACT 1 -> logits, sigmoid, mask (as nm_dense<1>)
template <int PREC, int ACT>
__global__ __launch_bounds__(NMH_THREADS, 2) void nmh_dense(const NmhArgs a) {
    using T = typename Type16<PREC>::T;
    using V8 = typename Type16<PREC>::V8;
    __shared__ u32x4 s_w[2][STAGE_U4];
    const uint32_t ct = blockIdx.x % a.n_ct, tile_local = blockIdx.x / a.n_ct;
    const NmTile tile = a.tiles[tile_local];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const bool active = static_cast<uint32_t>(32 * wave) < tile.n_valid;   // wave-uniform: a wave with no valid row only copies W
    const uint32_t chunks = a.k_pad / NM_KC16;
    const uint32_t stages = (chunks + NM_PC - 1) / NM_PC;
    const u32x4* wsrc = a.w_packed + static_cast<size_t>(ct) * stages * STAGE_U4;
    // rows of the activation buffer: every row of an active wave was written by the previous kernel
    const u32x4* xrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
        xrow[t] = reinterpret_cast<const u32x4*>(static_cast<const T*>(a.x_in) + (static_cast<size_t>(tile_local) * NM_BM + 32 * wave + 16 * t + (lane & 15)) * a.k_pad) + g;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 xv[NM_PC][2], xn[NM_PC][2];
    u32x4 wreg[STAGE_LD];
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t][s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    stage_fetch(wsrc, wreg);
    if (active) {
#pragma unroll
        for (int i = 0; i < NM_PC; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t) xv[i][t] = static_cast<uint32_t>(i) < chunks ? xrow[t][4 * i] : zero;
    }
    stage_put(s_w[0], wreg);
    __syncthreads();

    for (uint32_t st = 0; st < stages; ++st) {
        const bool more = st + 1 < stages;
        if (more) {
            stage_fetch(wsrc + static_cast<size_t>(st + 1) * STAGE_U4, wreg);
            if (active) {
#pragma unroll
                for (int i = 0; i < NM_PC; ++i) {
                    const uint32_t kc = NM_PC * (st + 1) + i;   // (a chunk past the row's end is not read)
#pragma unroll
                    for (int t = 0; t < 2; ++t) xn[i][t] = kc < chunks ? xrow[t][4 * kc] : zero;
                }
            }
        }
        if (active) {
            const u32x4* sw = s_w[st & 1];
#pragma unroll
            for (int i = 0; i < NM_PC; ++i)
                if (NM_PC * st + i < chunks) {   // (uniform) the padded chunks of the last stage are skipped
                    u32x4 w[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) w[s] = sw[i * CHUNK_U4 + s * 64 + lane];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int t = 0; t < 2; ++t)
                            acc[t][s] = Type16<PREC>::mfma(__builtin_bit_cast(V8, w[s]), __builtin_bit_cast(V8, xv[i][t]), acc[t][s]);
                }
            if (more) {
#pragma unroll
                for (int i = 0; i < NM_PC; ++i)
#pragma unroll
                    for (int t = 0; t < 2; ++t) xv[i][t] = xn[i][t];
            }
        }
        if (more) stage_put(s_w[(st + 1) & 1], wreg);
        __syncthreads();
    }
    if (!active) return;

    // accumulator layout with the roles swapped: lane l holds activation row l & 15, columns cb + 4 s + reg
    const uint32_t cb = NM_BN * ct + 16 * g;
    f32x4 bias[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) bias[s] = cb < a.n ? reinterpret_cast<const f32x4*>(a.bias + cb)[s] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t r = 32 * wave + 16 * t + (lane & 15);   // row of the tile
        if constexpr (ACT == 0) {
            if (cb < a.n_pad) {   // (columns n .. n_pad - 1, the half chunk of the next layer's K: acc and bias are zero)
                V8 lo, hi;
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        lo[4 * s + reg] = static_cast<T>(fmaxf(acc[t][s][reg] + bias[s][reg], 0.0f));
                        hi[4 * s + reg] = static_cast<T>(fmaxf(acc[t][s + 2][reg] + bias[s + 2][reg], 0.0f));
                    }
                V8* dst = reinterpret_cast<V8*>(static_cast<T*>(a.h_out) + (static_cast<size_t>(tile_local) * NM_BM + r) * a.n_pad + cb);
                dst[0] = lo;
                dst[1] = hi;
            }
        } else {
            f32x4 logit[4];
            uint32_t bits = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                logit[s] = acc[t][s] + bias[s];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) bits |= (logit[s][reg] > 0.0f ? 1u : 0u) << (4 * s + reg);
            }
            const uint32_t upper = __shfl_xor(bits, 16);   // the row's next 16 columns (lane group g ^ 1); every lane takes part
            if (r < tile.n_valid) {
                const size_t row = a.rows ? a.rows[static_cast<size_t>(tile_local) * NM_BM + r].out_row
                                          : static_cast<size_t>(tile.stream) * a.stride_frames + tile.f0 + r;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const size_t at = row * NM_OUT + cb + 4 * s;
                    if (a.logits) *reinterpret_cast<f32x4*>(a.logits + at) = logit[s];
                    if (a.prob) {
                        f32x4 p;
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) p[reg] = 1.0f / (1.0f + expf(-logit[s][reg]));
                        *reinterpret_cast<f32x4*>(a.prob + at) = p;
                    }
                }
                if (a.mask && !(g & 1)) a.mask[row * 4 + 2 * ct + (g >> 1)] = bits | (upper << 16);
            }
        }
    }
}

// the three kernels of a type
struct Kernels {
    void (*features)(NmhArgs);
    void (*hidden)(NmhArgs);
    void (*output)(NmhArgs);
};
template <int PREC>
constexpr Kernels kernels_of() {
    return Kernels{nmh_features<PREC>, nmh_dense<PREC, 0>, nmh_dense<PREC, 1>};
}
}  // namespace

void nmh_chunk(const NmContext& c, const NmTile* d_tiles, const NmRow* d_rows, uint32_t nt, const float* d_db, size_t stride_frames,
               const pvq_note_model_outputs& outs, hipStream_t stream) {
    const NoteModelDims& d = c.d;
    const NmWorkspace& w = c.at;
    const Kernels kern = c.precision == PVQ_NOTE_BF16 ? kernels_of<PVQ_NOTE_BF16>() : kernels_of<PVQ_NOTE_F16>();
    NmhArgs a{};
    a.tiles = d_tiles;
    a.rows = d_rows;
    a.stride_frames = stride_frames;
    a.n_bins = d.n_bins;
    a.t_frames = d.t_frames;
    a.o_pool = d.o_pool;
    // the features, once per row
    a.db = d_db;
    a.conv = c.conv;
    a.h_out = c.ws + w.feat_at;
    a.k_pad = w.kf_pad;
    a.p_blocks = (w.kf_pad / NM_CH + 63) / 64;
    hipLaunchKernelGGL(kern.features, dim3(nt * NM_BM * a.p_blocks), dim3(64), 0, stream, a);
    // fc1
    a.x_in = c.ws + w.feat_at;
    a.w_packed = static_cast<const u32x4*>(c.w[0]);
    a.bias = c.bias[0];
    a.h_out = c.ws + w.h_at[0];
    a.n = d.mlp;
    a.n_pad = w.mlp_pad;
    a.n_ct = (d.mlp + NM_BN - 1) / NM_BN;
    hipLaunchKernelGGL(kern.hidden, dim3(nt * a.n_ct), dim3(NMH_THREADS), 0, stream, a);
    int cur = 0;
    a.k_pad = w.mlp_pad;
    for (uint32_t i = 1; i <= d.layers; ++i) {
        a.x_in = c.ws + w.h_at[cur];
        a.h_out = c.ws + w.h_at[cur ^ 1];
        a.w_packed = static_cast<const u32x4*>(c.w[i]);
        a.bias = c.bias[i];
        hipLaunchKernelGGL(kern.hidden, dim3(nt * a.n_ct), dim3(NMH_THREADS), 0, stream, a);
        cur ^= 1;
    }
    a.x_in = c.ws + w.h_at[cur];
    a.h_out = nullptr;
    a.w_packed = static_cast<const u32x4*>(c.w[d.layers + 1]);
    a.bias = c.bias[d.layers + 1];
    a.n = a.n_pad = NM_OUT;
    a.n_ct = NM_OUT / NM_BN;
    a.prob = outs.d_prob;
    a.logits = outs.d_logits;
    a.mask = outs.d_mask;
    hipLaunchKernelGGL(kern.output, dim3(nt * a.n_ct), dim3(NMH_THREADS), 0, stream, a);
}

}  // namespace pvq
