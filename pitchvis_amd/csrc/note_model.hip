// note_model.hip — see note_model.hpp.
//
// Both kernels are one GEMM shape.  A workgroup of 4 waves owns a tile of NM_BM = 128 rows x NM_BN = 64 columns; wave w owns rows
// 32 w .. 32 w + 31 (two 16-row MFMA tiles) and ALL 64 columns (four 16-column strips): 8 accumulator tiles, 32 registers.  K is
// walked in stages of NM_PC = 4 chunks of 16: the stage's B operand (16 KiB, host-packed so that lane l's float4 of strip s holds the
// operands of the chunk's four v_mfma_f32_16x16x4_f32) is copied global -> registers -> LDS one stage ahead, double buffered, one
// barrier per stage; 32 KiB of LDS, two workgroups per CU.  The A operand never touches LDS: lane l (row l & 15, k group g = l >> 4)
// holds k = 4 g .. 4 g + 3 of the chunk as one float4,
//   nm_conv_fc1: computed — the chunk is pooled position p, k = channel, so the lane evaluates channels 4 g .. 4 g + 3 of
//                max(conv[2 p], conv[2 p + 1], 0) from x[4 p .. 4 p + 6] of its row's window, which it keeps in registers (19 per
//                stage per row tile, 16 new ones fetched a stage ahead);
//   nm_dense:    one 16-byte load from the [rows][K] activation, fetched a stage ahead.
// A row's result depends on its window alone: the k order, the accumulator it meets and the instruction sequence are the same
// wherever the row sits (tile, wave, lane, chunk of the call), so equal windows give equal bits.
#include "note_model.hpp"

#include <algorithm>
#include <string>

#include "note_carry.hpp"
#include "note_device.hpp"
#include "note_model_half.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int NM_THREADS = 256;
constexpr int CHUNK_F4 = NM_BN * NM_KC / 4;    // float4 of one chunk of the packed B operand (4 strips x 64 lanes)
constexpr int STAGE_F4 = NM_PC * CHUNK_F4;     // ... of one stage
constexpr int STAGE_LD = STAGE_F4 / NM_THREADS;   // float4 per thread per stage
constexpr int X_STAGE = 4 * NM_PC;             // new window values per stage and row
constexpr int X_REGS = X_STAGE + 3;            // positions 4 p0 .. 4 p0 + 4 NM_PC + 2
static_assert(STAGE_F4 % NM_THREADS == 0, "the stage copy is whole float4 per thread");
static_assert(sizeof(NmTile) == 16, "NmTile is read as laid out in note_model_plan.hpp");

struct NmArgs {
    const NmTile* tiles;     // this launch's tiles
    const NmRow* rows;       // null: a tile is n_valid frames of one stream from f0.  Else the launch's row table, entry 128 * tile_local + r:
                             //   row r's window and output row (note_carry.hip; the tile's stream and f0 are unread)
    const float* db;         // nm_conv_fc1: [n_streams][stride_frames][n_bins]
    const float* conv;       // nm_conv_fc1: conv weights [16][5], bias [16]
    const float* a_in;       // nm_dense: [tiles * 128][k]
    const float4* b_packed;  // [column tiles][stages * NM_PC chunks][CHUNK_F4]
    const float* bias;       // [n]
    float* h_out;            // ACT 0: [tiles * 128][n]
    float* prob;             // ACT 1: [n_streams][stride_frames][128], may be null
    float* logits;           //        the same
    uint32_t* mask;          //        [n_streams][stride_frames][4], may be null
    size_t stride_frames;
    uint32_t n_bins, t_frames, L;
    uint32_t chunks;         // K / 16: pooled positions (nm_conv_fc1), k / 16 (nm_dense)
    uint32_t k, n;           // nm_dense: row length of a_in; columns of the product
    uint32_t n_ct;           // column tiles
};

__device__ __forceinline__ void stage_fetch(const float4* __restrict__ src4, f32x4 (&r)[STAGE_LD]) {
    const f32x4* src = reinterpret_cast<const f32x4*>(src4);
#pragma unroll
    for (int j = 0; j < STAGE_LD; ++j) r[j] = src[threadIdx.x + NM_THREADS * j];
}
__device__ __forceinline__ void stage_put(float4* dst4, const f32x4 (&r)[STAGE_LD]) {
    f32x4* dst = reinterpret_cast<f32x4*>(dst4);
#pragma unroll
    for (int j = 0; j < STAGE_LD; ++j) dst[threadIdx.x + NM_THREADS * j] = r[j];
}

// acc[t][s] += a[t] (16 rows x 16 k) * chunk (16 k x 16 columns of strip s); consecutive instructions meet different accumulators
__device__ __forceinline__ void chunk_mfma(const float4* chunk, int lane, const float4 (&a)[2], f32x4 (&acc)[2][4]) {
    float4 b[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) b[s] = chunk[s * 64 + lane];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[s].x, acc[t][s], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[s].y, acc[t][s], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[s].z, acc[t][s], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[s].w, acc[t][s], 0, 0, 0);
}

// ACT 0: ReLU(acc + bias) -> h_out.  ACT 1: logits, sigmoid and mask of the valid rows.  Accumulator layout of the 16x16 tile: lane l
// holds column l & 15, rows 4 (l >> 4) + reg.
template <int ACT>
__device__ __forceinline__ void epilogue(const NmArgs& a, const NmTile tile, uint32_t tile_local, uint32_t ct, int wave, int lane,
                                         const f32x4 (&acc)[2][4]) {
    const int g = lane >> 4, c = lane & 15;
    float bias[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t col = NM_BN * ct + 16 * s + c;
        bias[s] = col < a.n ? a.bias[col] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const uint32_t r = 32 * wave + 16 * t + 4 * g + reg;   // row of the tile
            if constexpr (ACT == 0) {
                float* dst = a.h_out + (static_cast<size_t>(tile_local) * NM_BM + r) * a.n;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const uint32_t col = NM_BN * ct + 16 * s + c;
                    if (col < a.n) dst[col] = fmaxf(acc[t][s][reg] + bias[s], 0.0f);
                }
            } else {
                float logit[4];
                unsigned long long bal[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    logit[s] = acc[t][s][reg] + bias[s];
                    bal[s] = __ballot(logit[s] > 0.0f);   // bits 16 g' .. 16 g' + 15: row 4 g' + reg, the strip's 16 columns
                }
                if (r < tile.n_valid) {
                    const size_t row = a.rows ? a.rows[static_cast<size_t>(tile_local) * NM_BM + r].out_row
                                              : static_cast<size_t>(tile.stream) * a.stride_frames + tile.f0 + r;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const size_t at = row * NM_OUT + NM_BN * ct + 16 * s + c;
                        if (a.logits) a.logits[at] = logit[s];
                        if (a.prob) a.prob[at] = 1.0f / (1.0f + expf(-logit[s]));
                    }
                    if (a.mask && c < 2) {   // lane c of the row's group writes word c of this column tile's two
                        const unsigned long long lo = c == 0 ? bal[0] : bal[2], hi = c == 0 ? bal[1] : bal[3];
                        a.mask[row * 4 + 2 * ct + c] = (static_cast<uint32_t>(lo >> (16 * g)) & 0xffffu) | ((static_cast<uint32_t>(hi >> (16 * g)) & 0xffffu) << 16);
                    }
                }
            }
        }
}

// conv + ReLU + pool as the A operand of fc1 (train.py:89-92): out = ReLU(features * fc1.weight^T + fc1.bias) -> h_out
__global__ __launch_bounds__(NM_THREADS, 2) void nm_conv_fc1(const NmArgs a) {
    __shared__ float4 s_b[2][STAGE_F4];
    const uint32_t ct = blockIdx.x % a.n_ct, tile_local = blockIdx.x / a.n_ct;
    const NmTile tile = a.tiles[tile_local];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const bool active = static_cast<uint32_t>(32 * wave) < tile.n_valid;   // wave-uniform: a wave with no valid row only copies B
    const uint32_t stages = (a.chunks + NM_PC - 1) / NM_PC;
    const float4* bsrc = a.b_packed + static_cast<size_t>(ct) * stages * STAGE_F4;

    // this lane's four channels
    float w[4][NM_KW], cb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int j = 0; j < NM_KW; ++j) w[c][j] = a.conv[(4 * g + c) * NM_KW + j];
        cb[c] = a.conv[NM_CH * NM_KW + 4 * g + c];
    }
    // the windows of this lane's two rows; a row past the tile's last valid one reads the tile's first row (its result is not stored)
    const float* xrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        uint32_t r = 32 * wave + 16 * t + (lane & 15);
        if (r >= tile.n_valid) r = 0;
        xrow[t] = a.rows ? a.rows[static_cast<size_t>(tile_local) * NM_BM + r].x   // (uniform choice)
                         : a.db + (static_cast<size_t>(tile.stream) * a.stride_frames + tile.f0 + r - (a.t_frames - 1)) * a.n_bins;
    }
    const uint32_t last = a.L - 1;   // every position a real chunk reads is <= last; the clamp serves the padded chunks of the last stage
    float x[2][X_REGS], xn[2][X_STAGE];
    f32x4 breg[STAGE_LD];
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t][s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    stage_fetch(bsrc, breg);
    if (active) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < X_REGS; ++j) x[t][j] = xrow[t][min(static_cast<uint32_t>(j), last)];
    }
    stage_put(s_b[0], breg);
    __syncthreads();

    for (uint32_t st = 0; st < stages; ++st) {
        const bool more = st + 1 < stages;
        if (more) {
            stage_fetch(bsrc + static_cast<size_t>(st + 1) * STAGE_F4, breg);
            if (active) {
                const uint32_t at = X_STAGE * (st + 1) + 3;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < X_STAGE; ++j) xn[t][j] = xrow[t][min(at + j, last)];
            }
        }
        if (active) {
            const float4* sb = s_b[st & 1];
#pragma unroll
            for (int i = 0; i < NM_PC; ++i) {
                if (NM_PC * st + i < a.chunks) {   // (uniform) the padded chunks of the last stage are skipped
                    float4 av[2];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        float v[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            float e = cb[c], o = cb[c];   // conv positions 2 p and 2 p + 1
#pragma unroll
                            for (int j = 0; j < NM_KW; ++j) {
                                e = fmaf(w[c][j], x[t][4 * i + j], e);
                                o = fmaf(w[c][j], x[t][4 * i + 2 + j], o);
                            }
                            v[c] = fmaxf(fmaxf(e, o), 0.0f);
                        }
                        av[t] = make_float4(v[0], v[1], v[2], v[3]);
                    }
                    chunk_mfma(sb + i * CHUNK_F4, lane, av, acc);
                }
            }
            if (more) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) x[t][j] = x[t][X_STAGE + j];
#pragma unroll
                    for (int j = 0; j < X_STAGE; ++j) x[t][3 + j] = xn[t][j];
                }
            }
        }
        if (more) stage_put(s_b[(st + 1) & 1], breg);
        __syncthreads();
    }
    if (active) epilogue<0>(a, tile, tile_local, ct, wave, lane, acc);
}

// out = a_in * W^T + bias: ACT 0 -> ReLU -> h_out (train.py:93-95); ACT 1 -> logits, sigmoid, mask (train.py:96-98, ml_system.rs:56-65)
template <int ACT>
__global__ __launch_bounds__(NM_THREADS, 2) void nm_dense(const NmArgs a) {
    __shared__ float4 s_b[2][STAGE_F4];
    const uint32_t ct = blockIdx.x % a.n_ct, tile_local = blockIdx.x / a.n_ct;
    const NmTile tile = a.tiles[tile_local];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const bool active = static_cast<uint32_t>(32 * wave) < tile.n_valid;
    const uint32_t stages = (a.chunks + NM_PC - 1) / NM_PC;
    const float4* bsrc = a.b_packed + static_cast<size_t>(ct) * stages * STAGE_F4;
    // rows of the activation buffer: every row of an active wave was written by the previous layer
    const float4* arow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
        arow[t] = reinterpret_cast<const float4*>(a.a_in + (static_cast<size_t>(tile_local) * NM_BM + 32 * wave + 16 * t + (lane & 15)) * a.k) + g;
    float4 av[NM_PC][2], an[NM_PC][2];
    f32x4 breg[STAGE_LD];
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t][s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    stage_fetch(bsrc, breg);
    if (active) {
#pragma unroll
        for (int i = 0; i < NM_PC; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t) av[i][t] = static_cast<uint32_t>(i) < a.chunks ? arow[t][4 * i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    stage_put(s_b[0], breg);
    __syncthreads();

    for (uint32_t st = 0; st < stages; ++st) {
        const bool more = st + 1 < stages;
        if (more) {
            stage_fetch(bsrc + static_cast<size_t>(st + 1) * STAGE_F4, breg);
            if (active) {
#pragma unroll
                for (int i = 0; i < NM_PC; ++i) {
                    const uint32_t kc = NM_PC * (st + 1) + i;   // (a chunk past the row's end is not read)
#pragma unroll
                    for (int t = 0; t < 2; ++t) an[i][t] = kc < a.chunks ? arow[t][4 * kc] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
        }
        if (active) {
            const float4* sb = s_b[st & 1];
#pragma unroll
            for (int i = 0; i < NM_PC; ++i)
                if (NM_PC * st + i < a.chunks) chunk_mfma(sb + i * CHUNK_F4, lane, av[i], acc);
            if (more) {
#pragma unroll
                for (int i = 0; i < NM_PC; ++i)
#pragma unroll
                    for (int t = 0; t < 2; ++t) av[i][t] = an[i][t];
            }
        }
        if (more) stage_put(s_b[(st + 1) & 1], breg);
        __syncthreads();
    }
    if (active) epilogue<ACT>(a, tile, tile_local, ct, wave, lane, acc);
}

// the f32 launches of the tiles d_tiles[0 .. nt): fc1 over the fused conv, the hidden layers, the output layer into `outs`
void nm_chunk(const NmContext& c, const NmTile* d_tiles, const NmRow* d_rows, uint32_t nt, const float* d_db, size_t stride_frames,
              const pvq_note_model_outputs& outs, hipStream_t stream) {
    const NoteModelDims& d = c.d;
    float* buf[2] = {reinterpret_cast<float*>(c.ws + c.at.h_at[0]), reinterpret_cast<float*>(c.ws + c.at.h_at[1])};
    NmArgs a{};
    a.tiles = d_tiles;
    a.rows = d_rows;
    a.stride_frames = stride_frames;
    a.n_bins = d.n_bins;
    a.t_frames = d.t_frames;
    a.L = d.L;
    // fc1 over the fused conv
    a.db = d_db;
    a.conv = c.conv;
    a.b_packed = static_cast<const float4*>(c.w[0]);
    a.bias = c.bias[0];
    a.h_out = buf[0];
    a.chunks = d.o_pool;
    a.k = d.n_features;
    a.n = d.mlp;
    a.n_ct = (d.mlp + NM_BN - 1) / NM_BN;
    hipLaunchKernelGGL(nm_conv_fc1, dim3(nt * a.n_ct), dim3(NM_THREADS), 0, stream, a);
    int cur = 0;
    a.chunks = d.mlp / NM_KC;
    a.k = d.mlp;
    for (uint32_t i = 1; i <= d.layers; ++i) {
        a.a_in = buf[cur];
        a.h_out = buf[cur ^ 1];
        a.b_packed = static_cast<const float4*>(c.w[i]);
        a.bias = c.bias[i];
        hipLaunchKernelGGL(nm_dense<0>, dim3(nt * a.n_ct), dim3(NM_THREADS), 0, stream, a);
        cur ^= 1;
    }
    a.a_in = buf[cur];
    a.h_out = nullptr;
    a.b_packed = static_cast<const float4*>(c.w[d.layers + 1]);
    a.bias = c.bias[d.layers + 1];
    a.n = NM_OUT;
    a.n_ct = NM_OUT / NM_BN;
    a.prob = outs.d_prob;
    a.logits = outs.d_logits;
    a.mask = outs.d_mask;
    hipLaunchKernelGGL(nm_dense<1>, dim3(nt * a.n_ct), dim3(NM_THREADS), 0, stream, a);
}
}  // namespace

NoteModel::~NoteModel() {
    if (device_id_ >= 0) (void)hipSetDevice(device_id_);   // the buffers go after this body, with their device set
}

// a dense layer as its precision's kernel reads it (note_model_pack_b, note_model_pack_b16), then its f32 bias
pvq_status NoteModel::upload(const float* W, const float* bias, uint32_t n, uint32_t k, bool conv_order, Layer& l) {
    std::vector<float> p32;
    std::vector<uint16_t> p16;
    const void* packed;
    if (host_.precision == PVQ_NOTE_F32) {
        p32 = note_model_pack_b(W, n, k, conv_order, host_.d.o_pool);
        packed = p32.data();
        l.bias_at = p32.size() * sizeof(float);
    } else {
        p16 = note_model_pack_b16(W, n, k, conv_order, host_.d.o_pool, host_.precision);
        packed = p16.data();
        l.bias_at = p16.size() * sizeof(uint16_t);
    }
    // (whole chunks of 4 KiB: the bias is 16-byte aligned)
    if (pvq_status s = l.buf.reserve(l.bias_at + n * sizeof(float))) return s;
    PVQ_HIP(hipMemcpy(l.buf.as<char>(), packed, l.bias_at, hipMemcpyHostToDevice));
    PVQ_HIP(hipMemcpy(l.buf.as<char>() + l.bias_at, bias, n * sizeof(float), hipMemcpyHostToDevice));
    return PVQ_OK;
}

pvq_status NoteModel::create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                             pvq_note_precision precision, std::unique_ptr<NoteModel>& out) {
    out.reset();
    NoteModelDims d;
    std::string err;
    pvq_status st = note_model_check(params, weights, d, err);
    if (st == PVQ_OK) st = note_model_check_range(d, *weights, precision, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    std::unique_ptr<NoteModel> m(new NoteModel());
    m->device_id_ = device_id < 0 ? -1 : device_id;
    m->host_.assign(d, *weights, precision);
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        const NoteModelHost& h = m->host_;
        std::vector<float> conv(h.conv_w);
        conv.insert(conv.end(), h.conv_b.begin(), h.conv_b.end());
        pvq_status s = m->conv_.upload(conv.data(), NOTE_CONV_VALUES * sizeof(float));
        if (s == PVQ_OK) s = m->upload(h.fc1_w.data(), h.fc1_b.data(), d.mlp, d.n_features, true, m->fc1_);
        m->layer_ = std::vector<Layer>(d.layers);
        for (uint32_t i = 0; s == PVQ_OK && i < d.layers; ++i) s = m->upload(h.layer_w[i].data(), h.layer_b[i].data(), d.mlp, d.mlp, false, m->layer_[i]);
        if (s == PVQ_OK) s = m->upload(h.out_w.data(), h.out_b.data(), NM_OUT, d.mlp, false, m->out_);
        if (s != PVQ_OK) return s;
    }
    out = std::move(m);
    return PVQ_OK;
}

// the argument checks of both row calls, before any device is touched
pvq_status NoteModel::check_rows(const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                                 const pvq_note_model_outputs& outs) const {
    const bool half = host_.precision != PVQ_NOTE_F32;
    if (!d_db) {
        set_last_error("note model: d_db is null");
        return PVQ_ERR_INVALID_ARG;
    }
    if (reinterpret_cast<uintptr_t>(outs.d_mask) & 3) {
        set_last_error("note model: d_mask must be 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if (half && ((reinterpret_cast<uintptr_t>(outs.d_prob) | reinterpret_cast<uintptr_t>(outs.d_logits)) & 15)) {   // nmh_dense stores float4
        set_last_error("note model: d_prob and d_logits of a 16-bit handle must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if (stride_frames > 0x7fffffffull || (n_streams && stride_frames > (~0ull >> 12) / n_streams)) {
        set_last_error("note model: too many frames in one call");
        return PVQ_ERR_INVALID_ARG;
    }
    for (uint32_t s = 0; n_frames && s < n_streams; ++s)
        if (n_frames[s] > stride_frames) {
            set_last_error("note model: n_frames of stream " + std::to_string(s) + " exceeds stride_frames");
            return PVQ_ERR_INVALID_ARG;
        }
    return PVQ_OK;
}

// every row of every output is zero before the model rows are written
pvq_status NoteModel::zero_outputs(size_t rows_all, const pvq_note_model_outputs& outs, hipStream_t stream) {
    if (rows_all == 0) return PVQ_OK;
    if (outs.d_prob) PVQ_HIP(hipMemsetAsync(outs.d_prob, 0, rows_all * NM_OUT * sizeof(float), stream));
    if (outs.d_logits) PVQ_HIP(hipMemsetAsync(outs.d_logits, 0, rows_all * NM_OUT * sizeof(float), stream));
    if (outs.d_mask) PVQ_HIP(hipMemsetAsync(outs.d_mask, 0, rows_all * 4 * sizeof(uint32_t), stream));
    return PVQ_OK;
}

// the workspace for n_tiles tiles and what the launches of a chunk work on; the tile table lies at the workspace's start
pvq_status NoteModel::prepare(size_t n_tiles, NmContext& c) {
    const NoteModelDims& d = host_.d;
    c.d = d;
    c.precision = host_.precision;
    c.at = note_model_workspace(d, host_.precision, n_tiles, ws_limit_);
    if (pvq_status s = ws_.reserve(c.at.total)) return s;
    c.ws = ws_.as<char>();
    c.conv = conv_.as<float>();
    const auto put = [&c](uint32_t i, const Layer& l) {
        c.w[i] = l.buf.as<char>();
        c.bias[i] = reinterpret_cast<const float*>(l.buf.as<char>() + l.bias_at);
    };
    put(0, fc1_);
    for (uint32_t i = 0; i < d.layers; ++i) put(1 + i, layer_[i]);
    put(1 + d.layers, out_);
    return PVQ_OK;
}

// the launches of n_tiles tiles, in chunks of whole tiles that fit the workspace; d_rows: null or their row table
pvq_status NoteModel::run(const NmContext& c, size_t n_tiles, const NmRow* d_rows, const float* d_db, size_t stride_frames,
                          const pvq_note_model_outputs& outs, hipStream_t stream) {
    const NmTile* d_tiles = ws_.as<NmTile>();
    const size_t chunk_tiles = c.at.chunk_tiles;
    for (size_t t0 = 0; t0 < n_tiles; t0 += chunk_tiles) {
        const uint32_t nt = static_cast<uint32_t>(std::min(chunk_tiles, n_tiles - t0));
        const NmRow* rows = d_rows ? d_rows + t0 * NM_BM : nullptr;
        if (host_.precision != PVQ_NOTE_F32) nmh_chunk(c, d_tiles + t0, rows, nt, d_db, stride_frames, outs, stream);
        else nm_chunk(c, d_tiles + t0, rows, nt, d_db, stride_frames, outs, stream);
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status NoteModel::rows_device(const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                                  const pvq_note_model_outputs& outs, hipStream_t stream) {
    const NoteModelDims& d = host_.d;
    if (pvq_status s = check_rows(d_db, n_frames, n_streams, stride_frames, outs)) return s;
    if (device_id_ < 0) {
        set_last_error("the batched note model runs on a GPU; this handle has none (pvq_note_model_infer is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    const size_t rows_all = static_cast<size_t>(n_streams) * stride_frames;
    if (rows_all == 0 || !(outs.d_prob || outs.d_logits || outs.d_mask)) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    // every row that is no model row is zero; the model rows are overwritten below
    if (pvq_status s = zero_outputs(rows_all, outs, stream)) return s;
    const std::vector<NmTile> tiles = note_model_tiles(d, n_frames, n_streams, stride_frames);
    if (tiles.empty()) return PVQ_OK;

    NmContext c;
    if (pvq_status s = prepare(tiles.size(), c)) return s;
    NmTile* d_tiles = ws_.as<NmTile>();
    PVQ_HIP(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(NmTile), hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns)
    return run(c, tiles.size(), nullptr, d_db, stride_frames, outs, stream);
}

pvq_status NoteModel::rows_carry_device(NoteCarry& carry, const float* d_db, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                                        const pvq_note_model_outputs& outs, hipStream_t stream) {
    const NoteModelDims& d = host_.d;
    if (pvq_status s = check_rows(d_db, n_frames, n_streams, stride_frames, outs)) return s;
    if (!carry.fits(d, device_id_) || carry.n_streams() != n_streams) {
        set_last_error("note carry: made for another n_streams, or for a model of other sizes or on another device");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched note model runs on a GPU; this handle has none (pvq_note_model_infer is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (pvq_status s = carry.plan(d, n_frames, stride_frames)) return s;
    const NcPlan& plan = carry.planned();
    PVQ_HIP(hipSetDevice(device_id_));
    if (pvq_status s = zero_outputs(static_cast<size_t>(n_streams) * stride_frames, outs, stream)) return s;
    if (plan.max_n == 0) return PVQ_OK;   // no stream gets a frame
    const size_t n_tiles = static_cast<size_t>(plan.tiles);
    NmContext c;
    if (pvq_status s = prepare(std::max<size_t>(1, n_tiles), c)) return s;   // (the tile list nc_rows writes lies in the workspace)
    // every frame a row needs is copied or read by the kernels queued here: the caller may overwrite d_db in stream order behind them
    if (pvq_status s = carry.stage(d_db, stride_frames, ws_.as<NmTile>(), stream)) return s;
    if (n_tiles && (outs.d_prob || outs.d_logits || outs.d_mask))   // (without an output the frames are still taken in)
        if (pvq_status s = run(c, n_tiles, carry.rows(), d_db, stride_frames, outs, stream)) return s;
    return carry.commit(d_db, stride_frames, stream);
}

}  // namespace pvq
