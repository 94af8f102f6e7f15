// note_trainer_half.hip — see note_trainer_half.hpp.
//
// nth_gemm: C = A B^T with A [M][K] and B [N][K] in bf16, K a multiple of 32 whose padding holds zeros.  A workgroup of 4 waves owns
// 64 rows x 64 columns, wave w the quadrant of rows 32 (w >> 1) .. and columns 32 (w & 1) ..: 2 x 2 accumulator tiles, 16 registers, and
// per chunk of 32 k two 16-byte LDS reads of A and two of B for four MFMAs (nt_gemm's 16 x 64 strip would read five).  K is walked in
// stages of NTH_BK = 64; both operands go global -> registers -> LDS one stage ahead, double buffered, one barrier per stage, 16 bytes
// per thread and piece, never transposed.  An operand lies in LDS as [row][8 pieces of 16 bytes] with piece p of row r at slot
// p ^ ((r >> 1) & 7): rows are 128 bytes, two to a 256-byte bank row, and the XOR puts the 16 lanes of every ds_read_b128 lane group
// (rows 0-3 and 12-15 of one k group with rows 4-11 of its neighbour) on 16 different slots; the 8 lanes of a ds_write_b128 group
// write one whole row.  Lane l (c = l & 15, g = l >> 4) reads k = 8 g .. 8 g + 7 of a chunk as the operand of one MFMA, for A and B alike.
//
// The accumulator layout (lane: column c, rows 4 g + reg) gives a lane four consecutive rows of one column, so the [col][row] copy of a
// 16-bit result is one 8-byte store per lane and tile, no LDS; the [row][col] copy is a 2-byte store per element, 32 bytes per 16 lanes.
// Rows M .. pad32(M) - 1 of the [col][row] copy and columns N .. pad32(N) - 1 of the [row][col] copy are written as zeros: they are
// the K padding of the products that read them.
//
// Order of every sum is fixed by the shapes alone, as in note_trainer.hip: equal inputs give equal bits.
#include "note_trainer_half.hpp"

#include <algorithm>

#include "note_device.hpp"

namespace pvq {

namespace {
using bf16 = __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

constexpr int NTH_THREADS = 256;
constexpr int NTH_PIECES = NTH_BK / 8;               // 16-byte pieces of an operand row per stage
constexpr int NTH_LD = NTH_BM * NTH_PIECES / NTH_THREADS;   // pieces per thread, operand and stage
constexpr int NTH_MAX_JOBS = 10;                     // dense weights of a model: fc1, up to 8 hidden layers, output
static_assert(NTH_BM == NTH_BN && NTH_BM * NTH_PIECES % NTH_THREADS == 0 && NTH_PIECES == 8, "the stage copy and the slot XOR");

using NthEpi = NoteEpi<bf16>;   // the gate is the stored 16-bit activation [M][ldg]

struct NthGemm {
    const bf16* A;   // [M][K]
    const bf16* B;   // [N][K]
    float* part;     // splits > 1: the partial sums [splits][M][N]
    float* C32;      // E_RAW, E_BIAS: [M][N]
    bf16* C16;       // E_HIDDEN, E_GATE: [M][ld16], ld16 = pad32(N)
    bf16* CT;        //   and [N][ldt], ldt = pad32(M); may be null
    uint32_t ld16, ldt;
    uint32_t M, N, K;
    uint32_t n_ct;
    uint32_t stages, stages_per_split, splits;
    NthEpi e;
};

// rows r0 .. r0 + 3 (r0 a multiple of 4) of column col: the epilogue, then every copy the product keeps
__device__ __forceinline__ void store4(const NthGemm& a, const f32x4 v, uint32_t r0, uint32_t col) {
    float o[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) o[reg] = (r0 + reg < a.M && col < a.N) ? epi_apply(a.e, v[reg], r0 + reg, col) : 0.0f;
    if (a.C32) {
        if (col < a.N) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (r0 + reg < a.M) a.C32[static_cast<size_t>(r0 + reg) * a.N + col] = o[reg];
        }
        return;
    }
    bf16x4 q;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) q[reg] = static_cast<bf16>(o[reg]);
    if (col < a.ld16) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (r0 + reg < a.M) a.C16[static_cast<size_t>(r0 + reg) * a.ld16 + col] = q[reg];
    }
    if (a.CT && col < a.N && r0 < a.ldt) *reinterpret_cast<bf16x4*>(a.CT + static_cast<size_t>(col) * a.ldt + r0) = q;   // (ldt is a multiple of 4)
}

// tile rows r0 .. r0 + 63 (bound R), k0 .. k0 + 63 (bound K, a multiple of 32) of src [R][K] -> NTH_LD 16-byte pieces per thread
__device__ __forceinline__ void fetch(const bf16* __restrict__ src, uint32_t R, uint32_t r0, uint32_t K, uint32_t k0, u32x4 (&r)[NTH_LD]) {
#pragma unroll
    for (int j = 0; j < NTH_LD; ++j) {
        const uint32_t f = threadIdx.x + NTH_THREADS * j;
        const uint32_t row = r0 + f / NTH_PIECES, k = k0 + 8 * (f % NTH_PIECES);
        r[j] = (row < R && k < K) ? *reinterpret_cast<const u32x4*>(src + static_cast<size_t>(row) * K + k) : u32x4{0u, 0u, 0u, 0u};
    }
}
__device__ __forceinline__ uint32_t slot(uint32_t row, uint32_t piece) { return row * NTH_PIECES + (piece ^ ((row >> 1) & 7u)); }
__device__ __forceinline__ void put(u32x4* dst, const u32x4 (&r)[NTH_LD]) {
#pragma unroll
    for (int j = 0; j < NTH_LD; ++j) {
        const uint32_t f = threadIdx.x + NTH_THREADS * j;
        dst[slot(f / NTH_PIECES, f % NTH_PIECES)] = r[j];
    }
}

__global__ __launch_bounds__(NTH_THREADS, 2) void nth_gemm(const NthGemm a) {
    __shared__ u32x4 s_a[2][NTH_BM * NTH_PIECES];
    __shared__ u32x4 s_b[2][NTH_BN * NTH_PIECES];
    const uint32_t ct = blockIdx.x % a.n_ct, rt = blockIdx.x / a.n_ct, z = blockIdx.y;
    const uint32_t m0 = NTH_BM * rt, n0 = NTH_BN * ct;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const uint32_t wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const uint32_t st0 = z * a.stages_per_split, st1 = min(st0 + a.stages_per_split, a.stages);

    u32x4 ra[NTH_LD], rb[NTH_LD];
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc[t][s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (st0 < st1) {
        fetch(a.A, a.M, m0, a.K, NTH_BK * st0, ra);
        fetch(a.B, a.N, n0, a.K, NTH_BK * st0, rb);
        put(s_a[0], ra);
        put(s_b[0], rb);
    }
    __syncthreads();
    for (uint32_t st = st0; st < st1; ++st) {
        const int cur = (st - st0) & 1;
        const bool more = st + 1 < st1;
        if (more) {
            fetch(a.A, a.M, m0, a.K, NTH_BK * (st + 1), ra);
            fetch(a.B, a.N, n0, a.K, NTH_BK * (st + 1), rb);
        }
#pragma unroll
        for (uint32_t ch = 0; ch < NTH_BK / 32; ++ch) {
            if (NTH_BK * st + 32 * ch >= a.K) break;   // (uniform) the half stage past a K of an odd number of chunks
            bf16x8 av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) av[t] = __builtin_bit_cast(bf16x8, s_a[cur][slot(wr + 16 * t + c, 4 * ch + g)]);
#pragma unroll
            for (int s = 0; s < 2; ++s) bv[s] = __builtin_bit_cast(bf16x8, s_b[cur][slot(wc + 16 * s + c, 4 * ch + g)]);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[t], bv[s], acc[t][s], 0, 0, 0);
        }
        if (more) {
            put(s_a[cur ^ 1], ra);
            put(s_b[cur ^ 1], rb);
        }
        __syncthreads();
    }

    // accumulator layout of a 16 x 16 tile: lane l holds column l & 15, rows 4 (l >> 4) + reg
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t r0 = m0 + wr + 16 * t + 4 * g, col = n0 + wc + 16 * s + c;
            if (a.splits > 1) {
                float* dst = a.part + static_cast<size_t>(z) * a.M * a.N;
                if (col < a.N) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg)
                        if (r0 + reg < a.M) dst[static_cast<size_t>(r0 + reg) * a.N + col] = acc[t][s][reg];
                }
            } else {
                store4(a, acc[t][s], r0, col);
            }
        }
}

// the partial sums added in split order, then the epilogue and the stores of an unsplit product.  Block (x: 16 columns, y: 64 rows),
// thread (column tid & 15, rows 16 (tid >> 6) + 4 ((tid >> 4) & 3) ..): nth_gemm's lane layout, over pad32(M) x pad32(N)
__global__ __launch_bounds__(NTH_THREADS) void nth_gemm_finish(const NthGemm a) {
    const uint32_t col = 16 * blockIdx.x + (threadIdx.x & 15);
    const uint32_t r0 = 64 * blockIdx.y + 16 * (threadIdx.x >> 6) + 4 * ((threadIdx.x >> 4) & 3);
    const size_t mn = static_cast<size_t>(a.M) * a.N;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (col < a.N) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            if (r0 + reg >= a.M) continue;
            const size_t i = static_cast<size_t>(r0 + reg) * a.N + col;
            float s = a.part[i];
            for (uint32_t z = 1; z < a.splits; ++z) s += a.part[z * mn + i];
            v[reg] = s;
        }
    }
    store4(a, v, r0, col);
}

// nt_features (note_trainer.hip) with each pooled feature rounded once: feat [batch][f_pad], columns F .. f_pad - 1 zeros
__global__ __launch_bounds__(NTH_THREADS) void nth_features(const float* __restrict__ db, const uint32_t* __restrict__ idx, const float* __restrict__ conv,
                                                            bf16* __restrict__ feat, uint32_t n_bins, uint32_t t_frames, uint32_t L, uint32_t o_pool, uint32_t f_pad) {
    extern __shared__ float s_x[];   // the window, L floats
    __shared__ float s_w[NOTE_CONV_VALUES];
    const uint32_t b = blockIdx.x;
    const float* x = db + (static_cast<size_t>(idx[b]) - (t_frames - 1)) * n_bins;
    for (uint32_t i = threadIdx.x; i < L; i += NTH_THREADS) s_x[i] = x[i];
    if (threadIdx.x < NOTE_CONV_VALUES) s_w[threadIdx.x] = conv[threadIdx.x];
    __syncthreads();
    const uint32_t F = NM_CH * o_pool;
    bf16* dst = feat + static_cast<size_t>(b) * f_pad;
    for (uint32_t i = threadIdx.x; i < f_pad; i += NTH_THREADS) {
        float v = 0.0f;
        if (i < F) {
            const uint32_t ch = i / o_pool, p = i - ch * o_pool;
            float e, o;
            conv_pair(s_w + ch * NM_KW, s_w[NM_CH * NM_KW + ch], s_x + 4 * p, e, o);   // reads x[4 p .. 4 p + 6] <= x[L - 1]
            v = fmaxf(fmaxf(e, o), 0.0f);
        }
        dst[i] = static_cast<bf16>(v);
    }
}

// src [R][C] (row length lds; f32, rounded here, or bf16) -> dst [R][pad32(C)] and dstt [C][pad32(R)], the padding zeros; either may be null
struct NthJob {
    const void* src;
    bf16* dst;
    bf16* dstt;
    uint32_t R, C, lds;
    uint32_t src_f32;
    uint32_t tile0, tiles_c;   // first tile of the job in the launch; 64 x 64 tiles per row of tiles
};
struct NthJobs {
    NthJob job[NTH_MAX_JOBS];
    uint32_t n;
};
__global__ __launch_bounds__(NTH_THREADS) void nth_relayout(const NthJobs js) {
    __shared__ bf16 s_t[64][66];
    uint32_t k = 0;
    while (k + 1 < js.n && blockIdx.x >= js.job[k + 1].tile0) ++k;
    const NthJob& j = js.job[k];
    const uint32_t tile = blockIdx.x - j.tile0;
    const uint32_t r0 = 64 * (tile / j.tiles_c), c0 = 64 * (tile % j.tiles_c);
    const uint32_t Cp = (j.C + 31u) & ~31u, Rp = (j.R + 31u) & ~31u;
    const uint32_t x = threadIdx.x & 63, y = threadIdx.x >> 6;
    for (uint32_t i = y; i < 64; i += 4) {
        const uint32_t row = r0 + i, col = c0 + x;
        bf16 v = static_cast<bf16>(0.0f);
        if (row < j.R && col < j.C) {
            const size_t at = static_cast<size_t>(row) * j.lds + col;
            v = j.src_f32 ? static_cast<bf16>(static_cast<const float*>(j.src)[at]) : static_cast<const bf16*>(j.src)[at];
        }
        s_t[i][x] = v;
        if (j.dst && row < j.R && col < Cp) j.dst[static_cast<size_t>(row) * Cp + col] = v;
    }
    __syncthreads();
    if (!j.dstt) return;
    for (uint32_t i = y; i < 64; i += 4) {
        const uint32_t col = c0 + i, row = r0 + x;
        if (col < j.C && row < Rp) j.dstt[static_cast<size_t>(col) * Rp + row] = s_t[x][i];
    }
}

// nt_bias_grad over 16-bit rows of length ld: the same four row phases, each added in row order; eight rows of a phase are loaded
// before they are added, which changes no sum
__global__ __launch_bounds__(NTH_THREADS) void nth_bias_grad(const bf16* __restrict__ d, float* __restrict__ out, uint32_t M, uint32_t N, uint32_t ld) {
    __shared__ float s_red[4][64];
    const uint32_t col = 64 * blockIdx.x + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    float s = 0.0f;
    if (col < N) {
        const bf16* p = d + col;
        uint32_t r = ph;
        for (; r + 28 < M; r += 32) {
            bf16 v[8];
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) v[u] = p[static_cast<size_t>(r + 4 * u) * ld];
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) s += static_cast<float>(v[u]);
        }
        for (; r < M; r += 4) s += static_cast<float>(p[static_cast<size_t>(r) * ld]);
    }
    s_red[ph][threadIdx.x & 63] = s;
    __syncthreads();
    if (ph == 0 && col < N) out[col] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

// where a product leaves its result
struct NthOut {
    float* c32 = nullptr;
    bf16* c16 = nullptr;
    bf16* ct = nullptr;
};

// one product C [M][N] = A [M][K] B [N][K]^T; a split one goes through `part` and nth_gemm_finish
void gemm(const bf16* A, const bf16* B, const NthOut& out, uint32_t M, uint32_t N, uint32_t K, const NthEpi& e, float* part, hipStream_t stream) {
    NthGemm a{};
    a.A = A;
    a.B = B;
    a.part = part;
    a.C32 = out.c32;
    a.C16 = out.c16;
    a.CT = out.ct;
    a.ld16 = nth_pad32(N);
    a.ldt = nth_pad32(M);
    a.M = M;
    a.N = N;
    a.K = K;
    a.n_ct = (N + NTH_BN - 1) / NTH_BN;
    a.stages = (K + NTH_BK - 1) / NTH_BK;
    const uint32_t want = nth_splits(M, N, K);
    a.stages_per_split = (a.stages + want - 1) / want;
    a.splits = (a.stages + a.stages_per_split - 1) / a.stages_per_split;   // no empty split
    a.e = e;
    hipLaunchKernelGGL(nth_gemm, dim3(((M + NTH_BM - 1) / NTH_BM) * a.n_ct, a.splits), dim3(NTH_THREADS), 0, stream, a);
    if (a.splits > 1)
        hipLaunchKernelGGL(nth_gemm_finish, dim3(a.ld16 / 16, (a.ldt + 63) / 64), dim3(NTH_THREADS), 0, stream, a);
}

void add_job(NthJobs& js, const void* src, bool f32, bf16* dst, bf16* dstt, uint32_t R, uint32_t C, uint32_t lds) {
    NthJob& j = js.job[js.n];
    j.src = src;
    j.dst = dst;
    j.dstt = dstt;
    j.R = R;
    j.C = C;
    j.lds = lds;
    j.src_f32 = f32 ? 1u : 0u;
    j.tiles_c = (nth_pad32(C) + 63) / 64;
    j.tile0 = js.n ? js.job[js.n - 1].tile0 + js.job[js.n - 1].tiles_c * ((nth_pad32(js.job[js.n - 1].R) + 63) / 64) : 0;
    ++js.n;
}
void relayout(const NthJobs& js, hipStream_t stream) {
    const NthJob& last = js.job[js.n - 1];
    hipLaunchKernelGGL(nth_relayout, dim3(last.tile0 + last.tiles_c * ((nth_pad32(last.R) + 63) / 64)), dim3(NTH_THREADS), 0, stream, js);
}

// the buffers of a call of `batch` rows
struct Buffers {
    const NthContext& c;
    bf16* ws;
    explicit Buffers(const NthContext& ctx) : c(ctx), ws(reinterpret_cast<bf16*>(ctx.ws16)) {}
    bf16* feat() const { return ws + c.plan->feat_at; }
    bf16* featt() const { return ws + c.plan->featt_at; }
    bf16* h(uint32_t i) const { return ws + c.plan->h_at + i * c.plan->h_stride; }
    bf16* ht(uint32_t i) const { return ws + c.plan->ht_at + i * c.plan->ht_stride; }
    bf16* dz() const { return ws + c.plan->dz_at; }
    bf16* dzt() const { return ws + c.plan->dzt_at; }
    bf16* da(int i) const { return ws + c.plan->da_at + i * c.plan->h_stride; }
    bf16* dat(int i) const { return ws + c.plan->dat_at + i * c.plan->ht_stride; }
    const bf16* w(size_t layer) const { return reinterpret_cast<const bf16*>(c.shadow) + c.plan->shadow[layer].w_at; }
    const bf16* wt(size_t layer) const { return reinterpret_cast<const bf16*>(c.shadow) + c.plan->shadow[layer].wt_at; }
};
}  // namespace

void nth_refresh_shadow(const NthContext& c, hipStream_t stream) {
    NthJobs js{};
    bf16* sh = reinterpret_cast<bf16*>(c.shadow);
    for (const NthShadow& s : c.plan->shadow) add_job(js, c.arena + s.src_at, true, sh + s.w_at, sh + s.wt_at, s.n, s.k, s.k);
    relayout(js, stream);
}

void nth_forward(const NthContext& c, const float* d_db, uint32_t batch, bool train, hipStream_t stream) {
    const NoteTrainerLayout& lay = *c.lay;
    const NoteModelDims& d = lay.d;
    const Buffers b(c);
    const float* w = c.arena;
    const uint32_t Fp = c.plan->f_pad, Mp = c.plan->mlp_pad, mlp = d.mlp;
    const uint32_t threshold = nt_keep_threshold(c.hyper.dropout);
    const bool drop = train && threshold > 0;
    const float scale = drop ? static_cast<float>(1.0 / (1.0 - c.hyper.dropout)) : 1.0f;

    hipLaunchKernelGGL(nth_features, dim3(batch), dim3(NTH_THREADS), static_cast<size_t>(d.L) * sizeof(float), stream, d_db, c.d_idx, w + lay.conv_w.at, b.feat(),
                       d.n_bins, d.t_frames, d.L, d.o_pool, Fp);
    NthEpi e{};
    e.kind = E_HIDDEN;
    e.bias = w + lay.fc1_b.at;
    e.scale = 1.0f;
    NthOut out;
    out.c16 = b.h(0);
    out.ct = train ? b.ht(0) : nullptr;
    gemm(b.feat(), b.w(0), out, batch, mlp, Fp, e, c.part, stream);
    for (uint32_t i = 0; i < d.layers; ++i) {
        e.bias = w + lay.layer_b[i].at;
        e.drop = drop ? 1 : 0;
        e.scale = scale;
        e.threshold = threshold;
        e.key = nt_layer_key(c.hyper.seed, c.steps, i);
        out.c16 = b.h(i + 1);
        out.ct = train ? b.ht(i + 1) : nullptr;
        gemm(b.h(i), b.w(1 + i), out, batch, mlp, Mp, e, c.part, stream);
    }
    e = NthEpi{};
    e.kind = E_BIAS;
    e.bias = w + lay.out_b.at;
    out = NthOut{};
    out.c32 = c.Z;
    gemm(b.h(d.layers), b.w(1 + d.layers), out, batch, NM_OUT, Mp, e, c.part, stream);
}

void nth_backward(const NthContext& c, uint32_t batch, hipStream_t stream) {
    const NoteTrainerLayout& lay = *c.lay;
    const NoteModelDims& d = lay.d;
    const Buffers b(c);
    float* grad = c.arena + lay.n_params;
    const uint32_t F = d.n_features, Fp = c.plan->f_pad, Mp = c.plan->mlp_pad, mlp = d.mlp, Bp = nth_pad32(batch);
    const bool drop = nt_keep_threshold(c.hyper.dropout) > 0;
    const float scale = drop ? static_cast<float>(1.0 / (1.0 - c.hyper.dropout)) : 1.0f;
    auto bias_grad = [&](const bf16* dz, float* out, uint32_t n, uint32_t ld) {
        hipLaunchKernelGGL(nth_bias_grad, dim3((n + 63) / 64), dim3(NTH_THREADS), 0, stream, dz, out, batch, n, ld);
    };

    // the output layer's dZ rounded once, both ways round; the features the other way round
    NthJobs js{};
    add_job(js, c.dZ, true, b.dz(), b.dzt(), batch, NM_OUT, NM_OUT);
    add_job(js, b.feat(), false, nullptr, b.featt(), batch, F, Fp);
    relayout(js, stream);

    NthEpi raw{};
    raw.kind = E_RAW;
    NthEpi gate{};
    gate.kind = E_GATE;
    gate.ldg = Mp;
    NthOut out;
    out.c32 = grad + lay.out_w.at;
    gemm(b.dzt(), b.ht(d.layers), out, NM_OUT, mlp, Bp, raw, c.part, stream);
    bias_grad(b.dz(), grad + lay.out_b.at, NM_OUT, NM_OUT);
    int cur = 0;
    gate.gate = b.h(d.layers);
    gate.scale = d.layers > 0 ? scale : 1.0f;   // (fc1 has no dropout behind it)
    out = NthOut{};
    out.c16 = b.da(cur);
    out.ct = b.dat(cur);
    gemm(b.dz(), b.wt(1 + d.layers), out, batch, mlp, NM_OUT, gate, c.part, stream);
    for (uint32_t i = d.layers; i >= 1; --i) {
        out = NthOut{};
        out.c32 = grad + lay.layer_w[i - 1].at;
        gemm(b.dat(cur), b.ht(i - 1), out, mlp, mlp, Bp, raw, c.part, stream);
        bias_grad(b.da(cur), grad + lay.layer_b[i - 1].at, mlp, Mp);
        gate.gate = b.h(i - 1);
        gate.scale = i - 1 > 0 ? scale : 1.0f;
        out = NthOut{};
        out.c16 = b.da(cur ^ 1);
        out.ct = b.dat(cur ^ 1);
        gemm(b.da(cur), b.wt(i), out, batch, mlp, Mp, gate, c.part, stream);
        cur ^= 1;
    }
    out = NthOut{};
    out.c32 = grad + lay.fc1_w.at;
    gemm(b.dat(cur), b.featt(), out, mlp, F, Bp, raw, c.part, stream);
    bias_grad(b.da(cur), grad + lay.fc1_b.at, mlp, Mp);
    out.c32 = c.dfeat;
    gemm(b.da(cur), b.wt(0), out, batch, F, Mp, raw, c.part, stream);
}

}  // namespace pvq
