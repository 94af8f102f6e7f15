// note_trainer.hip — see note_trainer.hpp.
//
// nt_gemm: a workgroup of 4 waves owns a tile of NT_BM = 64 rows x NT_BN = 64 columns; wave w owns rows 16 w .. 16 w + 15 and all 64
// columns (four 16-column strips): 4 accumulator tiles, 16 registers.  K is walked in stages of NT_BK = 32.  Both operands of a
// stage go global -> registers -> LDS one stage ahead, double buffered, one barrier per stage, and both lie in LDS as [row or
// column][k] with a row of 36 floats, so lane l (row or column l & 15, k group g = l >> 4) reads k = 4 g .. 4 g + 3 of a 16-k chunk
// as one 16-byte read: element i of it is the operand of the chunk's i-th v_mfma_f32_16x16x4_f32, for A and B alike.  An operand
// whose k runs along its rows in memory (H and W in the NT product, dZ in NN) is copied as it is; one whose k runs down its columns
// (W in NN, dZ and H in TN) is read in 16-byte pieces along its rows and written to LDS transposed.  Rows, columns and k beyond the
// matrix are read as zeros and never stored: the K tail of the weight gradient (K = batch) adds exact zeros.
//
// Order of every sum is fixed by the shapes alone (tile, stage and split follow from M, N, K; reductions over rows walk them in
// index order; nothing is accumulated atomically), so equal inputs give equal bits.
#include "note_trainer.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "note_device.hpp"
#include "note_epoch.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int NT_THREADS = 256;
constexpr int NT_LD = NT_BK + 4;   // LDS row: 36 floats, 16-byte aligned rows, 16-byte reads of neighbouring rows on different banks

enum { G_NT = 0, G_NN = 1, G_TN = 2 };
using Epi = NoteEpi<float>;   // the gate is an f32 activation [M][N]: gemm() sets its row length

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;        // [M][N]; with splits > 1 the partial sums [splits][M][N]
    uint32_t M, N, K;
    uint32_t lda, ldb;   // row length of A and B as they lie in memory
    uint32_t n_ct;       // column tiles
    uint32_t stages, stages_per_split, splits;
    Epi e;
};

// k along the rows of src: tile rows r0 .. r0 + 63 (bound R), k0 .. k0 + 31 (bound K, a multiple of 4) -> two 16-byte pieces per thread
__device__ __forceinline__ void fetch_rows(const float* __restrict__ src, uint32_t ld, uint32_t R, uint32_t r0, uint32_t K, uint32_t k0, f32x4 (&r)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t f = threadIdx.x + NT_THREADS * j;
        const uint32_t row = r0 + (f >> 3), k = k0 + 4 * (f & 7);
        r[j] = (row < R && k < K) ? *reinterpret_cast<const f32x4*>(src + static_cast<size_t>(row) * ld + k) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}
__device__ __forceinline__ void put_rows(float (*dst)[NT_LD], const f32x4 (&r)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t f = threadIdx.x + NT_THREADS * j;
        *reinterpret_cast<f32x4*>(&dst[f >> 3][4 * (f & 7)]) = r[j];
    }
}
// k down the columns of src ([K][X], X a multiple of 4): tile k0 .. k0 + 31 (bound K), x0 .. x0 + 63 (bound X).  A wave reads 64
// contiguous bytes of each of 16 rows; thread: k = 16 j + ((tid >> 2) & 15), x = x0 + 4 ((tid & 3) + 4 wave)
__device__ __forceinline__ void fetch_cols(const float* __restrict__ src, uint32_t ld, uint32_t X, uint32_t x0, uint32_t K, uint32_t k0, f32x4 (&r)[2]) {
    const uint32_t x = x0 + 4 * ((threadIdx.x & 3) + 4 * (threadIdx.x >> 6));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t k = k0 + 16 * j + ((threadIdx.x >> 2) & 15);
        r[j] = (k < K && x < X) ? *reinterpret_cast<const f32x4*>(src + static_cast<size_t>(k) * ld + x) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}
__device__ __forceinline__ void put_cols(float (*dst)[NT_LD], const f32x4 (&r)[2]) {
    const uint32_t x = 4 * ((threadIdx.x & 3) + 4 * (threadIdx.x >> 6));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t k = 16 * j + ((threadIdx.x >> 2) & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[x + i][k] = r[j][i];
    }
}

template <int MODE>
__device__ __forceinline__ void fetch_ab(const GemmArgs& a, uint32_t m0, uint32_t n0, uint32_t k0, f32x4 (&ra)[2], f32x4 (&rb)[2]) {
    if constexpr (MODE == G_TN) fetch_cols(a.A, a.lda, a.M, m0, a.K, k0, ra);
    else fetch_rows(a.A, a.lda, a.M, m0, a.K, k0, ra);
    if constexpr (MODE == G_NT) fetch_rows(a.B, a.ldb, a.N, n0, a.K, k0, rb);
    else fetch_cols(a.B, a.ldb, a.N, n0, a.K, k0, rb);
}
template <int MODE>
__device__ __forceinline__ void put_ab(float (*sa)[NT_LD], float (*sb)[NT_LD], const f32x4 (&ra)[2], const f32x4 (&rb)[2]) {
    if constexpr (MODE == G_TN) put_cols(sa, ra);
    else put_rows(sa, ra);
    if constexpr (MODE == G_NT) put_rows(sb, rb);
    else put_cols(sb, rb);
}

// G_NT: C = A[M][K] * B[N][K]^T.  G_NN: C = A[M][K] * B[K][N].  G_TN: C = A[K][M]^T * B[K][N].
template <int MODE>
__global__ __launch_bounds__(NT_THREADS) void nt_gemm(const GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float s_a[2][NT_BM][NT_LD];
    __shared__ __attribute__((aligned(16))) float s_b[2][NT_BN][NT_LD];
    const uint32_t ct = blockIdx.x % a.n_ct, rt = blockIdx.x / a.n_ct, z = blockIdx.y;
    const uint32_t m0 = NT_BM * rt, n0 = NT_BN * ct;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const uint32_t st0 = z * a.stages_per_split, st1 = min(st0 + a.stages_per_split, a.stages);

    f32x4 ra[2], rb[2];
    f32x4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (st0 < st1) {
        fetch_ab<MODE>(a, m0, n0, NT_BK * st0, ra, rb);
        put_ab<MODE>(s_a[0], s_b[0], ra, rb);
    }
    __syncthreads();
    for (uint32_t st = st0; st < st1; ++st) {
        const int cur = (st - st0) & 1;
        const bool more = st + 1 < st1;
        if (more) fetch_ab<MODE>(a, m0, n0, NT_BK * (st + 1), ra, rb);
#pragma unroll
        for (int ch = 0; ch < NT_BK / 16; ++ch) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&s_a[cur][16 * wave + c][16 * ch + 4 * g]);
            f32x4 bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) bv[s] = *reinterpret_cast<const f32x4*>(&s_b[cur][16 * s + c][16 * ch + 4 * g]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[s][i], acc[s], 0, 0, 0);
        }
        if (more) put_ab<MODE>(s_a[cur ^ 1], s_b[cur ^ 1], ra, rb);
        __syncthreads();
    }

    // accumulator layout of a 16 x 16 tile: lane l holds column l & 15, rows 4 (l >> 4) + reg
    float* dst = a.C + (a.splits > 1 ? static_cast<size_t>(z) * a.M * a.N : 0);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const uint32_t row = m0 + 16 * wave + 4 * g + reg;
        if (row >= a.M) continue;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t col = n0 + 16 * s + c;
            if (col >= a.N) continue;
            const float v = acc[s][reg];
            dst[static_cast<size_t>(row) * a.N + col] = a.splits > 1 ? v : epi_apply(a.e, v, row, col);
        }
    }
}

// C[i] = epilogue(part[0][i] + part[1][i] + ...), the splits added in their order
__global__ __launch_bounds__(NT_THREADS) void nt_gemm_finish(const float* __restrict__ part, float* __restrict__ C, uint32_t M, uint32_t N, uint32_t splits, const Epi e) {
    const size_t mn = static_cast<size_t>(M) * N;
    const size_t i = static_cast<size_t>(blockIdx.x) * NT_THREADS + threadIdx.x;
    if (i >= mn) return;
    float v = part[i];
    for (uint32_t z = 1; z < splits; ++z) v += part[z * mn + i];
    C[i] = epi_apply(e, v, static_cast<uint32_t>(i / N), static_cast<uint32_t>(i % N));
}

// feat[b][c * o_pool + p] = max(conv[c][2 p], conv[c][2 p + 1], 0) of the window that ends at row idx[b] (train.py:17-21,46,89-91)
__global__ __launch_bounds__(NT_THREADS) void nt_features(const float* __restrict__ db, const uint32_t* __restrict__ idx, const float* __restrict__ conv,
                                                          float* __restrict__ feat, uint32_t n_bins, uint32_t t_frames, uint32_t L, uint32_t o_pool) {
    extern __shared__ float s_x[];   // the window, L floats
    __shared__ float s_w[NOTE_CONV_VALUES];
    const uint32_t b = blockIdx.x;
    const float* x = db + (static_cast<size_t>(idx[b]) - (t_frames - 1)) * n_bins;
    for (uint32_t i = threadIdx.x; i < L; i += NT_THREADS) s_x[i] = x[i];
    if (threadIdx.x < NOTE_CONV_VALUES) s_w[threadIdx.x] = conv[threadIdx.x];
    __syncthreads();
    const uint32_t F = NM_CH * o_pool;
    float* dst = feat + static_cast<size_t>(b) * F;
    for (uint32_t i = threadIdx.x; i < F; i += NT_THREADS) {
        const uint32_t ch = i / o_pool, p = i - ch * o_pool;
        float e, o;
        conv_pair(s_w + ch * NM_KW, s_w[NM_CH * NM_KW + ch], s_x + 4 * p, e, o);   // reads x[4 p .. 4 p + 6] <= x[2 (O_conv - 1) + 4] <= x[L - 1]
        dst[i] = fmaxf(fmaxf(e, o), 0.0f);
    }
}

// Row b's share of the conv gradients: dFeat goes to the larger of each pair (the first on a tie, as max_pool1d), through the ReLU
// (gradient 0 at 0), to the five taps and the bias.  Thread (channel ch = tid >> 4, q = tid & 15) walks pooled positions q, q + 16, ..
// in order; the 16 partial sums of a channel are then added in q order.  part[b][0 .. 79] weights [16][5], [80 .. 95] bias.
__global__ __launch_bounds__(NT_THREADS) void nt_conv_grad(const float* __restrict__ db, const uint32_t* __restrict__ idx, const float* __restrict__ conv,
                                                           const float* __restrict__ dfeat, float* __restrict__ part, uint32_t n_bins, uint32_t t_frames,
                                                           uint32_t L, uint32_t o_pool) {
    extern __shared__ float s_x[];
    __shared__ float s_w[NOTE_CONV_VALUES];
    __shared__ float s_red[NT_THREADS][NM_KW + 1];
    const uint32_t b = blockIdx.x;
    const float* x = db + (static_cast<size_t>(idx[b]) - (t_frames - 1)) * n_bins;
    for (uint32_t i = threadIdx.x; i < L; i += NT_THREADS) s_x[i] = x[i];
    if (threadIdx.x < NOTE_CONV_VALUES) s_w[threadIdx.x] = conv[threadIdx.x];
    __syncthreads();
    const uint32_t ch = threadIdx.x >> 4, q = threadIdx.x & 15;
    const float* g_row = dfeat + static_cast<size_t>(b) * NM_CH * o_pool + static_cast<size_t>(ch) * o_pool;
    float acc[NM_KW + 1];
#pragma unroll
    for (int j = 0; j <= NM_KW; ++j) acc[j] = 0.0f;
    for (uint32_t p = q; p < o_pool; p += 16) {
        float e, o;
        conv_pair(s_w + ch * NM_KW, s_w[NM_CH * NM_KW + ch], s_x + 4 * p, e, o);
        const bool second = o > e;
        if ((second ? o : e) > 0.0f) {
            const float gv = g_row[p];
            const float* xs = s_x + 4 * p + (second ? 2 : 0);
#pragma unroll
            for (int j = 0; j < NM_KW; ++j) acc[j] = fmaf(gv, xs[j], acc[j]);
            acc[NM_KW] += gv;
        }
    }
#pragma unroll
    for (int j = 0; j <= NM_KW; ++j) s_red[threadIdx.x][j] = acc[j];
    __syncthreads();
    if (threadIdx.x < NOTE_CONV_VALUES) {
        const uint32_t c2 = threadIdx.x / (NM_KW + 1), j = threadIdx.x % (NM_KW + 1);
        float s = 0.0f;
        for (int k = 0; k < 16; ++k) s += s_red[16 * c2 + k][j];
        part[static_cast<size_t>(b) * NOTE_CONV_VALUES + (j < NM_KW ? c2 * NM_KW + j : NM_CH * NM_KW + c2)] = s;
    }
}
// grad[i] = part[0][i] + part[1][i] + ... in row order
__global__ __launch_bounds__(128) void nt_conv_reduce(const float* __restrict__ part, float* __restrict__ grad, uint32_t batch) {
    if (threadIdx.x >= NOTE_CONV_VALUES) return;
    float s = 0.0f;
    for (uint32_t b = 0; b < batch; ++b) s += part[static_cast<size_t>(b) * NOTE_CONV_VALUES + threadIdx.x];
    grad[threadIdx.x] = s;
}

// out[col] = sum over rows of d[row][col]: thread (phase = tid >> 6, column) adds rows phase, phase + 4, .. in order, the four phases
// are added in order
__global__ __launch_bounds__(NT_THREADS) void nt_bias_grad(const float* __restrict__ d, float* __restrict__ out, uint32_t M, uint32_t N) {
    __shared__ float s_red[4][64];
    const uint32_t col = 64 * blockIdx.x + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    float s = 0.0f;
    if (col < N)
        for (uint32_t r = ph; r < M; r += 4) s += d[static_cast<size_t>(r) * N + col];
    s_red[ph][threadIdx.x & 63] = s;
    __syncthreads();
    if (ph == 0 && col < N) out[col] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

// One workgroup per row of the batch, one thread per output.  loss = max(z, 0) - z y + log1p(exp(-|z|)); dz = (sigmoid(z) - y) * inv_n
// with inv_n = 1 / (batch * 128) (train.py:153-156: BCELoss's mean reduction, backward).  The row's 128 losses are added as a tree in double.
__global__ __launch_bounds__(NM_OUT) void nt_loss(const float* __restrict__ z, const float* __restrict__ targets, const uint32_t* __restrict__ idx,
                                                  float inv_n, float* __restrict__ dz, float* __restrict__ logits_out, double* __restrict__ row_loss) {
    __shared__ double s_red[NM_OUT];
    const uint32_t b = blockIdx.x, j = threadIdx.x;
    const float zv = z[static_cast<size_t>(b) * NM_OUT + j];
    const float y = targets[static_cast<size_t>(idx[b]) * NM_OUT + j];
    const float l = fmaxf(zv, 0.0f) - zv * y + log1pf(expf(-fabsf(zv)));
    dz[static_cast<size_t>(b) * NM_OUT + j] = (1.0f / (1.0f + expf(-zv)) - y) * inv_n;
    if (logits_out) logits_out[static_cast<size_t>(b) * NM_OUT + j] = zv;
    s_red[j] = static_cast<double>(l);
    __syncthreads();
    for (int s = NM_OUT / 2; s > 0; s >>= 1) {
        if (j < static_cast<uint32_t>(s)) s_red[j] += s_red[j + s];
        __syncthreads();
    }
    if (j == 0) row_loss[b] = s_red[0];
}
__global__ __launch_bounds__(NT_THREADS) void nt_loss_final(const double* __restrict__ row_loss, uint32_t batch, double inv_n, float* __restrict__ loss) {
    __shared__ double s_red[NT_THREADS];
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < batch; b += NT_THREADS) s += row_loss[b];
    s_red[threadIdx.x] = s;
    __syncthreads();
    for (int k = NT_THREADS / 2; k > 0; k >>= 1) {
        if (threadIdx.x < static_cast<uint32_t>(k)) s_red[threadIdx.x] += s_red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = static_cast<float>(s_red[0] * inv_n);
}

// The test pass (train.py:164-198).  One workgroup per row of a chunk, one thread per output, shaped like nt_loss without its dz.  Row b of
// the chunk is entry pos0 + b of the pass; everything it leaves is indexed by that position, so a test batch that straddles two chunks
// needs no special case.  Prediction z > 0, label y > 0.5 (train.py:177-178): a wave's ballot is 64 bits of the row's 128-bit mask (bit k =
// word k / 32, bit k % 32, as pvq_note_model_outputs.d_mask); masks[pos][0 .. 3] prediction, [4 .. 7] label.  counts[pos] = tp, fp, fn,
// correct by popcount; row_loss[pos] the row's 128 losses added as nt_loss's tree in double.
__global__ __launch_bounds__(NM_OUT) void nt_test_rows(const float* __restrict__ z, const float* __restrict__ targets, const uint32_t* __restrict__ idx,
                                                       size_t pos0, uint32_t* __restrict__ masks, uint4* __restrict__ counts, double* __restrict__ row_loss,
                                                       float* __restrict__ logits_out) {
    __shared__ double s_red[NM_OUT];
    __shared__ uint32_t s_cnt[NM_OUT / 64][4];
    const uint32_t b = blockIdx.x, j = threadIdx.x, wave = j >> 6;
    const size_t pos = pos0 + b;
    const float zv = z[static_cast<size_t>(b) * NM_OUT + j];
    const float y = targets[static_cast<size_t>(idx[b]) * NM_OUT + j];
    const float l = fmaxf(zv, 0.0f) - zv * y + log1pf(expf(-fabsf(zv)));
    if (logits_out) logits_out[pos * NM_OUT + j] = zv;
    const unsigned long long p = __ballot(zv > 0.0f), q = __ballot(y > 0.5f);
    if ((j & 63) == 0) {
        uint32_t* m = masks + pos * 8;
        m[2 * wave] = static_cast<uint32_t>(p);
        m[2 * wave + 1] = static_cast<uint32_t>(p >> 32);
        m[4 + 2 * wave] = static_cast<uint32_t>(q);
        m[4 + 2 * wave + 1] = static_cast<uint32_t>(q >> 32);
        s_cnt[wave][0] = __popcll(p & q);
        s_cnt[wave][1] = __popcll(p & ~q);
        s_cnt[wave][2] = __popcll(~p & q);
        s_cnt[wave][3] = 64 - __popcll(p ^ q);
    }
    s_red[j] = static_cast<double>(l);
    __syncthreads();
    for (int s = NM_OUT / 2; s > 0; s >>= 1) {
        if (j < static_cast<uint32_t>(s)) s_red[j] += s_red[j + s];
        __syncthreads();
    }
    if (j == 0) {
        counts[pos] = make_uint4(s_cnt[0][0] + s_cnt[1][0], s_cnt[0][1] + s_cnt[1][1], s_cnt[0][2] + s_cnt[1][2], s_cnt[0][3] + s_cnt[1][3]);
        row_loss[pos] = s_red[0];
    }
}
// One wave per test batch k = rows k * batch .. of the pass (the last may be short).  Lane l adds rows l, l + 64, .. of the batch in that
// order, then the 64 lanes are added as a tree: the order of the loss sum in double depends on the batch's row count alone.
__global__ __launch_bounds__(NT_THREADS) void nt_test_batches(const uint4* __restrict__ counts, const double* __restrict__ row_loss, size_t n_idx,
                                                              uint32_t batch, size_t n_batches, pvq_note_test_batch* __restrict__ out) {
    const size_t k = static_cast<size_t>(blockIdx.x) * (NT_THREADS / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (k >= n_batches) return;   // (a whole wave)
    const size_t r0 = k * batch;
    const uint32_t rows = static_cast<uint32_t>(min(static_cast<size_t>(batch), n_idx - r0));
    uint32_t tp = 0, fp = 0, fn = 0, ok = 0;
    double s = 0.0;
    for (uint32_t r = lane; r < rows; r += 64) {
        const uint4 c = counts[r0 + r];
        tp += c.x;
        fp += c.y;
        fn += c.z;
        ok += c.w;
        s += row_loss[r0 + r];
    }
    for (int off = 32; off > 0; off >>= 1) {
        tp += __shfl_down(tp, off);
        fp += __shfl_down(fp, off);
        fn += __shfl_down(fn, off);
        ok += __shfl_down(ok, off);
        s += __shfl_down(s, off);
    }
    if (lane == 0) {
        pvq_note_test_batch o;
        o.rows = rows;
        o.tp = tp;
        o.fp = fp;
        o.fn = fn;
        o.correct = ok;
        o._pad = 0;
        o.loss = s / (static_cast<double>(rows) * NM_OUT);
        out[k] = o;
    }
}
// out[pitch][tp, fp, fn] over all rows of the pass, from the masks: thread = pitch, a workgroup walks rows blockIdx.x, + gridDim.x, ..
// and adds its counts to `out` (zeroed before the launch) atomically: integer sums, the same in any order.
__global__ __launch_bounds__(NM_OUT) void nt_test_pitches(const uint32_t* __restrict__ masks, size_t n_idx, uint32_t* __restrict__ out) {
    const uint32_t w = threadIdx.x >> 5, bit = threadIdx.x & 31;
    uint32_t tp = 0, fp = 0, fn = 0;
    for (size_t r = blockIdx.x; r < n_idx; r += gridDim.x) {
        const uint32_t p = (masks[r * 8 + w] >> bit) & 1u, q = (masks[r * 8 + 4 + w] >> bit) & 1u;
        tp += p & q;
        fp += p & (q ^ 1u);
        fn += (p ^ 1u) & q;
    }
    atomicAdd(out + 3 * threadIdx.x, tp);
    atomicAdd(out + 3 * threadIdx.x + 1, fp);
    atomicAdd(out + 3 * threadIdx.x + 2, fn);
}

// torch.optim.Adam with L2 weight decay (train.py:141-144), four elements per thread.  The element's arithmetic is done in double
// and rounded once per stored value: the kernel moves 28 bytes per element and has the time.
__global__ __launch_bounds__(NT_THREADS) void nt_adam(f32x4* __restrict__ w, const f32x4* __restrict__ g, f32x4* __restrict__ m, f32x4* __restrict__ v,
                                                      size_t n4, const NtAdamStep s) {
    const size_t i = static_cast<size_t>(blockIdx.x) * NT_THREADS + threadIdx.x;
    if (i >= n4) return;
    f32x4 wv = w[i], mv = m[i], vv = v[i];
    const f32x4 gv = g[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double wd = static_cast<double>(wv[k]);
        const double gd = static_cast<double>(gv[k]) + s.weight_decay * wd;
        const double md = s.beta1 * static_cast<double>(mv[k]) + (1.0 - s.beta1) * gd;
        const double vd = s.beta2 * static_cast<double>(vv[k]) + (1.0 - s.beta2) * gd * gd;
        mv[k] = static_cast<float>(md);
        vv[k] = static_cast<float>(vd);
        wv[k] = static_cast<float>(wd - s.step_size * md / (sqrt(vd) * s.inv_bc2_sqrt + s.eps));
    }
    w[i] = wv;
    m[i] = mv;
    v[i] = vv;
}

size_t round64(size_t n) { return (n + 63) & ~static_cast<size_t>(63); }

// one product; a split one goes through `part` and nt_gemm_finish
void gemm(int mode, const float* A, const float* B, float* C, uint32_t M, uint32_t N, uint32_t K, uint32_t lda, uint32_t ldb, const Epi& e, float* part,
          hipStream_t stream) {
    GemmArgs a{};
    a.A = A;
    a.B = B;
    a.M = M;
    a.N = N;
    a.K = K;
    a.lda = lda;
    a.ldb = ldb;
    a.n_ct = (N + NT_BN - 1) / NT_BN;
    a.stages = (K + NT_BK - 1) / NT_BK;
    const uint32_t want = nt_splits(M, N, K);
    a.stages_per_split = (a.stages + want - 1) / want;
    a.splits = (a.stages + a.stages_per_split - 1) / a.stages_per_split;   // no empty split
    a.C = a.splits > 1 ? part : C;
    a.e = e;
    a.e.ldg = N;
    const dim3 grid(((M + NT_BM - 1) / NT_BM) * a.n_ct, a.splits);
    if (mode == G_NT) hipLaunchKernelGGL(nt_gemm<G_NT>, grid, dim3(NT_THREADS), 0, stream, a);
    else if (mode == G_NN) hipLaunchKernelGGL(nt_gemm<G_NN>, grid, dim3(NT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(nt_gemm<G_TN>, grid, dim3(NT_THREADS), 0, stream, a);
    if (a.splits > 1) {
        const size_t mn = static_cast<size_t>(M) * N;
        hipLaunchKernelGGL(nt_gemm_finish, dim3(static_cast<uint32_t>((mn + NT_THREADS - 1) / NT_THREADS)), dim3(NT_THREADS), 0, stream, part, C, M, N,
                           a.splits, a.e);
    }
}
}  // namespace

NoteTrainer::~NoteTrainer() {
    if (device_id_ < 0) return;
    (void)hipSetDevice(device_id_);
    (void)hipDeviceSynchronize();
    for (int s = 0; s < 2; ++s) {
        if (idx_copied_[s]) (void)hipEventDestroy(idx_copied_[s]);
        if (h_idx_[s]) (void)hipHostFree(h_idx_[s]);
    }
    if (h_test_out_) (void)hipHostFree(h_test_out_);
    if (h_epoch_) (void)hipHostFree(h_epoch_);
}

NthContext NoteTrainer::half_context() const {
    NthContext c;
    c.lay = &lay_;
    c.plan = &half_;
    c.arena = arena_.as<float>();
    c.shadow = shadow_.as<uint16_t>();
    c.ws16 = ws16_.as<uint16_t>();
    c.part = ws(ws_part_);
    c.d_idx = reinterpret_cast<const uint32_t*>(ws(ws_idx_));
    c.Z = ws(ws_z_);
    c.dZ = ws(ws_dz_);
    c.dfeat = ws(ws_dfeat_);
    c.hyper = hyper_;
    c.steps = steps_;
    return c;
}

pvq_status NoteTrainer::create(int device_id, const pvq_note_model_params* params, const pvq_note_model_weights* weights,
                               const pvq_note_trainer_hyper* hyper, uint32_t max_batch, pvq_note_precision precision, std::unique_ptr<NoteTrainer>& out) {
    out.reset();
    NoteModelDims d;
    std::string err;
    pvq_status st = note_trainer_check_precision(static_cast<int>(precision), err);
    if (st == PVQ_OK) st = note_model_check(params, weights, d, err);
    if (st == PVQ_OK) st = note_trainer_check_hyper(hyper, max_batch, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    std::unique_ptr<NoteTrainer> t(new NoteTrainer());
    t->device_id_ = device_id < 0 ? -1 : device_id;
    t->lay_ = note_trainer_layout(d);
    t->hyper_ = *hyper;
    t->max_batch_ = max_batch;
    t->precision_ = precision;
    if (precision == PVQ_NOTE_BF16) t->half_ = note_trainer_half_plan(t->lay_, max_batch);
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        const size_t n = t->lay_.n_params;
        const std::vector<float> arena = note_trainer_arena(t->lay_, *weights);
        if (pvq_status s = t->arena_.reserve(4 * n * sizeof(float))) return s;
        PVQ_HIP(hipMemcpy(t->arena_.as<float>(), arena.data(), n * sizeof(float), hipMemcpyHostToDevice));
        PVQ_HIP(hipMemset(t->arena_.as<float>() + n, 0, 3 * n * sizeof(float)));
        // the workspace, sized once from max_batch
        const size_t B = max_batch;
        size_t at = 0;
        auto take = [&at](size_t floats) {
            const size_t here = at;
            at += round64(floats);
            return here;
        };
        t->ws_feat_ = take(B * d.n_features);
        t->ws_dfeat_ = take(B * d.n_features);
        t->ws_h_ = take((d.layers + 1) * round64(B * d.mlp));
        t->ws_da_ = take(2 * round64(B * d.mlp));
        t->ws_z_ = take(B * NM_OUT);
        t->ws_dz_ = take(B * NM_OUT);
        t->ws_convpart_ = take(B * NOTE_CONV_VALUES);
        t->ws_rowloss_ = take(2 * B);   // doubles
        t->ws_part_ = take(NT_PART_FLOATS);
        t->ws_idx_ = take(B);           // uint32
        if (pvq_status s = t->ws_.reserve(at * sizeof(float))) return s;
        for (int s = 0; s < 2; ++s) {
            PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&t->h_idx_[s]), B * sizeof(uint32_t), hipHostMallocDefault));
            PVQ_HIP(hipEventCreateWithFlags(&t->idx_copied_[s], hipEventDisableTiming));
        }
        if (precision == PVQ_NOTE_BF16) {
            // the shadow weights and the 16-bit workspace; zeroed once, so no product ever meets a padding that is no number
            if (pvq_status s = t->shadow_.reserve(t->half_.shadow_total * sizeof(uint16_t))) return s;
            if (pvq_status s = t->ws16_.reserve(t->half_.ws_total * sizeof(uint16_t))) return s;
            PVQ_HIP(hipMemset(t->shadow_.as<void>(), 0, t->half_.shadow_total * sizeof(uint16_t)));
            PVQ_HIP(hipMemset(t->ws16_.as<void>(), 0, t->half_.ws_total * sizeof(uint16_t)));
            nth_refresh_shadow(t->half_context(), nullptr);
            PVQ_HIP(hipGetLastError());
            PVQ_HIP(hipDeviceSynchronize());
        }
    }
    out = std::move(t);
    return PVQ_OK;
}

// idx -> pinned slot -> device.  The slot is free once the copy queued from it two calls ago has run.
pvq_status NoteTrainer::upload_idx(const uint32_t* idx, uint32_t rows, hipStream_t stream) {
    const int slot = static_cast<int>(calls_++ & 1);
    if (idx_pending_[slot]) PVQ_HIP(hipEventSynchronize(idx_copied_[slot]));
    std::memcpy(h_idx_[slot], idx, rows * sizeof(uint32_t));
    uint32_t* d_idx = reinterpret_cast<uint32_t*>(ws(ws_idx_));
    PVQ_HIP(hipMemcpyAsync(d_idx, h_idx_[slot], rows * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    PVQ_HIP(hipEventRecord(idx_copied_[slot], stream));
    idx_pending_[slot] = true;
    return PVQ_OK;
}

// forward (train.py:87-99)
void NoteTrainer::forward(const float* d_db, uint32_t batch, bool train, hipStream_t stream) {
    if (precision_ == PVQ_NOTE_BF16) {
        nth_forward(half_context(), d_db, batch, train, stream);
        return;
    }
    const NoteModelDims& d = lay_.d;
    const float* w = arena_.as<float>();
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ws(ws_idx_));
    float* feat = ws(ws_feat_);
    const size_t h_stride = round64(static_cast<size_t>(max_batch_) * d.mlp);
    auto H = [&](uint32_t i) { return ws(ws_h_) + i * h_stride; };
    float* Z = ws(ws_z_);
    float* part = ws(ws_part_);
    const uint32_t F = d.n_features, mlp = d.mlp;
    const uint32_t threshold = nt_keep_threshold(hyper_.dropout);
    const bool drop = train && threshold > 0;
    const float scale = drop ? static_cast<float>(1.0 / (1.0 - hyper_.dropout)) : 1.0f;
    const size_t x_bytes = static_cast<size_t>(d.L) * sizeof(float);

    hipLaunchKernelGGL(nt_features, dim3(batch), dim3(NT_THREADS), x_bytes, stream, d_db, d_idx, w + lay_.conv_w.at, feat, d.n_bins, d.t_frames, d.L, d.o_pool);
    Epi e{};
    e.kind = E_HIDDEN;
    e.bias = w + lay_.fc1_b.at;
    e.scale = 1.0f;
    gemm(G_NT, feat, w + lay_.fc1_w.at, H(0), batch, mlp, F, F, F, e, part, stream);
    for (uint32_t i = 0; i < d.layers; ++i) {
        e.bias = w + lay_.layer_b[i].at;
        e.drop = drop ? 1 : 0;
        e.scale = scale;
        e.threshold = threshold;
        e.key = nt_layer_key(hyper_.seed, steps_, i);
        gemm(G_NT, H(i), w + lay_.layer_w[i].at, H(i + 1), batch, mlp, mlp, mlp, mlp, e, part, stream);
    }
    e = Epi{};
    e.kind = E_BIAS;
    e.bias = w + lay_.out_b.at;
    gemm(G_NT, H(d.layers), w + lay_.out_w.at, Z, batch, NM_OUT, mlp, mlp, mlp, e, part, stream);
}

// backward from nt_loss's dZ: the output layer, the hidden layers from the last to the first, fc1 -> every dense gradient, dfeat
void NoteTrainer::backward(uint32_t batch, hipStream_t stream) {
    if (precision_ == PVQ_NOTE_BF16) {
        nth_backward(half_context(), batch, stream);
        return;
    }
    const NoteModelDims& d = lay_.d;
    const float* w = arena_.as<float>();
    float* grad = arena_.as<float>() + lay_.n_params;
    const size_t h_stride = round64(static_cast<size_t>(max_batch_) * d.mlp);
    auto H = [&](uint32_t i) { return ws(ws_h_) + i * h_stride; };
    float* dA[2] = {ws(ws_da_), ws(ws_da_) + h_stride};
    float* dZ = ws(ws_dz_);
    float* part = ws(ws_part_);
    const uint32_t F = d.n_features, mlp = d.mlp;
    const bool drop = nt_keep_threshold(hyper_.dropout) > 0;
    const float scale = drop ? static_cast<float>(1.0 / (1.0 - hyper_.dropout)) : 1.0f;

    Epi raw{};
    raw.kind = E_RAW;
    Epi gate{};
    gate.kind = E_GATE;
    gemm(G_TN, dZ, H(d.layers), grad + lay_.out_w.at, NM_OUT, mlp, batch, NM_OUT, mlp, raw, part, stream);
    hipLaunchKernelGGL(nt_bias_grad, dim3((NM_OUT + 63) / 64), dim3(NT_THREADS), 0, stream, dZ, grad + lay_.out_b.at, batch, static_cast<uint32_t>(NM_OUT));
    int cur = 0;
    gate.gate = H(d.layers);
    gate.scale = d.layers > 0 ? scale : 1.0f;   // (fc1 has no dropout behind it, train.py:93)
    gemm(G_NN, dZ, w + lay_.out_w.at, dA[cur], batch, mlp, NM_OUT, NM_OUT, mlp, gate, part, stream);
    for (uint32_t i = d.layers; i >= 1; --i) {
        gemm(G_TN, dA[cur], H(i - 1), grad + lay_.layer_w[i - 1].at, mlp, mlp, batch, mlp, mlp, raw, part, stream);
        hipLaunchKernelGGL(nt_bias_grad, dim3((mlp + 63) / 64), dim3(NT_THREADS), 0, stream, dA[cur], grad + lay_.layer_b[i - 1].at, batch, mlp);
        gate.gate = H(i - 1);
        gate.scale = i - 1 > 0 ? scale : 1.0f;
        gemm(G_NN, dA[cur], w + lay_.layer_w[i - 1].at, dA[cur ^ 1], batch, mlp, mlp, mlp, mlp, gate, part, stream);
        cur ^= 1;
    }
    gemm(G_TN, dA[cur], ws(ws_feat_), grad + lay_.fc1_w.at, mlp, F, batch, mlp, F, raw, part, stream);
    hipLaunchKernelGGL(nt_bias_grad, dim3((mlp + 63) / 64), dim3(NT_THREADS), 0, stream, dA[cur], grad + lay_.fc1_b.at, batch, mlp);
    gemm(G_NN, dA[cur], w + lay_.fc1_w.at, ws(ws_dfeat_), batch, F, mlp, mlp, F, raw, part, stream);
}

// the checks, the upload, then run_step
pvq_status NoteTrainer::step(int mode, const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, uint32_t batch, float* d_loss,
                             float* d_logits, hipStream_t stream) {
    const NoteModelDims& d = lay_.d;
    std::string err;
    const pvq_status st = note_trainer_check_step(d, max_batch_, mode, d_db, d_targets, n_rows, idx, batch, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    if (device_id_ < 0) {
        set_last_error("the note trainer runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    const pvq_status up = upload_idx(idx, batch, stream);
    if (up != PVQ_OK) return up;
    return run_step(mode, d_db, d_targets, batch, d_loss, d_logits, stream);
}

// forward, loss; when training: backward, the conv gradient; PVQ_TRAIN_STEP: Adam, the shadow refresh of a bf16 handle
pvq_status NoteTrainer::run_step(int mode,const float* d_db, const float* d_targets, uint32_t batch, float* d_loss, float* d_logits, hipStream_t stream) {
    const NoteModelDims& d = lay_.d;
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ws(ws_idx_));
    const size_t n = lay_.n_params;
    float* arena = arena_.as<float>();
    float* grad = arena + n;
    double* row_loss = reinterpret_cast<double*>(ws(ws_rowloss_));
    const bool train = mode != PVQ_TRAIN_EVAL;

    forward(d_db, batch, train, stream);
    const double inv_n = 1.0 / (static_cast<double>(batch) * NM_OUT);
    hipLaunchKernelGGL(nt_loss, dim3(batch), dim3(NM_OUT), 0, stream, ws(ws_z_), d_targets, d_idx, static_cast<float>(inv_n), ws(ws_dz_), d_logits, row_loss);
    if (d_loss) hipLaunchKernelGGL(nt_loss_final, dim3(1), dim3(NT_THREADS), 0, stream, row_loss, batch, inv_n, d_loss);
    if (train) {
        backward(batch, stream);
        // the conv from dfeat, then Adam
        float* conv_part = ws(ws_convpart_);
        hipLaunchKernelGGL(nt_conv_grad, dim3(batch), dim3(NT_THREADS), static_cast<size_t>(d.L) * sizeof(float), stream, d_db, d_idx, arena + lay_.conv_w.at,
                           ws(ws_dfeat_), conv_part, d.n_bins, d.t_frames, d.L, d.o_pool);
        hipLaunchKernelGGL(nt_conv_reduce, dim3(1), dim3(128), 0, stream, conv_part, grad + lay_.conv_w.at, batch);
        if (mode == PVQ_TRAIN_STEP) {
            const size_t n4 = n / 4;
            hipLaunchKernelGGL(nt_adam, dim3(static_cast<uint32_t>((n4 + NT_THREADS - 1) / NT_THREADS)), dim3(NT_THREADS), 0, stream,
                               reinterpret_cast<f32x4*>(arena), reinterpret_cast<const f32x4*>(grad), reinterpret_cast<f32x4*>(arena + 2 * n),
                               reinterpret_cast<f32x4*>(arena + 3 * n), n4, note_trainer_adam_step(hyper_, steps_ + 1));
            ++steps_;
            if (precision_ == PVQ_NOTE_BF16) nth_refresh_shadow(half_context(), stream);
        }
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status NoteTrainer::test(const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx, uint32_t batch,
                             pvq_note_test_batch* out_batches, uint32_t* out_pitch, float* d_logits, hipStream_t stream) {
    std::string err;
    const pvq_status st = note_trainer_check_test(lay_.d, d_db, d_targets, n_rows, idx, n_idx, batch, out_batches, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    if (device_id_ < 0) {
        set_last_error("the note trainer runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    const NoteTrainerTestPlan plan = note_trainer_test_plan(n_idx, max_batch_, batch);
    // grow-only buffers: the rows' masks [n_idx][8] words, counts [n_idx] uint4 and losses [n_idx] doubles; the records and pitch counts
    if (pvq_status s = test_rows_.reserve(plan.rows_bytes)) return s;
    if (pvq_status s = test_out_.reserve(plan.out_bytes)) return s;
    if (plan.out_bytes > h_test_out_bytes_) {
        if (h_test_out_) PVQ_HIP(hipHostFree(h_test_out_));
        h_test_out_ = nullptr;
        h_test_out_bytes_ = 0;
        PVQ_HIP(hipHostMalloc(&h_test_out_, plan.out_bytes, hipHostMallocDefault));
        h_test_out_bytes_ = plan.out_bytes;
    }
    char* rows_base = test_rows_.as<char>();
    uint32_t* masks = reinterpret_cast<uint32_t*>(rows_base);
    uint4* counts = reinterpret_cast<uint4*>(rows_base + 32 * n_idx);
    double* row_loss = reinterpret_cast<double*>(rows_base + 48 * n_idx);
    pvq_note_test_batch* d_batches = test_out_.as<pvq_note_test_batch>();
    const size_t batch_bytes = plan.n_batches * sizeof(pvq_note_test_batch);
    uint32_t* d_pitch = reinterpret_cast<uint32_t*>(test_out_.as<char>() + batch_bytes);
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ws(ws_idx_));

    for (const NtTestChunk& c : plan.chunks) {
        const pvq_status up = upload_idx(idx + c.begin, c.rows, stream);
        if (up != PVQ_OK) return up;
        forward(d_db, c.rows, false, stream);
        hipLaunchKernelGGL(nt_test_rows, dim3(c.rows), dim3(NM_OUT), 0, stream, ws(ws_z_), d_targets, d_idx, c.begin, masks, counts, row_loss, d_logits);
    }
    constexpr uint32_t per_block = NT_THREADS / 64;
    hipLaunchKernelGGL(nt_test_batches, dim3(static_cast<uint32_t>((plan.n_batches + per_block - 1) / per_block)), dim3(NT_THREADS), 0, stream, counts, row_loss,
                       n_idx, batch, plan.n_batches, d_batches);
    if (out_pitch) {
        PVQ_HIP(hipMemsetAsync(d_pitch, 0, NT_TEST_PITCH_BYTES, stream));
        hipLaunchKernelGGL(nt_test_pitches, dim3(static_cast<uint32_t>(std::min<size_t>(n_idx, 1024))), dim3(NM_OUT), 0, stream, masks, n_idx, d_pitch);
    }
    PVQ_HIP(hipGetLastError());
    // the one read-back, the one wait
    const size_t back = batch_bytes + (out_pitch ? NT_TEST_PITCH_BYTES : 0);
    PVQ_HIP(hipMemcpyAsync(h_test_out_, test_out_.as<void>(), back, hipMemcpyDeviceToHost, stream));
    PVQ_HIP(hipStreamSynchronize(stream));
    std::memcpy(out_batches, h_test_out_, batch_bytes);
    if (out_pitch) std::memcpy(out_pitch, static_cast<const char*>(h_test_out_) + batch_bytes, NT_TEST_PITCH_BYTES);
    return PVQ_OK;
}

// The split up once, its gathered order by one kernel, then per batch: its slice of the order into the step's index array (device to
// device) and the step's launches, the loss into the batch's slot.  One read-back, one wait.
pvq_status NoteTrainer::epoch(const float* d_db, const float* d_targets, size_t n_rows, const uint32_t* idx, size_t n_idx, uint32_t batch,
                              uint64_t shuffle_seed, uint64_t epoch, float* out_losses, double* out_mean_loss, hipStream_t stream) {
    std::string err;
    const pvq_status st = note_trainer_check_epoch(lay_.d, max_batch_, d_db, d_targets, n_rows, idx, n_idx, batch, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    if (device_id_ < 0) {
        set_last_error("the note trainer runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    const NoteTrainerEpochPlan plan = note_trainer_epoch_plan(n_idx, batch);
    if (pvq_status s = epoch_buf_.reserve(plan.device_bytes)) return s;
    if (plan.host_bytes > h_epoch_bytes_) {
        if (h_epoch_) PVQ_HIP(hipHostFree(h_epoch_));
        h_epoch_ = nullptr;
        h_epoch_bytes_ = 0;
        PVQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_epoch_), plan.host_bytes, hipHostMallocDefault));
        h_epoch_bytes_ = plan.host_bytes;
    }
    uint32_t* words = epoch_buf_.as<uint32_t>();
    uint32_t* d_split = words + plan.idx_at;
    uint32_t* d_order = words + plan.order_at;
    float* d_losses = reinterpret_cast<float*>(words + plan.loss_at);
    uint32_t* d_idx = reinterpret_cast<uint32_t*>(ws(ws_idx_));

    std::memcpy(h_epoch_ + plan.h_idx_at, idx, n_idx * sizeof(uint32_t));
    PVQ_HIP(hipMemcpyAsync(d_split, h_epoch_ + plan.h_idx_at, n_idx * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    note_epoch_gather(d_split, d_order, static_cast<uint32_t>(n_idx), shuffle_seed, epoch, stream);
    for (size_t k = 0; k < plan.n_batches; ++k) {
        const uint32_t rows = k + 1 < plan.n_batches ? batch : plan.last_rows;
        PVQ_HIP(hipMemcpyAsync(d_idx, d_order + k * batch, rows * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        const pvq_status rs = run_step(PVQ_TRAIN_STEP, d_db, d_targets, rows, d_losses + k, nullptr, stream);
        if (rs != PVQ_OK) return rs;
    }
    // the one read-back, the one wait
    float* h_losses = reinterpret_cast<float*>(h_epoch_ + plan.h_loss_at);
    PVQ_HIP(hipMemcpyAsync(h_losses, d_losses, plan.n_batches * sizeof(float), hipMemcpyDeviceToHost, stream));
    PVQ_HIP(hipStreamSynchronize(stream));
    if (out_losses) std::memcpy(out_losses, h_losses, plan.n_batches * sizeof(float));
    if (out_mean_loss) *out_mean_loss = note_epoch_mean_loss(h_losses, plan.n_batches);
    return PVQ_OK;
}

pvq_status NoteTrainer::write(int what, const float* host, size_t count) {
    std::string err;
    const pvq_status st = note_trainer_check_write(what, host, count, lay_.n_params, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    if (device_id_ < 0) {
        set_last_error("the note trainer's state lives on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    PVQ_HIP(hipMemcpy(arena_.as<float>() + static_cast<size_t>(what) * lay_.n_params, host, lay_.n_params * sizeof(float), hipMemcpyHostToDevice));
    if (what == PVQ_TRAIN_WEIGHTS && precision_ == PVQ_NOTE_BF16) {
        // the 16-bit shadow is a function of the weights: as after nt_adam
        nth_refresh_shadow(half_context(), nullptr);
        PVQ_HIP(hipGetLastError());
        PVQ_HIP(hipDeviceSynchronize());
    }
    return PVQ_OK;
}

pvq_status NoteTrainer::set_steps(uint64_t steps) {
    std::string err;
    const pvq_status st = note_trainer_check_steps(steps, err);
    if (st != PVQ_OK) {
        set_last_error(err);
        return st;
    }
    steps_ = steps;
    return PVQ_OK;
}

pvq_status NoteTrainer::read(int what, float* out, size_t capacity) {
    if (what < PVQ_TRAIN_WEIGHTS || what > PVQ_TRAIN_ADAM_V) {
        set_last_error("note trainer: unknown array");
        return PVQ_ERR_INVALID_ARG;
    }
    if (!out || capacity < lay_.n_params) {
        set_last_error("note trainer: the read-back buffer is null or holds fewer than " + std::to_string(lay_.n_params) + " floats");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the note trainer's state lives on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    PVQ_HIP(hipMemcpy(out, arena_.as<float>() + static_cast<size_t>(what) * lay_.n_params, lay_.n_params * sizeof(float), hipMemcpyDeviceToHost));
    return PVQ_OK;
}

}  // namespace pvq
