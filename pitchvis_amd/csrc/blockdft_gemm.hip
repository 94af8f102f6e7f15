// blockdft_gemm.hip — the hop-DFT GEMM and combine-tree stages of the block-DFT path (vqt_blockdft.hip has the map), with their launchers.
//
// Kernels:  blockdft_gemm_tree[_bf16x3] (MFMA GEMM + combine tree fused; the first 64 hop blocks of a window)
//           blockdft_tree_finish (the last one or two tree levels of windows of more than 64 hop blocks)
//           blockdft_gemm_gen (hops that do not divide the windows: whole hop blocks + the window's remainder)
//           blockdft_gemm_rows + blockdft_combine (the same two stages unfused: more than 8 window groups)
#include "blockdft_device.hpp"

namespace pvq {

// ------------------------------------------------------------------------------------------------
// GEMM: P[j][n] = sum_m pcm[s(n) + j*K + m] * E[m][n]        (exact fp32 MFMA)
// ------------------------------------------------------------------------------------------------
// 16-byte raw buffer load.  Bound to the LLVM intrinsic by name: this compiler lowers
// __builtin_amdgcn_raw_buffer_load_b64 / _b128 to a single-dword load.
__device__ f32x4 pvq_raw_buffer_load_f32x4(i32x4 srsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");

// LDS-DMA (global_load_lds_*): 64 lanes x 16 (4) bytes from per-lane global addresses to wave-uniform LDS base + 16 (4) * lane, no register
// destination; counted in vmcnt like any load.
typedef __attribute__((address_space(1))) const void pvq_gvoid;
typedef __attribute__((address_space(3))) void pvq_lvoid;
__device__ __forceinline__ void lds_dma16(const void* g_lane, void* lds_wave) {
    __builtin_amdgcn_global_load_lds((pvq_gvoid*)g_lane, (pvq_lvoid*)lds_wave, 16, 0, 0);
}
__device__ __forceinline__ void lds_dma4(const void* g_lane, void* lds_wave) {
    __builtin_amdgcn_global_load_lds((pvq_gvoid*)g_lane, (pvq_lvoid*)lds_wave, 4, 0, 0);
}

struct GemmArgs {
    const float* pcm_base;    // rebased per launch so that byte offsets fit 32 bits
    unsigned pcm_bytes;       // bytes readable from pcm_base (hardware bounds check: beyond -> 0)
    const float* E;
    int ld;                   // Ntot
    float* P;
    int n_rows;               // rows of P to produce
    int K;                    // hop
    const long long* tile_s;  // per 64-float column tile: window begin relative to the n_fft buffer end (w0 - n_fft)
    long long base;           // index, relative to pcm_base, of the end of frame 0 of this launch
    int n_col_tiles;          // column tiles of this kernel's BN
    int p_rows;               // row capacity of the tile-major P: P[(tile64 * p_rows + row) * 64 + (col & 63)]
};

// ------------------------------------------------------------------------------------------------
// Fused form (windows of <= 64 hop blocks): the 128 x 32-complex-column tile of P never leaves the
// workgroup.  After the K loop the accumulators go to LDS (aliasing the staging buffers), the doubling
// tree runs there, and only X_f for the tile's 128 - Nb + 1 complete frames is written.  Row tiles of a
// group therefore advance by S_g = 129 - Nb_g blocks (1.02x ... 1.97x recomputation of the GEMM rows,
// +20 % MFMA work at 48 kHz / hop 256) in exchange for dropping the P round trip through memory
// (172 MB written + ~200 MB read per 32 768 frames) and the separate combine launch.
// ------------------------------------------------------------------------------------------------
// Many streams in one launch: SegDev / XTile (blockdft_plan.hpp).  segs == nullptr: one segment described by the kernel arguments
// themselves (the single-stream entry points).

struct GemmTreeArgs {
    const float* pcm_base;
    unsigned pcm_bytes;
    const float* E;           // [K][Ntot], (cos, sin) of e^{-i th_c u_m} interleaved per column; the fp32 form reads rows m < K/2
    int ld;                   // Ntot
    float2* X;                // frame-tile blocked: X[((frame / 64) * xcp + col) * 64 + frame % 64]
    float2* Y;                // same layout, 64-block partial sums of the groups whose windows span more than 64 blocks
    int xcp;                  // columns per frame tile (incl. the zeroed pad columns)
    int n_frames;             // frames of this launch
    int K;                    // hop
    long long base;           // index, relative to pcm_base, of the end of frame 0 of this launch
    int n_groups;
    const int4* tile_list;    // (group, column tile in the group, first frame, position) per tile — frame-stripe order in eight queues, see launch
    const BlockGroup* groups;
    BlockGroup gv[8];         // the same descriptors by value (the fused path takes at most 8 window groups): read from the kernel argument segment, not through a second dependent memory round trip
    const float2* comb_tw;
    const __bf16* Et;         // [3][Ntot][K] hi/mid/lo planes of E^T (split-bf16 form only)
    const float4* E16;        // [column tile][k < K / 2][n < 16]: (cos c_n, cos c_{n+16}, -sin c_n, -sin c_{n+16}): B operands of the 16x16x4 fp32 form
    unsigned long long* stamps;   // developer knob PVQ_STAMPS: [workgroup][8] 100 MHz clock: 0 start, 1 after K loop, 2 after tree, 3 end, 4 all waves past the K loop, 5 P tile in LDS, 6 register levels done
    unsigned long long* clk;      // profiling only (pvq_vqt_set_profiling): every 64th workgroup stores (shader clock, 100 MHz clock) before and after its K loop
    const SegDev* segs;           // many-streams launches: the segment table (nullptr: one segment = the arguments above)
    // general hops (blockdft_gemm_gen)
    const float4* E16R;           // per group and column tile: [k < rem / 2][n < 16], as E16
    const float2* gen_tw;         // per group: phi_c = e^{-2 pi i c hop / W} and tau_c (see the kernel), n_tiles * 32 columns each
    int gen_kind;                 // 1: remainder tiles (R' -> Y, or -> X for windows shorter than the hop); 2: whole-block tiles (Q', combined, + tau R' -> X)
#ifdef PVQ_DEV_KNOBS
    int tree_tail;                // developer knob PVQ_TREE_TAIL: 0 = a tile's last tree levels as an LDS pass of their own before the store (the former epilogue)
#endif
};

// which (group, row tile, column tile) a workgroup of the fused kernels owns
struct FusedTile {
    BlockGroup G;
    int S;        // complete frames per row tile
    int ntl, nt;  // column tile within the group / global
    int f0;       // first frame == first block row
    int nfr;      // rows this group produces: n_frames complete frames, or n_frames + nb - 64 partial sums when nb > 64
    int xt0, yt0; // first 64-frame tile of the tile's segment in X / Y (0 in a single-stream launch)
};
// the stream a tile reads and where its frames go: the kernel arguments, or the tile's entry of the segment table
struct TileStream {
    const float* pcm_base;
    unsigned pcm_bytes;
    long long base;
    int n_frames, xt0, yt0;
};
__device__ __forceinline__ TileStream tile_stream(const GemmTreeArgs& a, int entry_x) {
    TileStream ts{a.pcm_base, a.pcm_bytes, a.base, a.n_frames, 0, 0};
    if (a.segs) {
        // The entry is the same for every lane, but the compiler cannot know that of loaded data: without the readfirstlanes the
        // buffer resource built from it counts as lane-dependent and EVERY operand load of the K loop is wrapped in a waterfall loop.
        const int4* sp = reinterpret_cast<const int4*>(a.segs + ((unsigned)entry_x >> 16));
        const int4 lo = sp[0], hi = sp[1];   // (pcm_off, base), (pcm_bytes, n_frames, x_tile0, y_tile0)
        auto rfl = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
        const long long pcm_off = (long long)(((unsigned long long)(unsigned)rfl(lo.y) << 32) | (unsigned)rfl(lo.x));
        ts.pcm_base = a.pcm_base + pcm_off;
        ts.base = (long long)(((unsigned long long)(unsigned)rfl(lo.w) << 32) | (unsigned)rfl(lo.z));
        ts.pcm_bytes = (unsigned)rfl(hi.x);
        ts.n_frames = rfl(hi.y);
        ts.xt0 = rfl(hi.z);
        ts.yt0 = rfl(hi.w);
    }
    return ts;
}
template <int BM = FT_BM>
__device__ __forceinline__ FusedTile fused_tile_of(const GemmTreeArgs& a, const int4& e, const TileStream& ts) {   // tile list entry: (group, column tile, first frame, slot)
    FusedTile t;
    t.G = a.gv[e.x];
    t.S = BM - t.G.nb_f + 1;
    t.nfr = ts.n_frames + t.G.nb - t.G.nb_f;
    t.xt0 = ts.xt0;
    t.yt0 = ts.yt0;
    t.ntl = e.y;
    t.f0 = e.z;
    t.nt = t.G.tile0 + t.ntl;
    return t;
}
template <int BM = FT_BM>
__device__ __forceinline__ FusedTile fused_tile(const GemmTreeArgs& a, TileStream& ts) {   // (the kernels of 32-column tiles: their lists carry no wide entries)
    int4 e = a.tile_list[blockIdx.x];
    ts = tile_stream(a, e.x);
    e.x &= 7;
    return fused_tile_of<BM>(a, e, ts);
}

// doubling tree over the [128][32 complex] P tile in LDS (rows padded to 33 so that the transposed store
// below is bank-conflict free), then the store of the S complete frames, column-major
constexpr int FT_LDP = CB_C + 1;                      // P tile row stride in complex elements
// the tile's combine twiddles (levels x 32 columns) into LDS, issued before the K loop so the tree never waits on memory
constexpr int FT_MAXL = 6;
__device__ __forceinline__ void fused_stage_twiddles(float2 (*tw)[CB_C], const FusedTile& t, const GemmTreeArgs& a, int tid) {
    const int l = tid >> 5, c = tid & (CB_C - 1);
    if (l < t.G.levels_f) tw[l][c] = a.comb_tw[t.G.tw_off + l * (t.G.n_tiles * CB_C) + t.ntl * CB_C + c];
}

// lo + w * hi with a fixed operation order — (re, im) = fma((-w.y, w.y), (hi.y, hi.x), fma((w.x, w.x), (hi.x, hi.y), lo)),
// two packed fp32 fmas (v_pk_fma_f32): every tree level, whichever code path evaluates it, rounds identically, so a
// frame's result does not depend on where it sits in a tile
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 tree_cmadd(float2 lo, float2 w, float2 hi) {
    const f32x2 t = __builtin_elementwise_fma((f32x2){w.x, w.x}, (f32x2){hi.x, hi.y}, (f32x2){lo.x, lo.y});
    const f32x2 r = __builtin_elementwise_fma((f32x2){-w.y, w.y}, (f32x2){hi.y, hi.x}, t);
    return make_float2(r.x, r.y);
}

// the first R <= 4 tree levels (strides 1 .. 8) in registers: a thread owns 16 consecutive rows of one column and
// reads them plus the 2^R - 1 rows above once; every A_{l+1}[j] = A_l[j] + w_l A_l[j + 2^l] is evaluated exactly as
// the level-by-level form would, without a pass through LDS per level.  Rows past the tile read as zero: they only
// feed outputs that are themselves incomplete.
// MIXED (a mixed tile: columns [0, n1) of one window group, the rest of another with its own twiddle table tw2 and r2 <= R register
// levels): a column of the second part takes the levels l < r2 and keeps its values past them — by select, never by a zero twiddle
// (0 * Inf must not appear where the group's own tree has none).
template <int R, int BM, bool MIXED = false>
__device__ __forceinline__ void fused_tree_register_levels(float2 (*A)[CB_C + 1], const float2 (*tw)[CB_C], int tid, int n1 = 0, int r2 = 0,
                                                           const float2 (*tw2)[CB_C] = nullptr) {
    constexpr int H = (1 << R) - 1;
    const int c = tid & (CB_C - 1), j0 = (tid >> 5) * 16;
    const bool p2 = MIXED && c >= n1;
    const float2* twc = p2 ? &tw2[0][c - n1] : &tw[0][c];   // level l: + l * CB_C
    const int rc = p2 ? r2 : R;
    float2 v[16 + H];
#pragma unroll
    for (int i = 0; i < 16 + H; ++i) v[i] = A[j0 + i][c];   // rows BM .. BM + 14 are spare rows of the tile (zeroed by the caller)
    int len = 16 + H;
#pragma unroll
    for (int l = 0; l < R; ++l) {
        const int st = 1 << l;
        const float2 w = MIXED ? twc[l * CB_C] : tw[l][c];
        const bool on = !MIXED || l < rc;
        len -= st;
#pragma unroll
        for (int i = 0; i < 16 + H; ++i)
            if (i < len) {
                const float2 t = tree_cmadd(v[i], w, v[i + st]);
                v[i] = on ? t : v[i];
            }
    }
    __syncthreads();   // every thread has read its halo
#pragma unroll
    for (int i = 0; i < 16; ++i) A[j0 + i][c] = v[i];
    __syncthreads();
}

constexpr int FT_REGL = 4;   // tree levels evaluated in registers; a tile has at most FT_MAXL - FT_REGL = 2 more (CB_MAX_NB = 64 blocks)
#ifdef PVQ_DEV_KNOBS
// PVQ_TREE_TAIL=0 (A/B, bit identity): the former epilogue — the levels past the register ones (strides >= 16) as a pass of their own
// through LDS: read, barrier, write back, barrier; two levels in one pass, outputs in groups of four to bound the registers.  The
// store then only copies.
template <int BM>
__device__ __forceinline__ void fused_tree_lds_levels(float2 (*A)[CB_C + 1], const float2 (*tw)[CB_C], int l, int levels, int tid) {
    const int c = tid & (CB_C - 1);
    constexpr int THREADS = 2 * BM;
    constexpr int PER = BM * CB_C / THREADS;  // 16
    auto cmadd = [](float2 lo, float2 w, float2 hi) { return tree_cmadd(lo, w, hi); };
    int valid = BM - ((1 << l) - 1);
    for (; l + 1 < levels; l += 2) {
        const int st = 1 << l;
        const float2 w1 = tw[l][c], w2 = tw[l + 1][c];
        valid -= 3 * st;
        float2 v[PER];
#pragma unroll
        for (int g = 0; g < PER; g += 4) {
#pragma unroll
            for (int q = g; q < g + 4; ++q) {
                const int j = (tid + q * THREADS) / CB_C;
                if (j < valid) {
                    const float2 t0 = cmadd(A[j][c], w1, A[j + st][c]);
                    const float2 t1 = cmadd(A[j + 2 * st][c], w1, A[j + 3 * st][c]);
                    v[q] = cmadd(t0, w2, t1);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = (tid + q * THREADS) / CB_C;
            if (j < valid) A[j][c] = v[q];
        }
        __syncthreads();
    }
    for (; l < levels; ++l) {
        const int st = 1 << l;
        valid -= st;
        const float2 w = tw[l][c];
        float2 v[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = (tid + q * THREADS) / CB_C;
            if (j < valid) v[q] = cmadd(A[j][c], w, A[j + st][c]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = (tid + q * THREADS) / CB_C;
            if (j < valid) A[j][c] = v[q];
        }
        __syncthreads();
    }
}
#endif

// the tree levels that leave their results in LDS: the register levels.  Returns how many levels (0, 1 or 2) the store still has to evaluate
template <int BM = FT_BM>   // BM rows, 2 * BM threads
__device__ __forceinline__ int fused_tree_levels(float* smem, const float2 (*tw)[CB_C], const FusedTile& t, const GemmTreeArgs& a, int tid, int stamp_slot) {
    float2 (*A)[FT_LDP] = reinterpret_cast<float2 (*)[FT_LDP]>(smem);  // [BM][33]
    const int levels = t.G.levels_f;
    const int l = levels < FT_REGL ? levels : FT_REGL;
    switch (l) {   // wave-uniform
        case 1: fused_tree_register_levels<1, BM>(A, tw, tid); break;
        case 2: fused_tree_register_levels<2, BM>(A, tw, tid); break;
        case 3: fused_tree_register_levels<3, BM>(A, tw, tid); break;
        case 4: fused_tree_register_levels<4, BM>(A, tw, tid); break;
        default: break;
    }
    PVQ_STAMP(6);
    int tail = levels - l;
#ifdef PVQ_DEV_KNOBS
    if (!a.tree_tail) {
        fused_tree_lds_levels<BM>(A, tw, l, levels, tid);
        tail = 0;
    }
#endif
    PVQ_STAMP(2);
    return tail;
}
// the tile's S complete frames to X (or Y): lanes walk the frames of one column: 512-byte runs in memory, conflict-free LDS reads.
// The tile's last `tail` tree levels (strides 16, 32) are evaluated here, on the way from LDS to memory: row j of the result needs
// rows j, j + 16 (, j + 32, j + 48) of the register levels' output in its own column, so no value has to change threads — no
// write-back, no barrier and no second read.  The same calls in the same order as a level-by-level pass (two levels: exactly as two
// radix-2 levels), the twiddles wave-uniform.  j < S = BM - nb_f + 1 keeps every read inside the tile's BM rows.
// (the column loop: row j of the tile's columns col0 .. col0 + ncv - 1 to dst, dst[cc * 64] taking column col0 + cc; tw: the twiddles of those columns)
template <int BM>
__device__ __forceinline__ void fused_store_cols(float* smem, const float2 (*tw)[CB_C], float2* dst, int col0, int ncv, int j, int tid, int tail) {
    float2 (*A)[FT_LDP] = reinterpret_cast<float2 (*)[FT_LDP]>(smem);  // [BM][33]
    // streamed out (non-temporal): the kernel-product stage that reads X back runs 5 % faster for it
    auto put = [&](int cc, float2 val) { __builtin_nontemporal_store((f32x2){val.x, val.y}, reinterpret_cast<f32x2*>(&dst[cc * 64])); };   // one 8-byte store
    constexpr int st = 1 << FT_REGL;
    if (tail == 2) {   // wave-uniform
#pragma unroll 4
        for (int cc = tid / BM; cc < ncv; cc += 2) {
            const float2 w1 = tw[FT_REGL][cc], w2 = tw[FT_REGL + 1][cc];
            const float2 t0 = tree_cmadd(A[j][col0 + cc], w1, A[j + st][col0 + cc]);
            const float2 t1 = tree_cmadd(A[j + 2 * st][col0 + cc], w1, A[j + 3 * st][col0 + cc]);
            put(cc, tree_cmadd(t0, w2, t1));
        }
    } else if (tail == 1) {
#pragma unroll 4
        for (int cc = tid / BM; cc < ncv; cc += 2) put(cc, tree_cmadd(A[j][col0 + cc], tw[FT_REGL][cc], A[j + st][col0 + cc]));
    } else {
#pragma unroll 4
        for (int cc = tid / BM; cc < ncv; cc += 2) put(cc, A[j][col0 + cc]);
    }
}
template <int BM = FT_BM>
__device__ __forceinline__ void fused_store_x(float* smem, const float2 (*tw)[CB_C], const FusedTile& t, const GemmTreeArgs& a, int tid, int tail) {
    const int j = tid % BM;
    const int f = t.f0 + j;
    if (j < t.S && f < t.nfr) {
        // windows of more than 64 blocks: 64-block partial sums go to Y, blockdft_tree_finish adds the last levels
        const bool to_y = t.G.nb > t.G.nb_f;
        float2* dst = (to_y ? a.Y : a.X) + ((size_t)((f >> 6) + (to_y ? t.yt0 : t.xt0)) * a.xcp + t.nt * CB_C) * 64 + (f & 63);
        const int ncv = t.G.n_cols - t.ntl * CB_C < CB_C ? t.G.n_cols - t.ntl * CB_C : CB_C;   // the tile's real columns: the padding of a group's last tile is never read with a non-zero coefficient and never written (X starts out zeroed)
        fused_store_cols<BM>(smem, tw, dst, 0, ncv, j, tid, tail);
    }
}
template <int BM = FT_BM>
__device__ __forceinline__ void fused_tree_store(float* smem, const float2 (*tw)[CB_C], const FusedTile& t, const GemmTreeArgs& a, int tid, int stamp_slot) {
    const int tail = fused_tree_levels<BM>(smem, tw, t, a, tid, stamp_slot);
    fused_store_x<BM>(smem, tw, t, a, tid, tail);
    if (a.stamps) {
        __builtin_amdgcn_s_waitcnt(0);   // stores issued and acknowledged
        __syncthreads();
        PVQ_STAMP(3);
    }
}

// A MIXED tile's epilogue (blockdft_plan.hpp: MixedPair): columns [0, n1) of the P tile are the last column tile of t's group, columns
// [n1, n1 + n2) the last column tile of a second group t2 of fewer hop blocks, whose frame t2.f0 + j sits in row j; tw[0] / tw[1] hold
// the two parts' twiddles.  Each column runs its own group's levels — the same tree_cmadd calls as in a tile of its own — and each part
// goes to the X columns it always had.  The rows advance by t's stride, so the second part stores rows j < t.S too, those of its frames
// that exist (its first frame index is negative where its windows begin later than t's at a stream's start).
template <int BM>
__device__ __forceinline__ void fused_tree_store_mixed(float* smem, const float2 (*tw)[FT_MAXL][CB_C], const FusedTile& t, const FusedTile& t2, int n1, int n2,
                                                       const GemmTreeArgs& a, int tid, int stamp_slot) {
    float2 (*A)[FT_LDP] = reinterpret_cast<float2 (*)[FT_LDP]>(smem);  // [BM][33]
    const int l1 = t.G.levels_f < FT_REGL ? t.G.levels_f : FT_REGL, l2 = t2.G.levels_f < FT_REGL ? t2.G.levels_f : FT_REGL;   // l2 <= l1
    switch (l1) {   // wave-uniform
        case 1: fused_tree_register_levels<1, BM, true>(A, tw[0], tid, n1, l2, tw[1]); break;
        case 2: fused_tree_register_levels<2, BM, true>(A, tw[0], tid, n1, l2, tw[1]); break;
        case 3: fused_tree_register_levels<3, BM, true>(A, tw[0], tid, n1, l2, tw[1]); break;
        case 4: fused_tree_register_levels<4, BM, true>(A, tw[0], tid, n1, l2, tw[1]); break;
        default: break;
    }
    PVQ_STAMP(6);
    PVQ_STAMP(2);
    const int j = tid % BM;
    if (j < t.S) {
        const int f1 = t.f0 + j, f2 = t2.f0 + j;
        if (f1 < t.nfr)
            fused_store_cols<BM>(smem, tw[0], a.X + ((size_t)((f1 >> 6) + t.xt0) * a.xcp + t.nt * CB_C) * 64 + (f1 & 63), 0, n1, j, tid, t.G.levels_f - l1);
        if (f2 >= 0 && f2 < t2.nfr)
            fused_store_cols<BM>(smem, tw[1], a.X + ((size_t)((f2 >> 6) + t2.xt0) * a.xcp + t2.nt * CB_C) * 64 + (f2 & 63), n1, n2, j, tid, t2.G.levels_f - l2);
    }
    if (a.stamps) {
        __builtin_amdgcn_s_waitcnt(0);   // stores issued and acknowledged
        __syncthreads();
        PVQ_STAMP(3);
    }
}

// fp32 MFMA form.  The hop DFT is evaluated about the centre of the hop block: with u_m = m - (K-1)/2,
//     P'[j][c] = sum_{m < K/2} (x[m] + x[K-1-m]) cos(th_c u_m)  +  i sum_{m < K/2} (x[m] - x[K-1-m]) (-sin(th_c u_m))
// (cos is even, sin odd about the centre), i.e. two real GEMMs of depth K/2 — the real parts from the mirrored sums,
// the imaginary parts from the mirrored differences — instead of one of depth K: half the MFMA work, exactly.
// P = rho_c P' with rho_c = e^{-i th_c (K-1)/2}; the tree is linear per column, so X = rho_c X' and the constant
// phase is folded into the kernel-product coefficients on the host (prepare_blockdft).
//
// The PCM matrix goes from memory straight into MFMA operand registers, no LDS staging and no barrier in the K loop:
// a wave owns 32 block rows x all 32 complex columns of the tile; lane (row = lane & 31, half = lane >> 5) fetches
// the 16 consecutive samples k0 + 16 half .. + 15 of its row and the 16 mirrored ones (64-byte runs: every cache line
// it touches is consumed by four back-to-back loads), forms the 16 sums and 16 differences in registers, and these
// ARE the A operands of 16 v_mfma_f32_32x32x2_f32 pairs (k order within a stage: k0 + 16 half + t; any order works
// as long as the B rows follow it).  acc0 += sums x cosines, acc1 += differences x (-sines).  The tile's slice of E
// (rows m < K/2, (cos, -sin) interleaved) is staged into LDS once per 128 rows of K/2 and read as one b64 per pair.
constexpr int FR_KC = 128;   // rows of E staged per pass (32 KB)
// idx_f / idx_b: sample index (relative to pcm_base) of the lane's front run and of its mirrored run
template <bool VEC>
__device__ __forceinline__ void fused_f32_stage_load(const i32x4& rsrc4, __amdgpu_buffer_rsrc_t rsrc, long long idx_f, long long idx_b,
                                                     float (&fr)[16], float (&bk)[16]) {
    if (VEC) {   // the whole tile lies inside the stream: offsets are plain non-negative byte offsets
        const unsigned off_f = (unsigned)(idx_f * 4ll), off_b = (unsigned)(idx_b * 4ll);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = pvq_raw_buffer_load_f32x4(rsrc4, (int)(off_f + 16u * q), 0, 0);
            const f32x4 w = pvq_raw_buffer_load_f32x4(rsrc4, (int)(off_b + 16u * q), 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fr[4 * q + i] = v[i];
                bk[4 * q + i] = w[i];
            }
        }
    } else {
        // tiles that touch the stream start / end: samples before the stream get an explicit out-of-range offset
        // (a wrapped negative offset plus the instruction's immediate offset would not wrap in the hardware's range
        // check), samples past the end are zeroed by the range check itself
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long jf = idx_f + q, jb = idx_b + q;
            const unsigned of = jf >= 0 ? (unsigned)(jf * 4ll) : 0xFFFFFFFCu;
            const unsigned ob = jb >= 0 ? (unsigned)(jb * 4ll) : 0xFFFFFFFCu;
            fr[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, of, 0, 0));
            bk[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, ob, 0, 0));
        }
    }
}

template <bool VEC, int BM, typename Args>
__device__ __forceinline__ void fused_f32_kloop(const Args& a, float* smem, long long idx_f0, long long idx_b0, const float* e_tile,
                                                int tid, f32x16& acc0, f32x16& acc1) {
    constexpr int THREADS = 2 * BM;
    const int lane = tid & 63;
    const unsigned long long pcm_addr = reinterpret_cast<unsigned long long>(a.pcm_base);
    const i32x4 rsrc4 = {(int)(unsigned)pcm_addr, (int)(unsigned)(pcm_addr >> 32), (int)a.pcm_bytes, 0x00020000};
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.pcm_base), 0, a.pcm_bytes, 0x00020000);
    const int K2 = a.K / 2;
    const float2* bsl = reinterpret_cast<const float2*>(smem) + (lane >> 5) * 16 * CB_C + (lane & 31);   // row 16 half, column lane & 31
    float fr[16], bk[16];
    for (int kc = 0; kc < K2; kc += FR_KC) {
        const int rows = K2 - kc < FR_KC ? K2 - kc : FR_KC;
        fused_f32_stage_load<VEC>(rsrc4, rsrc, idx_f0 + kc, idx_b0 - kc, fr, bk);
        if (kc > 0) __syncthreads();   // every wave is done with the previous slice
        for (int i = tid; i < rows * (FT_BN / 4); i += THREADS) {
            const int r = i / (FT_BN / 4), c4 = i % (FT_BN / 4);
            *reinterpret_cast<float4*>(smem + r * FT_BN + c4 * 4) = *reinterpret_cast<const float4*>(e_tile + (size_t)(kc + r) * a.ld + c4 * 4);
        }
        __syncthreads();
        for (int k0 = 0; k0 < rows; k0 += 32) {
            float sm[16], df[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                sm[t] = fr[t] + bk[15 - t];
                df[t] = fr[t] - bk[15 - t];
            }
            if (k0 + 32 < rows)
                fused_f32_stage_load<VEC>(rsrc4, rsrc, idx_f0 + (kc + k0 + 32), idx_b0 - (kc + k0 + 32), fr, bk);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float2 b = bsl[(k0 + t) * CB_C];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sm[t], b.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(df[t], b.y, acc1, 0, 0, 0);
            }
        }
    }
}

// The same mirrored GEMM on v_mfma_f32_16x16x4_f32 (the form blockdft_gemm_tree runs).  A wave still owns 32 block rows x 32
// complex columns (two 16-row tiles x (re, im) x two 16-column halves = 8 accumulators of 4 registers), but lane
// (row = lane & 15, kq = lane >> 4) now fetches 4 consecutive samples of its row and the 4 mirrored ones with ONE 16-byte load
// each: the four lanes of a row read one contiguous 64-byte run, 16 cache lines per load instruction where the 32x32x2 form's
// lanes touch 64 — its address processing took as long as its MFMAs (16 vs 15.6 us per workgroup pair), which is what held a
// workgroup running its K loop alone (its CU partner in its tree / store phase) at 63 % of the matrix pipe.  MFMA t of a k
// group (16 mirrored sample pairs) takes sample 4 kq + t of every lane; B operand of lane (n, kq): row 16 g + 4 kq + t of the
// E slice, (cos c_n, cos c_{n+16}, -sin c_n, -sin c_{n+16}) as one 16-byte LDS read.  Operands double-buffered, one k group ahead.
typedef float f32x4a __attribute__((ext_vector_type(4)));
template <int BM, bool HALF>   // tiles that lie wholly inside the stream (all but a handful per launch); HALF: at most 16 columns (a group's last tile): the second 16-column half is not computed
// depth: samples of a row the DFT runs over (the hop; the general-hop kernel's second GEMM runs over the first `rem` samples of rows that
// still lie a.K = hop samples apart)
__device__ __forceinline__ void fused_f32_kloop16(const GemmTreeArgs& a, const float* pcm_base, unsigned pcm_bytes, float* smem, long long tile_lo, const float4* e_tile, int tid,
                                                  f32x4a (&accR)[2][2], f32x4a (&accI)[2][2], const float* tw_src, float* tw_dst, int tw_levels, int tw_stride, int stamp_slot, int depth,
                                                  const float* tw_src2 = nullptr, int tw_levels2 = 0, int tw_stride2 = 0) {   // (a mixed tile: its second part's twiddles, into the second table)
    constexpr int THREADS = 2 * BM;
    const int lane = tid & 63, wave = tid >> 6, m16 = lane & 15, kq = lane >> 4;
    const unsigned long long pcm_addr = reinterpret_cast<unsigned long long>(pcm_base);
    const i32x4 rsrc4 = {(int)(unsigned)pcm_addr, (int)(unsigned)(pcm_addr >> 32), (int)pcm_bytes, 0x00020000};
    const int K2 = depth / 2;
    const int nG = K2 / 32;   // (K2 is a multiple of 32: the fused path takes hops that are multiples of 64)
    // A load step fetches a DOUBLE k group (32 mirrored sample pairs): lane (row, kq) takes the 8 consecutive samples 32 G + 8 kq ...
    // of its row and the 8 mirrored ones, two 16-byte loads each, issued back to back — the four lanes of a row read one whole
    // 128-byte line at a time.  Fetched 16 pairs at a time (one 64-byte half line per step, the other half a step later) every line
    // crossed the L2 -> L1 path twice: by then the CU's other waves had pushed it out of the L1 again, and the K loop ran at the
    // L2's 64-66 GB/s per CU, not at the matrix pipe's rate.  MFMA t of half h of double group G takes sample
    // 32 G + 8 kq + 4 h + t of every lane; the B rows follow that order.
    // Addresses: one loop-invariant byte offset per lane, row tile and direction; the double group moves in the instruction's
    // SCALAR offset (front runs + 128 G bytes; the mirrored runs are anchored at the LAST double group and take + 128 (nG - 1 - G)).
    unsigned vf[2], vb[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const long long row_lo = tile_lo + (long long)(wave * 32 + mt * 16 + m16) * a.K;
        vf[mt] = (unsigned)((row_lo + 8 * kq) * 4ll);
        vb[mt] = (unsigned)((row_lo + depth - 8 - 8 * kq) * 4ll) - 128u * (unsigned)(nG - 1);
    }
    float fr[2][2][8], bk[2][2][8];
    // The prefetch is UNCONDITIONAL (the group index is clamped: past the last group the last one is fetched again into the idle
    // buffer).  Inside a uniform `if` the compiler must place the s_waitcnt for the path on which the loads were NOT issued: it waited
    // for vmcnt(4), then vmcnt(0) right after issuing the eight loads of the next group, i.e. for the loads it had just issued — the
    // K loop ran with no prefetch distance at all, hidden only while a CU's other workgroup had its own K loop to run.
    auto load_dgroup = [&](int buf, int G) {   // G: double k group of the whole depth
        const int Gc = G < nG - 1 ? G : nG - 1;
        const int sf = 128 * Gc, sb = 128 * (nG - 1 - Gc);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 v = pvq_raw_buffer_load_f32x4(rsrc4, (int)vf[mt], sf + 16 * h, 0);   // (the half's 16 bytes ride in the scalar offset too: one address register per run)
                const f32x4 w = pvq_raw_buffer_load_f32x4(rsrc4, (int)vb[mt], sb + 16 * h, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    fr[buf][mt][4 * h + t] = v[t];
                    bk[buf][mt][4 * h + t] = w[t];
                }
            }
        }
    };
    float4* El = reinterpret_cast<float4*>(smem);   // [rows][16]
    // one k row = 8 MFMAs; its B operand (one 16-byte LDS read per lane) is fetched one row ahead, so that no MFMA waits on the LDS
    const float4* erow = El + (8 * kq) * 16 + m16;   // row 32 Gl + 8 kq + 4 h + t of the staged slice
    auto b_at = [&](int Gl, int h, int t) { return erow[(32 * Gl + 4 * h + t) * 16]; };
    auto mfma_row = [&](int buf, int h, int t, const float4& b) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float sm = fr[buf][mt][4 * h + t] + bk[buf][mt][7 - 4 * h - t];
            const float df = fr[buf][mt][4 * h + t] - bk[buf][mt][7 - 4 * h - t];
            accR[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm, b.x, accR[mt][0], 0, 0, 0);
            if (!HALF) accR[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm, b.y, accR[mt][1], 0, 0, 0);
            accI[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(df, b.z, accI[mt][0], 0, 0, 0);
            if (!HALF) accI[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(df, b.w, accI[mt][1], 0, 0, 0);
        }
    };
    // the 8 k rows of double group Gl from operand buffer `buf`; bc: the first row's B operand (already fetched), returns the next group's
    auto mfma_dgroup = [&](int buf, int Gl, float4 bc) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int h = r >> 2, t = r & 3;
            // (past the slice's last row this reads on into the workgroup's LDS region: in bounds, never used)
            const float4 bn = r < 7 ? b_at(Gl, (r + 1) >> 2, (r + 1) & 3) : b_at(Gl + 1, 0, 0);
            __builtin_amdgcn_sched_barrier(0);   // the next row's read is in flight before this row's MFMAs
            mfma_row(buf, h, t, bc);
            __builtin_amdgcn_sched_barrier(0);
            bc = bn;
        }
        return bc;
    };
    // The slice of E goes straight to LDS (LDS-DMA, 1 KB per wave instruction, no registers), issued ahead of the first operand
    // loads: ONE memory round trip before the first MFMA.  (As a load -> wait -> ds_write loop it was four dependent round
    // trips, each also waiting for the operand loads issued before it, behind two more for the tile's twiddles and descriptor.)
    auto stage_e = [&](int kc, int rows) {   // 1 KB pieces of the slice (rows x 256 bytes), dealt to the waves; a full slice unrolled: all pieces in flight together
        constexpr int NWV = THREADS / 64, FULL = FR_KC / 4 / NWV;
        const float4* src = e_tile + (size_t)kc * 16 + wave * 64 + lane;
        float4* dst = El + wave * 64;
        if (rows == FR_KC && FR_KC / 4 % NWV == 0) {
#pragma unroll
            for (int q = 0; q < FULL; ++q) lds_dma16(src + q * (NWV * 64), dst + q * (NWV * 64));
        } else {
            for (int j = wave; j < rows / 4; j += NWV) lds_dma16(e_tile + (size_t)kc * 16 + j * 64 + lane, El + j * 64);
        }
    };
    stage_e(0, K2 < FR_KC ? K2 : FR_KC);
    for (int l = wave; l < tw_levels; l += THREADS / 64)   // the tile's combine twiddles: one level (32 complex = 64 floats) per wave instruction
        lds_dma4(tw_src + (size_t)l * tw_stride, tw_dst + l * (2 * CB_C));
    for (int l = wave; l < tw_levels2; l += THREADS / 64)
        lds_dma4(tw_src2 + (size_t)l * tw_stride2, tw_dst + (FT_MAXL + l) * (2 * CB_C));
    load_dgroup(0, 0);
    // (one wait for everything the prologue fetched.  Waiting only for the DMA pieces — s_waitcnt vmcnt(8) + a raw s_barrier — lets a
    // wave start on its own first operands, but hipcc does not credit a hand-written wait: with an LDS-DMA "possibly in flight" it
    // waits vmcnt(0) at the first use of every later load, which takes the K loop's prefetch distance away again.)
    __syncthreads();
    PVQ_STAMP(7);
    for (int kc = 0; kc < K2; kc += FR_KC) {
        const int rows = K2 - kc < FR_KC ? K2 - kc : FR_KC;
        if (kc > 0) {   // (hops of 512 and more: the next slice of E replaces the one every wave is done with)
            __syncthreads();
            stage_e(kc, rows);
            __syncthreads();
        }
        const int ng = rows / 32, G0 = kc / 32;
        float4 bc = b_at(0, 0, 0);
        for (int Gl = 0; Gl < ng; Gl += 2) {   // two double groups per pass: buffer indices stay compile-time
            load_dgroup(1, G0 + Gl + 1);
            bc = mfma_dgroup(0, Gl, bc);
            if (Gl + 1 >= ng) break;           // (a 32-row slice: hop 64)
            load_dgroup(0, G0 + Gl + 2);
            bc = mfma_dgroup(1, Gl + 1, bc);
        }
    }
}

// The same loop for the tiles that touch the stream's start or end (dword loads, each range-checked by the buffer hardware;
// samples before the stream get an explicit out-of-range offset, see fused_f32_stage_load): same MFMAs on the same samples in
// the same order — k group g = 2 G + h — but one 16-pair half of a double group per load step, which keeps its 32 dword loads
// per step inside the register budget.
template <int BM>
__device__ __forceinline__ void fused_f32_kloop16_edge(const GemmTreeArgs& a, const float* pcm_base, unsigned pcm_bytes, float* smem, long long tile_lo, const float4* e_tile, int tid,
                                                       f32x4a (&accR)[2][2], f32x4a (&accI)[2][2], const float* tw_src, float* tw_dst, int tw_levels, int tw_stride, int stamp_slot, int depth) {
    constexpr int THREADS = 2 * BM;
    const int lane = tid & 63, wave = tid >> 6, m16 = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pcm_base), 0, pcm_bytes, 0x00020000);
    const int K2 = depth / 2;
    int jf0[2], jb0[2];   // sample indices relative to pcm_base (|.| < 2^30: the launch's stream is at most 4 GB)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int row_lo = (int)tile_lo + (wave * 32 + mt * 16 + m16) * a.K;
        jf0[mt] = row_lo + 8 * kq;
        jb0[mt] = row_lo + depth - 4 - 8 * kq;
    }
    float fr[2][2][4], bk[2][2][4];
    auto load_group = [&](int buf, int g) {
        const int so = 32 * (g >> 1) + 4 * (g & 1);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int xf = jf0[mt] + so + t, xb = jb0[mt] - so + t;
                fr[buf][mt][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, xf >= 0 ? (unsigned)xf * 4u : 0xFFFFFFFCu, 0, 0));
                bk[buf][mt][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, xb >= 0 ? (unsigned)xb * 4u : 0xFFFFFFFCu, 0, 0));
            }
    };
    float4* El = reinterpret_cast<float4*>(smem);   // [rows][16]
    auto mfma_group = [&](int buf, int gl) {        // gl: k group inside the staged slice
        const float4* e = El + (32 * (gl >> 1) + 8 * kq + 4 * (gl & 1)) * 16 + m16;
        float4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = e[t * 16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float sm = fr[buf][mt][t] + bk[buf][mt][3 - t];
                const float df = fr[buf][mt][t] - bk[buf][mt][3 - t];
                accR[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm, b[t].x, accR[mt][0], 0, 0, 0);
                accR[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm, b[t].y, accR[mt][1], 0, 0, 0);
                accI[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(df, b[t].z, accI[mt][0], 0, 0, 0);
                accI[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(df, b[t].w, accI[mt][1], 0, 0, 0);
            }
        }
    };
    load_group(0, 0);
    for (int l = wave; l < tw_levels; l += THREADS / 64) tw_dst[l * (2 * CB_C) + lane] = tw_src[(size_t)l * tw_stride];
    for (int kc = 0; kc < K2; kc += FR_KC) {
        const int rows = K2 - kc < FR_KC ? K2 - kc : FR_KC;
        if (kc > 0) __syncthreads();   // every wave is done with the previous slice
        for (int i = tid; i < rows * 16; i += THREADS) El[i] = e_tile[(size_t)kc * 16 + i];
        __syncthreads();
        const int ng = rows / 16, g0 = kc / 16;
        for (int gl = 0; gl < ng; gl += 2) {   // two k groups per pass: buffer indices stay compile-time (rows is a multiple of 32)
            load_group(1, g0 + gl + 1);
            mfma_group(0, gl);
            if (g0 + gl + 2 < K2 / 16) load_group(0, g0 + gl + 2);
            mfma_group(1, gl + 1);
        }
    }
}

// WIDE tiles: the same rows against TWO neighbouring column tiles (64 complex columns) in one K loop.  What bounds a workgroup is
// not a resource but the chain of latencies a tile pays once — launch gap, descriptor, the first operand burst, the waves' skew at
// the loop's end — so a wide tile pays them once for twice the MFMAs.  A wave holds 16 accumulators (64 registers);
// the A operands are single-buffered per 16-row tile and fetched one STAGE ahead — stage = (row tile, double k group) = 64 MFMAs,
// the same prefetch distance in MFMAs as the narrow loop's double buffer: while row tile 1 of double group G runs, row tile 0's
// loads of group G + 1 are in flight, and so on in turn.  Every accumulator adds the same products in the same order as in the
// narrow loop: results are bit-identical whichever form a tile takes.  The two tiles' slices of E lie 32 KB apart in LDS.
template <int BM>
__device__ __forceinline__ void fused_f32_kloop64(const GemmTreeArgs& a, const float* pcm_base, unsigned pcm_bytes, float* smem, long long tile_lo, const float4* e_tile, int tid,
                                                  f32x4a (&accR)[2][4], f32x4a (&accI)[2][4], const float* tw_src, float* tw_dst, int tw_levels, int tw_stride, int stamp_slot) {
    constexpr int THREADS = 2 * BM, NWV = THREADS / 64;
    const int lane = tid & 63, wave = tid >> 6, m16 = lane & 15, kq = lane >> 4;
    const unsigned long long pcm_addr = reinterpret_cast<unsigned long long>(pcm_base);
    const i32x4 rsrc4 = {(int)(unsigned)pcm_addr, (int)(unsigned)(pcm_addr >> 32), (int)pcm_bytes, 0x00020000};
    const int K2 = a.K / 2;
    const int nG = K2 / 32;
    unsigned vf[2], vb[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const long long row_lo = tile_lo + (long long)(wave * 32 + mt * 16 + m16) * a.K;
        vf[mt] = (unsigned)((row_lo + 8 * kq) * 4ll);
        vb[mt] = (unsigned)((row_lo + a.K - 8 - 8 * kq) * 4ll) - 128u * (unsigned)(nG - 1);
    }
    float fr[2][8], bk[2][8];
    auto load_stage = [&](int mt, int G) {   // unconditional, clamped (see fused_f32_kloop16)
        const int Gc = G < nG - 1 ? G : nG - 1;
        const int sf = 128 * Gc, sb = 128 * (nG - 1 - Gc);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 v = pvq_raw_buffer_load_f32x4(rsrc4, (int)vf[mt], sf + 16 * h, 0);
            const f32x4 w = pvq_raw_buffer_load_f32x4(rsrc4, (int)vb[mt], sb + 16 * h, 0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fr[mt][4 * h + t] = v[t];
                bk[mt][4 * h + t] = w[t];
            }
        }
    };
    float4* El = reinterpret_cast<float4*>(smem);   // [column tile][FR_KC rows][16]
    const float4* erow = El + (8 * kq) * 16 + m16;
    auto b_at = [&](int Gl, int r, int ct) { return erow[(32 * Gl + r) * 16 + ct * (FR_KC * 16)]; };
    // one stage: 8 k rows x 2 column tiles = 16 steps of 4 MFMAs, the B operand fetched one step ahead
    auto mfma_stage = [&](int mt, int Gl, int Gl_next, float4 bc) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = i >> 1, ct = i & 1;
            const float4 bn = i < 15 ? b_at(Gl, (i + 1) >> 1, (i + 1) & 1) : b_at(Gl_next, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            const float sm = fr[mt][r] + bk[mt][7 - r];
            const float df = fr[mt][r] - bk[mt][7 - r];
            accR[mt][2 * ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm, bc.x, accR[mt][2 * ct], 0, 0, 0);
            accR[mt][2 * ct + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(sm, bc.y, accR[mt][2 * ct + 1], 0, 0, 0);
            accI[mt][2 * ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(df, bc.z, accI[mt][2 * ct], 0, 0, 0);
            accI[mt][2 * ct + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(df, bc.w, accI[mt][2 * ct + 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            bc = bn;
        }
        return bc;
    };
    auto stage_e = [&](int kc, int rows) {   // both tiles' slices, 1 KB pieces dealt to the waves
        constexpr int FULL = FR_KC / 4 / NWV;
        if (rows == FR_KC && FR_KC / 4 % NWV == 0) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int q = 0; q < FULL; ++q)
                    lds_dma16(e_tile + (size_t)ct * K2 * 16 + (size_t)kc * 16 + (q * NWV + wave) * 64 + lane, El + ct * (FR_KC * 16) + (q * NWV + wave) * 64);
        } else {
            for (int j = wave; j < 2 * (rows / 4); j += NWV) {
                const int ct = j >= rows / 4, jj = ct ? j - rows / 4 : j;
                lds_dma16(e_tile + (size_t)ct * K2 * 16 + (size_t)kc * 16 + jj * 64 + lane, El + ct * (FR_KC * 16) + jj * 64);
            }
        }
    };
    stage_e(0, K2 < FR_KC ? K2 : FR_KC);
    // twiddles: levels x 64 complex columns = two 64-float pieces per level, [column tile][level][32]
    for (int j = wave; j < 2 * tw_levels; j += NWV) {
        const int l = j >> 1, ct = j & 1;
        lds_dma4(tw_src + (size_t)l * tw_stride + ct * (2 * CB_C), tw_dst + (ct * FT_MAXL + l) * (2 * CB_C));
    }
    load_stage(0, 0);
    load_stage(1, 0);
    __syncthreads();
    PVQ_STAMP(7);
    for (int kc = 0; kc < K2; kc += FR_KC) {
        const int rows = K2 - kc < FR_KC ? K2 - kc : FR_KC;
        if (kc > 0) {
            __syncthreads();
            stage_e(kc, rows);
            __syncthreads();
        }
        const int ng = rows / 32, G0 = kc / 32;
        float4 bc = b_at(0, 0, 0);
        for (int Gl = 0; Gl < ng; ++Gl) {
            bc = mfma_stage(0, Gl, Gl, bc);
            load_stage(0, G0 + Gl + 1);
            bc = mfma_stage(1, Gl, Gl + 1, bc);
            load_stage(1, G0 + Gl + 1);
        }
    }
}

// P' accumulators of one 32-column tile -> LDS as [row][32 complex + pad]  (C/D layout of the 16x16 MFMA: column = lane & 15,
// rows 4 (lane >> 4) + r), and the 15 spare rows zeroed
template <int BM, int NP, int NP0>
__device__ __forceinline__ void fused_dump_p(float* smem, const f32x4a (&accR)[2][NP], const f32x4a (&accI)[2][NP], int tid) {
    float2 (*Pt)[FT_LDP] = reinterpret_cast<float2 (*)[FT_LDP]>(smem);
    const int lane = tid & 63, wave = tid >> 6, m16 = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int np = 0; np < 2; ++np)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Pt[wave * 32 + mt * 16 + 4 * kq + r][np * 16 + m16] = make_float2(accR[mt][NP0 + np][r], accI[mt][NP0 + np][r]);
    for (int i = tid; i < 15 * FT_LDP; i += 2 * BM) Pt[BM][i] = make_float2(0.0f, 0.0f);   // the spare rows (Pt[BM][..] runs on through them)
}

// one 32-column tile from the K loop to the store
// mixed_x: the entry's .x if it is a MIXED one (the host emits them for tiles inside the stream only), else 0; n_frames: the frames of the tile's segment
template <int BM>
__device__ __forceinline__ void fused_f32_narrow_tile(const GemmTreeArgs& a, const float* pcm_base, unsigned pcm_bytes, float* smem, float2 (*tw_lds)[FT_MAXL][CB_C], const FusedTile& T, bool inside,
                                                      long long tile_lo, int tid, int stamp_slot, int mixed_x, int n_frames) {
    const int lane = tid & 63;
    // the tile's combine twiddles (levels x 32 complex columns = 64 floats per level): a wave copies a level, a dword per lane
    const float* tw_src = reinterpret_cast<const float*>(a.comb_tw + T.G.tw_off + T.ntl * CB_C) + lane;   // level l: + l * tw_stride floats
    float* tw_dst = reinterpret_cast<float*>(&tw_lds[0][0][0]);
    const int tw_levels = T.G.levels_f, tw_stride = 2 * T.G.n_tiles * CB_C;
    const bool mixed = mixed_x != 0;   // workgroup-uniform
    const float4* e_tile = a.E16 + (size_t)(mixed ? a.ld / FT_BN + ((mixed_x >> TILE_MIXED_PAIR_SHIFT) & 7) : T.nt) * (a.K / 2) * 16;   // (a pair's merged slice: behind the regular column tiles)
    // a mixed tile's second part: the last column tile of group g2, frame T.f0 + j + d in row j (K is a power of two on this path)
    FusedTile T2 = T;
    int n1 = 0, n2 = 0;
    if (mixed) {
        T2.G = a.gv[(mixed_x >> TILE_MIXED_G2_SHIFT) & 7];
        T2.ntl = T2.G.n_tiles - 1;
        T2.nt = T2.G.tile0 + T2.ntl;
        T2.f0 = T.f0 + (int)((T.G.s_rel - T2.G.s_rel) >> __builtin_ctz(a.K));
        T2.nfr = n_frames;
        n1 = T.G.n_cols - T.ntl * CB_C;
        n2 = T2.G.n_cols - T2.ntl * CB_C;
    }
    const float* tw_src2 = reinterpret_cast<const float*>(a.comb_tw + T2.G.tw_off + T2.ntl * CB_C) + lane;
    const int tw_levels2 = mixed ? T2.G.levels_f : 0, tw_stride2 = 2 * T2.G.n_tiles * CB_C;
    f32x4a accR[2][2], accI[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int np = 0; np < 2; ++np)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                accR[mt][np][r] = 0.0f;
                accI[mt][np][r] = 0.0f;
            }
    // the clock the chip holds under this kernel's MFMA load: shader-clock ticks over 100 MHz ticks across the K loop.  The
    // start stamps go straight to memory so that nothing stays live in registers across the loop
    if (a.clk != nullptr && (blockIdx.x & 63) == 0 && tid == 0) {
        a.clk[(blockIdx.x >> 6) * 4 + 0] = __builtin_amdgcn_s_memtime();
        a.clk[(blockIdx.x >> 6) * 4 + 1] = __builtin_amdgcn_s_memrealtime();
    }
    // a group's last column tile may hold 16 columns or fewer (3 of the 21 tiles at 48 kHz / 252 bins): half the MFMAs
    // (a mixed tile: both parts together)
    const bool half = mixed ? n1 + n2 <= 16 : T.ntl == T.G.n_tiles - 1 && T.G.n_cols - T.ntl * CB_C <= 16;
    if (__builtin_expect(!inside, 0))   // (a handful of tiles per launch)
        fused_f32_kloop16_edge<BM>(a, pcm_base, pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, tw_src, tw_dst, tw_levels, tw_stride, stamp_slot, a.K);
    else if (half)
        fused_f32_kloop16<BM, true>(a, pcm_base, pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, tw_src, tw_dst, tw_levels, tw_stride, stamp_slot, a.K, tw_src2, tw_levels2, tw_stride2);
    else
        fused_f32_kloop16<BM, false>(a, pcm_base, pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, tw_src, tw_dst, tw_levels, tw_stride, stamp_slot, a.K, tw_src2, tw_levels2, tw_stride2);
    if (a.clk != nullptr && (blockIdx.x & 63) == 0 && tid == 0) {
        a.clk[(blockIdx.x >> 6) * 4 + 2] = __builtin_amdgcn_s_memtime();
        a.clk[(blockIdx.x >> 6) * 4 + 3] = __builtin_amdgcn_s_memrealtime();
    }
    PVQ_STAMP(1);
    __syncthreads();   // the E slice is dead: the P' tile takes its place
    PVQ_STAMP(4);
    fused_dump_p<BM, 2, 0>(smem, accR, accI, tid);
    __syncthreads();
    PVQ_STAMP(5);
    if (mixed)
        fused_tree_store_mixed<BM>(smem, tw_lds, T, T2, n1, n2, a, tid, stamp_slot);
    else
        fused_tree_store<BM>(smem, tw_lds[0], T, a, tid, stamp_slot);
}


// three more stamps per workgroup, behind the gridDim.x rows of eight: its first instruction, its last wave's last store issued, and that
// store acknowledged — what lies between one workgroup's last and the next one's first is the dispatcher's (scripts/dev_conc.py)
#define PVQ_END_STAMPS \
    if (a.stamps) { \
        unsigned long long* ends = a.stamps + (size_t)gridDim.x * 8 + (size_t)stamp_slot * 4; \
        if (lane == 0) atomicMax(ends + 1, wall_clock64()); \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
        if (lane == 0) atomicMax(ends + 2, wall_clock64()); \
        if (tid == 0) ends[0] = t_entry; \
    }
template <int BM, int KFIX = 0>   // rows of hop blocks per tile; 2 * BM threads = BM / 32 waves of 32 rows x 32 (wide tiles: 64) complex columns; KFIX: the hop, where the instantiation knows it (0: any)
__global__ __launch_bounds__(2 * BM, 4) void blockdft_gemm_tree(GemmTreeArgs a) {
    if constexpr (KFIX != 0) __builtin_assume(a.K == KFIX);   // 4 waves per SIMD = two 512-thread (four 256-thread) workgroups per CU: at most 128 registers
    constexpr bool WIDE = BM == 256;                   // (the 128-row form, a test shape, takes narrow tiles only)
    constexpr int B_FLOATS = (WIDE ? 2 : 1) * FR_KC * FT_BN;   // a wide tile's two slices of E
    constexpr int P_FLOATS = (BM + 15) * FT_LDP * 2;   // 15 spare rows: the register tree levels read their halo without a range check
    __shared__ __attribute__((aligned(16))) float smem[B_FLOATS > P_FLOATS ? B_FLOATS : P_FLOATS];  // the E slice(s), then the P tile
    __shared__ float2 tw_lds[2][FT_MAXL][CB_C];
    const unsigned long long t_entry = wall_clock64();
    const int tid = threadIdx.x, lane = tid & 63;
    const int4 entry = a.tile_list[blockIdx.x];   // .x: group | wide << 8 | segment << 16
    const TileStream ts = tile_stream(a, entry.x);
    FusedTile T = fused_tile_of<BM>(a, make_int4(entry.x & 7, entry.y, entry.z, entry.w), ts);   // (gv[8])
    const bool wide = ((entry.x >> 8) & 1) != 0;
    if (T.f0 >= T.nfr) return;
    const int stamp_slot = blockIdx.x;
    PVQ_STAMP(0);
    const long long s = ts.base + T.G.s_rel;
    const long long tile_lo = s + (long long)T.f0 * a.K, tile_hi = tile_lo + (long long)BM * a.K;  // sample range of the tile
    const bool inside = tile_lo >= 0 && tile_hi * 4ll <= (long long)ts.pcm_bytes;
    if (WIDE && wide && inside) {
        const float* tw_src = reinterpret_cast<const float*>(a.comb_tw + T.G.tw_off + T.ntl * CB_C) + lane;
        float* tw_dst = reinterpret_cast<float*>(&tw_lds[0][0][0]);
        const float4* e_tile = a.E16 + (size_t)T.nt * (a.K / 2) * 16;
        f32x4a accR[2][4], accI[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int np = 0; np < 4; ++np)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    accR[mt][np][r] = 0.0f;
                    accI[mt][np][r] = 0.0f;
                }
        if (a.clk != nullptr && (blockIdx.x & 63) == 0 && tid == 0) {
            a.clk[(blockIdx.x >> 6) * 4 + 0] = __builtin_amdgcn_s_memtime();
            a.clk[(blockIdx.x >> 6) * 4 + 1] = __builtin_amdgcn_s_memrealtime();
        }
        fused_f32_kloop64<BM>(a, ts.pcm_base, ts.pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, tw_src, tw_dst, T.G.levels_f, 2 * T.G.n_tiles * CB_C, stamp_slot);
        if (a.clk != nullptr && (blockIdx.x & 63) == 0 && tid == 0) {
            a.clk[(blockIdx.x >> 6) * 4 + 2] = __builtin_amdgcn_s_memtime();
            a.clk[(blockIdx.x >> 6) * 4 + 3] = __builtin_amdgcn_s_memrealtime();
        }
        PVQ_STAMP(1);
        // the two tiles' P' one after the other through the same buffer (the second waits in its accumulators)
        __syncthreads();   // the E slices are dead
        PVQ_STAMP(4);
        fused_dump_p<BM, 4, 0>(smem, accR, accI, tid);
        __syncthreads();
        PVQ_STAMP(5);
        fused_tree_store<BM>(smem, tw_lds[0], T, a, tid, stamp_slot);
        __syncthreads();
        fused_dump_p<BM, 4, 2>(smem, accR, accI, tid);
        __syncthreads();
        T.ntl += 1;
        T.nt += 1;
        fused_tree_store<BM>(smem, tw_lds[1], T, a, tid, stamp_slot);
        PVQ_END_STAMPS
        return;
    }
    // (the host pairs only tiles that lie inside the stream — same test, same numbers, launch(): the range-checked loop takes one tile)
    fused_f32_narrow_tile<BM>(a, ts.pcm_base, ts.pcm_bytes, smem, tw_lds, T, inside, tile_lo, tid, stamp_slot, WIDE && inside && (entry.x & TILE_MIXED) ? entry.x : 0, ts.n_frames);
    PVQ_END_STAMPS
}

// ------------------------------------------------------------------------------------------------
// General hops: a multiple of 64 samples that does NOT divide the windows (1 600 samples = 30 analyses per second at 48 kHz, the
// cadence of pitchvis_serial/src/main.rs:41; the trainer's 3 x chunk, pitchvis_train/src/train.rs:43).  With W = nq hop + rem,
//
//     X_f[c] = sum_{q < nq} phi_c^q Q[f + q][c]  +  phi_c^nq R[f + nq][c],     phi_c = e^{-2 pi i c hop / W},
//     Q[j][c] = sum_{m < hop} x[s + j hop + m] e^{-2 pi i c m / W}   (the whole hop block, as in the power-of-two case),
//     R[j][c] = sum_{m < rem} x[s + j hop + m] e^{-2 pi i c m / W}   (the block's first rem samples),
//
// so every hop block is still transformed once (twice: whole and head) for all the frames that share it — the cost is per SAMPLE,
// not per frame — and only the combine changes: nq <= 16 terms by Horner's rule instead of a power-of-two tree.  Both GEMMs are the
// mirrored half-depth form about their block's centre (Q' = Q / rho_Q, R' = R / rho_R); rho_Q goes into the kernel-product
// coefficients as before and tau_c = phi_c^nq rho_R / rho_Q multiplies R'.  Two launches of this kernel: the R tiles first (256 rows
// = 256 frames, rows taken nq blocks further on, results to Y — or straight to X for a window shorter than the hop, nq = 0), then
// the Q tiles (257 - nq frames per tile), which add tau Y on their way out.  Same K loop, same P tile, same X layout as
// blockdft_gemm_tree: the kernel-product and peak stages do not know the difference.
// ------------------------------------------------------------------------------------------------
template <int BM>
__device__ __forceinline__ void gen_horner(float* smem, const float2* phi, int nq, int tid) {
    float2 (*A)[FT_LDP] = reinterpret_cast<float2 (*)[FT_LDP]>(smem);  // [BM + 15][33]
    const int c = tid & (CB_C - 1), j0 = (tid >> 5) * 16;
    const float2 w = phi[c];
    float2 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = make_float2(0.0f, 0.0f);
    // out[i] = v[i] + w (v[i + 1] + w (... + w v[i + nq - 1])): rows taken from the far end; row r feeds output i as term q = r - i
    for (int r = 15 + nq - 1; r >= 0; --r) {
        const float2 x = A[j0 + r][c];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = r - i;
            if (q >= 0 && q < nq) acc[i] = tree_cmadd(x, w, acc[i]);   // (uniform; the first term: x + w * 0 = x exactly)
        }
    }
    __syncthreads();   // every thread has read its halo
#pragma unroll
    for (int i = 0; i < 16; ++i) A[j0 + i][c] = acc[i];
    __syncthreads();
}

template <int BM>
__global__ __launch_bounds__(2 * BM, 4) void blockdft_gemm_gen(GemmTreeArgs a) {
    constexpr int B_FLOATS = FR_KC * FT_BN;
    constexpr int P_FLOATS = (BM + 15) * FT_LDP * 2;
    __shared__ __attribute__((aligned(16))) float smem[B_FLOATS > P_FLOATS ? B_FLOATS : P_FLOATS];  // the E slice, then the P tile
    __shared__ float2 gtw[2][CB_C];   // phi, tau of the tile's columns
    const int tid = threadIdx.x;
    const int4 entry = a.tile_list[blockIdx.x];   // .x: group | segment << 16
    const TileStream ts = tile_stream(a, entry.x);
    const BlockGroup G = a.gv[entry.x & 7];
    const int ntl = entry.y, f0 = entry.z, nt = G.tile0 + ntl;
    if (f0 >= ts.n_frames) return;
    const int stamp_slot = blockIdx.x;
    const bool is_r = a.gen_kind == 1;
    const int depth = is_r ? G.rem : a.K;
    // rows of the tile: hop blocks f0 .. f0 + BM - 1 of the group's block grid (R tiles: nq blocks further on)
    const long long tile_lo = ts.base + G.s_rel + (long long)(f0 + (is_r ? G.nq : 0)) * a.K;
    const long long tile_hi = tile_lo + (long long)(BM - 1) * a.K + depth;
    const bool inside = tile_lo >= 0 && tile_hi * 4ll <= (long long)ts.pcm_bytes;
    const float4* e_tile = is_r ? a.E16R + G.e16r_off + (size_t)ntl * (G.rem / 2) * 16 : a.E16 + (size_t)nt * (a.K / 2) * 16;
    if (tid < 2 * CB_C) gtw[tid >> 5][tid & (CB_C - 1)] = a.gen_tw[G.gtw_off + (tid >> 5) * (G.n_tiles * CB_C) + ntl * CB_C + (tid & (CB_C - 1))];
    f32x4a accR[2][2], accI[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int np = 0; np < 2; ++np)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                accR[mt][np][r] = 0.0f;
                accI[mt][np][r] = 0.0f;
            }
    const bool half = ntl == G.n_tiles - 1 && G.n_cols - ntl * CB_C <= 16;
    float* no_tw = reinterpret_cast<float*>(&gtw[0][0]);   // (no tree twiddles to stage: tw_levels = 0)
    if (!inside)
        fused_f32_kloop16_edge<BM>(a, ts.pcm_base, ts.pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, no_tw, no_tw, 0, 0, stamp_slot, depth);
    else if (half)
        fused_f32_kloop16<BM, true>(a, ts.pcm_base, ts.pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, no_tw, no_tw, 0, 0, stamp_slot, depth);
    else
        fused_f32_kloop16<BM, false>(a, ts.pcm_base, ts.pcm_bytes, smem, tile_lo, e_tile, tid, accR, accI, no_tw, no_tw, 0, 0, stamp_slot, depth);
    __syncthreads();   // the E slice is dead: the P' tile takes its place
    fused_dump_p<BM, 2, 0>(smem, accR, accI, tid);
    __syncthreads();
    if (!is_r && G.nq > 1) gen_horner<BM>(smem, gtw[0], G.nq, tid);
    // store: lanes walk the frames of one column (512-byte runs); Q tiles add tau * R'[f + nq] (the R launch left it in Y)
    float2 (*A)[FT_LDP] = reinterpret_cast<float2 (*)[FT_LDP]>(smem);
    const int j = tid % BM;
    const int f = f0 + j;
    const int S = is_r ? BM : BM - (G.nq > 1 ? G.nq - 1 : 0);
    if (j < S && f < ts.n_frames) {
        const size_t at = ((size_t)((f >> 6) + ts.xt0) * a.xcp + nt * CB_C) * 64 + (f & 63);
        float2* dst = (is_r && G.nq > 0 ? a.Y : a.X) + at;
        const float2* ysrc = a.Y + at;
        const bool add_y = !is_r && G.rem > 0;
        const int ncv = G.n_cols - ntl * CB_C < CB_C ? G.n_cols - ntl * CB_C : CB_C;
#pragma unroll 4
        for (int cc = tid / BM; cc < ncv; cc += 2) {
            float2 val = A[j][cc];
            if (add_y) val = tree_cmadd(val, gtw[1][cc], ysrc[cc * 64]);
            if (is_r && G.nq > 0)
                dst[cc * 64] = val;   // read back by the Q launch: through the L2
            else
                __builtin_nontemporal_store((f32x2){val.x, val.y}, reinterpret_cast<f32x2*>(&dst[cc * 64]));
        }
    }
}

// Unfused form of the same GEMM (windows of more than 64 hop blocks: the tree runs as its own kernel over P' in memory):
// BM rows x 32 complex columns per workgroup, the K loop of the fused kernel, P' written tile-major as (re, im) pairs.
template <int BM>
__global__ __launch_bounds__(2 * BM, 2) void blockdft_gemm_rows(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[FR_KC * FT_BN];   // the E slice
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware tile order: workgroups are dealt round robin over the 8 XCDs (b and b + 8 share an L2), so an XCD owns
    // whole row panels: all column tiles that re-read one panel of the stream hit one L2
    const int b = blockIdx.x;
    const int xcd = b & 7, bi = b >> 3;
    const int nt = bi % a.n_col_tiles;
    const int mt = (bi / a.n_col_tiles) * 8 + xcd;
    if (mt * BM >= a.n_rows) return;
    const int j0 = mt * BM;
    const long long s = a.base + a.tile_s[nt];
    const long long tile_lo = s + (long long)j0 * a.K, tile_hi = tile_lo + (long long)BM * a.K;
    const long long row0 = tile_lo + (long long)(wave * 32 + (lane & 31)) * a.K;
    const int half = lane >> 5;
    const long long off_f0 = row0 + 16 * half;
    const long long off_b0 = row0 + a.K - 16 - 16 * half;
    const float* e_tile = a.E + (size_t)nt * FT_BN;
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        acc0[q] = 0.0f;
        acc1[q] = 0.0f;
    }
    if (tile_lo >= 0 && tile_hi * 4ll <= (long long)a.pcm_bytes)
        fused_f32_kloop<true, BM>(a, smem, off_f0, off_b0, e_tile, tid, acc0, acc1);
    else
        fused_f32_kloop<false, BM>(a, smem, off_f0, off_b0, e_tile, tid, acc0, acc1);
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5); a row of the tile is 256 contiguous bytes
    float2* Pt = reinterpret_cast<float2*>(a.P) + (size_t)nt * a.p_rows * CB_C;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = j0 + wave * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (row < a.n_rows) Pt[(size_t)row * CB_C + (lane & 31)] = make_float2(acc0[q], acc1[q]);
    }
}

// Split-bf16 form of the fused kernel ("bf16x3", the default; pvq_vqt_set_gemm_precision): same tile, same
// epilogue.  Each fp32 operand is written exactly as hi + mid + lo with three bf16 values (8+8+8 mantissa bits)
// and the product is accumulated in fp32 from the six partial products whose weight is >= 2^-16 (hh, hm, mh, hl,
// lh, mm); the dropped terms are below 2^-24 of the product, i.e. at fp32 rounding level, and every partial
// product of two bf16 numbers is exact in fp32.  v_mfma_f32_32x32x16_bf16 runs at 16x the rate of the fp32 MFMA,
// so six of them replace eight fp32 MFMAs at 6/16 of the matrix-pipe time.  E is split once on the host (planes
// stored [plane][n][k], k contiguous = the B-operand fragment order); the PCM tile is split while it is staged
// (16 consecutive samples per thread: 16-byte loads, 16-byte LDS writes).  LDS: 3 planes x (128 + 64) rows x 32
// bf16 = 36 KB of staging, swizzled instead of padded (4 workgroups per CU), aliased by the P tile.  Measured
// accuracy equals the fp32 MFMA form (6e-7 of the frame peak); the K loop runs at ~35 % of the bf16 matrix peak,
// bounded by the LDS staging and barrier structure of a 128 x 64 tile, not by the matrix pipe.
template <int BM> struct FbGeom {
    static constexpr int PLANE = (BM + FT_BN) * FB_BK;            // bf16 elements of one plane: BM PCM rows, then 64 E^T rows
    static constexpr int STAGE_BYTES = 3 * PLANE * 2;             // 36 864 B at BM = 128
    static constexpr int P_BYTES = (BM + 15) * FT_LDP * 8;        // the P tile that aliases the staging area (+ 15 spare rows: the tree's halo reads need no range check)
    static constexpr int LDS_BYTES = STAGE_BYTES > P_BYTES ? STAGE_BYTES : P_BYTES;
};
// element offset of the 8-sample chunk `ch` (0..3) of row `row` inside a plane.  Rows are 64 bytes, unpadded; the
// chunk index is XORed with (row / 4) % 4, which makes the b128 fragment reads (16 consecutive rows, one chunk),
// the PCM staging writes (8 rows x 2 chunks) and the E^T staging writes (4 rows x 4 chunks) bank-conflict free.
__device__ __forceinline__ int fb_off(int row, int ch) { return row * FB_BK + ((ch ^ ((row >> 2) & 3)) << 3); }

// K loop of the split-bf16 fused kernel.  VEC: the tile's samples all lie inside the stream, so each
// thread's 16 consecutive samples come as four 16-byte loads; otherwise (tiles that touch the stream start
// or end) as 16 dword loads, each range-checked by the buffer hardware.
template <bool VEC, int BM>
__device__ __forceinline__ void fused_bf16x3_kloop(const GemmTreeArgs& a, const float* pcm_base, unsigned pcm_bytes, unsigned char* smem_raw, long long a_idx0, const __bf16* e_ptr,
                                                   int tid, f32x16& acc0, f32x16& acc1) {
    constexpr int FB_PLANE = FbGeom<BM>::PLANE;
    __bf16* lds = reinterpret_cast<__bf16*>(smem_raw);
    const int lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const unsigned long long pcm_addr = reinterpret_cast<unsigned long long>(pcm_base);
    const i32x4 rsrc4 = {(int)(unsigned)pcm_addr, (int)(unsigned)(pcm_addr >> 32), (int)pcm_bytes, 0x00020000};
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pcm_base), 0, pcm_bytes, 0x00020000);
    // A staging: thread -> (row = tid / 2, 16 consecutive k); B staging: thread -> (n = tid / 4, 8 consecutive k) x 3 planes
    const int a_row = tid >> 1, b_n = tid >> 2;
    const size_t plane = (size_t)a.ld * a.K;
    float ra[16];
    bf16x8 rb[3];
    auto load = [&](int k0) {
        if (VEC) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = pvq_raw_buffer_load_f32x4(rsrc4, (int)((unsigned)(a_idx0 * 4ll) + (unsigned)k0 * 4u + 16u * q), 0, 0);
                ra[4 * q + 0] = v[0];
                ra[4 * q + 1] = v[1];
                ra[4 * q + 2] = v[2];
                ra[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {   // samples before the stream: an explicit out-of-range offset (see fused_f32_stage_load)
                const long long j = a_idx0 + k0 + q;
                ra[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, j >= 0 ? (unsigned)(j * 4ll) : 0xFFFFFFFCu, 0, 0));
            }
        }
        if (BM == 128 || tid < 256) {
#pragma unroll
            for (int p = 0; p < 3; ++p) rb[p] = *reinterpret_cast<const bf16x8*>(e_ptr + p * plane + k0);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            bf16x8 vh, vm, vl;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float x = ra[8 * h + q];
                const __bf16 hi = (__bf16)x;
                const float r1 = x - (float)hi;
                const __bf16 mid = (__bf16)r1;
                vh[q] = hi;
                vm[q] = mid;
                vl[q] = (__bf16)(r1 - (float)mid);
            }
            const int o = fb_off(a_row, (tid & 1) * 2 + h);
            *reinterpret_cast<bf16x8*>(lds + o) = vh;
            *reinterpret_cast<bf16x8*>(lds + FB_PLANE + o) = vm;
            *reinterpret_cast<bf16x8*>(lds + 2 * FB_PLANE + o) = vl;
        }
        if (BM == 128 || tid < 256) {   // 64 E^T rows x 4 chunks: 256 threads
            const int ob = fb_off(BM + b_n, tid & 3);
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(lds + p * FB_PLANE + ob) = rb[p];
        }
    };
    const int n_iter = a.K / FB_BK;
    const int ar = wm * 64 + (lane & 31), kh = lane >> 5, bc = BM + wn * 32 + (lane & 31);
    load(0);
    for (int it = 0; it < n_iter; ++it) {
        store();
        __syncthreads();
        if (it + 1 < n_iter) load((it + 1) * FB_BK);
#pragma unroll
        for (int kk = 0; kk < FB_BK / 16; ++kk) {
            bf16x8 a0[3], a1[3], bv[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                a0[p] = *reinterpret_cast<const bf16x8*>(lds + p * FB_PLANE + fb_off(ar, kk * 2 + kh));
                a1[p] = *reinterpret_cast<const bf16x8*>(lds + p * FB_PLANE + fb_off(ar + 32, kk * 2 + kh));
                bv[p] = *reinterpret_cast<const bf16x8*>(lds + p * FB_PLANE + fb_off(bc, kk * 2 + kh));
            }
            // smallest terms first
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], bv[1], acc0, 0, 0, 0);  // mid*mid
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[1], bv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], bv[2], acc0, 0, 0, 0);  // hi*lo
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], bv[2], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[2], bv[0], acc0, 0, 0, 0);  // lo*hi
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[2], bv[0], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], bv[1], acc0, 0, 0, 0);  // hi*mid
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], bv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], bv[0], acc0, 0, 0, 0);  // mid*hi
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[1], bv[0], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], bv[0], acc0, 0, 0, 0);  // hi*hi
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], bv[0], acc1, 0, 0, 0);
        }
        __syncthreads();
    }
}

template <int BM>   // rows of hop blocks per tile; 2 * BM threads (wave tile 64 x 32)
__global__ __launch_bounds__(2 * BM, BM == 128 ? 4 : 2) void blockdft_gemm_tree_bf16x3(GemmTreeArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[FbGeom<BM>::LDS_BYTES];
    __shared__ float2 tw_lds[FT_MAXL][CB_C];
    float* smem = reinterpret_cast<float*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TileStream ts;
    const FusedTile T = fused_tile<BM>(a, ts);
    const int f0 = T.f0, nt = T.nt;
    if (f0 >= T.nfr) return;
    if (tid < 256) fused_stage_twiddles(tw_lds, T, a, tid);
    const int wm = wave >> 1, wn = wave & 1;
    const long long s = ts.base + T.G.s_rel;
    const long long tile_lo = s + (long long)f0 * a.K, tile_hi = tile_lo + (long long)BM * a.K;  // sample range of the tile
    const long long a_off0 = tile_lo + (long long)(tid >> 1) * a.K + (tid & 1) * 16;   // sample index of the thread's 16-sample run
    const __bf16* e_ptr = a.Et + (size_t)(nt * FT_BN + ((tid & 255) >> 2)) * a.K + (tid & 3) * 8;
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        acc0[q] = 0.0f;
        acc1[q] = 0.0f;
    }
    if (tile_lo >= 0 && tile_hi * 4ll <= (long long)ts.pcm_bytes)
        fused_bf16x3_kloop<true, BM>(a, ts.pcm_base, ts.pcm_bytes, smem_raw, a_off0, e_ptr, tid, acc0, acc1);
    else
        fused_bf16x3_kloop<false, BM>(a, ts.pcm_base, ts.pcm_bytes, smem_raw, a_off0, e_ptr, tid, acc0, acc1);
    const int bc = wn * 32 + (lane & 31);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = wm * 64 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        smem[row * (2 * FT_LDP) + bc] = acc0[q];
        smem[(row + 32) * (2 * FT_LDP) + bc] = acc1[q];
    }
    if (tid < 15 * FT_LDP) reinterpret_cast<float2*>(smem)[BM * FT_LDP + tid] = make_float2(0.0f, 0.0f);   // the spare rows
    __syncthreads();
    fused_tree_store<BM>(smem, tw_lds, T, a, tid, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Last tree levels for windows of more than 64 hop blocks: the fused kernel leaves Y_f = sum_{b<64} phi^b P'[f+b];
// X'_f = sum_q phi^{64 q} Y_{f+64q} (2 or 4 terms) with the same level-by-level multiply-adds as the rest of the tree.
// Y_{f+64q} is the same lane of the same column q frame tiles further on: 512-byte runs in, 512-byte runs out.
// ------------------------------------------------------------------------------------------------
struct FinishArgs {
    const float2* Y;
    float2* X;
    int xcp;
    int n_frames;
    int col0;          // first X column of the group
    int n_cols;        // columns of the group (padded to its tiles): the twiddle table's row stride
    int n_real;        // columns of the group that exist (the padding is neither written by the fused kernel nor combined here)
    int levels_f, levels;
    const float2* tw;  // the group's combine twiddles: [levels][n_cols]
    const XTile* xmap; // many-streams launches: per X tile, the Y tile of the same frames and the number of frames that exist
};
__global__ __launch_bounds__(256) void blockdft_tree_finish(FinishArgs a) {
    const int fr = threadIdx.x & 63, cc = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int tile = blockIdx.x;
    int ytile = tile, n_live = a.n_frames - tile * 64;
    if (a.xmap) {
        ytile = a.xmap[tile].y_tile;
        n_live = a.xmap[tile].live_step & 255;
    }
    if (cc >= a.n_real || fr >= n_live) return;
    const int col = a.col0 + cc;
    const int nq = 1 << (a.levels - a.levels_f);   // 2 or 4
    float2 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < nq) v[q] = a.Y[((size_t)(ytile + q) * a.xcp + col) * 64 + fr];
    const float2 w0 = a.tw[(size_t)a.levels_f * a.n_cols + cc];
    if (nq == 2) {
        v[0] = tree_cmadd(v[0], w0, v[1]);
    } else {
        const float2 w1 = a.tw[(size_t)(a.levels_f + 1) * a.n_cols + cc];
        v[0] = tree_cmadd(tree_cmadd(v[0], w0, v[1]), w1, tree_cmadd(v[2], w0, v[3]));
    }
    a.X[((size_t)tile * a.xcp + col) * 64 + fr] = v[0];
}

// ------------------------------------------------------------------------------------------------
// combine: X_f[c] = sum_b phi_c^b P[f+b][c] by a doubling tree in LDS
// ------------------------------------------------------------------------------------------------
struct CombineArgs {
    const float* P;
    int p_rows;        // row capacity of the tile-major P
    float2* X;         // frame-tile blocked: X[((frame / 64) * xcp + col) * 64 + frame % 64]
    int xcp;
    int n_frames;      // frames in this chunk
    int n_rows;        // rows of P present
    const int* tile_group;
    const BlockGroup* groups;
    const float2* comb_tw;
};

// CT frames x CW complex columns per workgroup; windows of up to MAXNB hop blocks.
template <int CT, int CW, int MAXNB>
__global__ __launch_bounds__(256) void blockdft_combine(CombineArgs a) {
    constexpr int MAXR = CT + MAXNB - 1;
    __shared__ float2 A[MAXR][CW + 1];   // +1: the transposed store below reads a column per wave
    const int tid = threadIdx.x;
    const int col0 = blockIdx.x * CW;          // first complex column of this tile (global X column)
    const int f0 = blockIdx.y * CT;
    const BlockGroup G = a.groups[a.tile_group[col0 / CB_C]];
    const int R = CT + G.nb - 1;
    const int c = tid & (CW - 1);
    // stage rows f0 .. f0+R-1 of this column tile
    for (int idx = tid; idx < R * CW; idx += 256) {
        const int j = idx / CW;
        const int row = f0 + j;
        float2 v = make_float2(0.0f, 0.0f);
        if (row < a.n_rows)
            v = *reinterpret_cast<const float2*>(a.P + ((size_t)(col0 / CB_C) * a.p_rows + row) * 64 + 2 * ((col0 % CB_C) + c));
        A[j][c] = v;
    }
    __syncthreads();
    constexpr int PER = (MAXR * CW + 255) / 256;
    int valid = R;
    for (int l = 0; l < G.levels; ++l) {
        const int s = 1 << l;
        valid -= s;  // rows with a complete span after this level
        const float2 w = a.comb_tw[G.tw_off + l * (G.n_tiles * CB_C) + (col0 - G.tile0 * CB_C) + c];
        float2 v[PER];
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int idx = tid + t * 256;
            const int j = idx / CW;
            if (j < valid) {
                const float2 lo = A[j][c], hi = A[j + s][c];
                v[t] = make_float2(lo.x + (w.x * hi.x - w.y * hi.y), lo.y + (w.x * hi.y + w.y * hi.x));
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int idx = tid + t * 256;
            const int j = idx / CW;
            if (j < valid) A[j][c] = v[t];
        }
        __syncthreads();
    }
    {
        const int j = tid & (CT - 1);
        const int f = f0 + j;
        if (f < a.n_frames)
            for (int cc = tid / CT; cc < CW; cc += 256 / CT) a.X[((size_t)(f >> 6) * a.xcp + col0 + cc) * 64 + (f & 63)] = A[j][cc];
    }
}

// The launch's tile list of one kind, from the cache or built and uploaded with its segment table and X-tile map (one allocation:
// list | segments | map).  The list is cached per (tile rows, kernel family, the runs' stream geometry): which tiles lie wholly
// inside their stream — 16-byte loads, wide entries — is decided by the planner with the kernel's own test (tile_inside_stream), so a
// list built for one geometry must never be used for another (round 3: a list keyed on the frame count alone let a launch read past
// a shorter stream's end).  A launch of one run hands its stream pointer and output rows over in the kernel arguments: they are not
// part of its key, so the middle sub-batches of a long stream share one list, and so do different buffers of one geometry.
static pvq_status get_tile_list(BlockDftTables* t, const BlockLaunch& L, int kind, int bm, int wide_mode, const TileListOptions& opt,
                                hipStream_t stream, BlockDftTables::TileList** out) {
    const LaunchShape& sh = *L.shape;
    const int list_mode = wide_mode | (opt.mixed.empty() ? 0 : 4);   // (a list with mixed entries is a list of its own)
    std::vector<SegKey> key = sh.segs;
    if (!L.multi) key[0].pcm_off = key[0].out_row0 = key[0].fbeg = 0;
    for (auto& c : t->tile_lists)
        if (c.bm == bm && c.wide == list_mode && c.multi == L.multi && c.kind == kind && c.key == key && c.slot_data == sh.slot_data) {
            *out = &c;
            return PVQ_OK;
        }
    BlockDftTables::TileList* tl = &t->tile_lists[t->tile_list_next];
    t->tile_list_next = (t->tile_list_next + 1) & 7;
    const HostTileList h = build_tile_list(t->groups, sh.segs, t->hop, bm, wide_mode, kind, opt);
    std::vector<SegDev> hsegs;
    std::vector<XTile> hmap;
    build_segment_map(L.streams, *L.runs, sh, hsegs, hmap);
    const size_t b_list = h.list.size() * sizeof(int4), b_segs = (hsegs.size() * sizeof(SegDev) + 15) / 16 * 16, b_map = hmap.size() * sizeof(XTile);
    pvq_status s = grow(&tl->d, &tl->cap, b_list + b_segs + b_map);
    if (s != PVQ_OK) return s;
    PVQ_HIP(hipStreamSynchronize(stream));   // an earlier launch may still read this slot
    char* dbase = reinterpret_cast<char*>(tl->d);
    PVQ_HIP(hipMemcpy(dbase, h.list.data(), b_list, hipMemcpyHostToDevice));
    PVQ_HIP(hipMemcpy(dbase + b_list, hsegs.data(), hsegs.size() * sizeof(SegDev), hipMemcpyHostToDevice));
    PVQ_HIP(hipMemcpy(dbase + b_list + b_segs, hmap.data(), b_map, hipMemcpyHostToDevice));
    tl->d_segs = reinterpret_cast<const SegDev*>(dbase + b_list);
    tl->d_xmap = reinterpret_cast<const XTile*>(dbase + b_list + b_segs);
    tl->key = key;
    tl->slot_data = sh.slot_data;
    tl->bm = bm;
    tl->wide = list_mode;
    tl->multi = L.multi;
    tl->kind = kind;
    tl->blocks = (int)h.list.size();
    tl->eff_tiles = h.eff_tiles;
    tl->eff_flop = h.eff_flop;
    *out = tl;
    return PVQ_OK;
}

// GEMM + tree fused: picks the tile shape, fetches the launch's tile list(s) and runs the kernel family of the hop and arithmetic
pvq_status Vqt::launch_blockdft_gemm_fused(BlockLaunch& L, hipStream_t stream) {
    BlockDftTables* t = dev_->block;
    const std::vector<SegKey>& segs = L.shape->segs;
    const size_t hop = t->hop;
    const bool use_bf = L.use_bf;
    if (segs.size() > 0xFFFFu) {
        set_last_error("too many streams in one launch");
        return PVQ_ERR_INTERNAL;
    }
    // 256-row tiles: 257 - Nb complete frames per tile (1.08x row recomputation instead of 1.2x with 128 rows) — for a launch that
    // fills the chip's 512 workgroup slots a few times over.  A smaller one (fewer than FUSED_SMALL 256-row tiles: up to ~12 000
    // frames at 48 kHz / 252 bins) takes 128-row tiles: twice the workgroups, each half as long — what such a launch lacks is
    // parallelism, not efficiency (hop 1 600: 4 096 frames 294 -> 216 us, 8 192: 324 -> 292; hop 256: 2 048 frames 61 -> 54;
    // profiles/r04_small_tiles.txt).  Same bits either way (a frame's values do not depend on its tile: tests/test_tile_shapes).
    constexpr double FUSED_SMALL = 1400.0;
    static const int bm_env = dev_knob("PVQ_FUSED_BM", 0);          // 128: 128-row tiles (the tile-shape bit-identity test)
    int fused_bm = 256;
    if (!use_bf && (bm_env == 128 || (bm_env == 0 && fused_tile_count(t->groups, segs, 256, use_bf) < FUSED_SMALL))) fused_bm = 128;
    // the tile order's knobs (blockdft_plan.hpp: build_tile_list)
    static const TileListOptions opt = [] {
        TileListOptions o;
        o.fs = dev_knob("PVQ_TILE_FS", 2048);
        o.balance = dev_knob("PVQ_BALANCE", 1);
        o.tail = dev_knob("PVQ_TAIL", 128);
        return o;
    }();
    static const int wide_env = dev_knob("PVQ_WIDE", 1);         // 0: narrow tiles only; 2: wide tiles to the very end of every queue
    const int wide_mode = !use_bf && fused_bm == 256 && !t->general ? wide_env : 0;   // (the split-bf16 kernel, the 128-row form and the general-hop kernel take 32-column tiles only)
    // mixed tiles (two window groups' partial last column tiles in one tile: blockdft_plan.hpp, MixedPair): the fp32 256-row kernel only.
    // Developer library: PVQ_MIXED_TILES=0 takes the former list (A/B, bit identity), and so does the former epilogue (PVQ_TREE_TAIL=0).
    static const bool mixed_env = dev_knob("PVQ_MIXED_TILES", 1) != 0 && dev_knob("PVQ_TREE_TAIL", 1) != 0;
    TileListOptions lopt = opt;
    if (mixed_env && !use_bf && fused_bm == 256 && !t->general) lopt.mixed = t->mixed;
    BlockDftTables::TileList* tl = nullptr;
    BlockDftTables::TileList* tl_r = nullptr;   // general hops: the remainder tiles
    pvq_status ls;
    if (t->general) {
        if ((ls = get_tile_list(t, L, 1, fused_bm, wide_mode, lopt, stream, &tl_r)) != PVQ_OK) return ls;
        if ((ls = get_tile_list(t, L, 2, fused_bm, wide_mode, lopt, stream, &tl)) != PVQ_OK) return ls;
        // (the second lookup may have evicted the first — the slots are handed out round robin — look it up again)
        if ((ls = get_tile_list(t, L, 1, fused_bm, wide_mode, lopt, stream, &tl_r)) != PVQ_OK) return ls;
    } else if ((ls = get_tile_list(t, L, 0, fused_bm, wide_mode, lopt, stream, &tl)) != PVQ_OK)
        return ls;
    L.d_xmap = L.multi ? tl->d_xmap : nullptr;
    const int n_wg = tl->blocks;   // list entries = workgroups of the non-persistent forms = rows of the stamp dump
    GemmTreeArgs fa;
    fa.pcm_base = L.pcm_base;
    fa.pcm_bytes = segs[0].pcm_bytes;
    fa.E = t->d_E;
    fa.ld = L.ntot;
    fa.X = t->d_X;
    fa.Y = t->d_Y;
    fa.xcp = L.xcp;
    fa.n_frames = (int)segs[0].nf;
    fa.K = (int)hop;
    fa.base = segs[0].base;
    fa.n_groups = t->n_groups;
    fa.tile_list = tl->d;
    fa.segs = L.multi ? tl->d_segs : nullptr;
    fa.groups = t->d_groups;
    for (int g = 0; g < 8; ++g) fa.gv[g] = t->groups[std::min(g, t->n_groups - 1)];
    fa.comb_tw = t->d_comb_tw;
    fa.Et = t->d_Et;
    fa.E16 = t->d_E16;
    fa.E16R = t->d_E16R;
    fa.gen_tw = t->d_gen_tw;
    fa.gen_kind = 0;
#ifdef PVQ_DEV_KNOBS
    static const int tree_tail_env = dev_knob("PVQ_TREE_TAIL", 1);   // 0: the former epilogue (A/B, bit identity)
    fa.tree_tail = tree_tail_env;
#endif
    static const char* stamps_env = dev_knob_str("PVQ_STAMPS");   // dump per-tile phase stamps of the first launch
    static bool stamps_done = false;
    static int stamps_skip = dev_knob("PVQ_STAMPS_SKIP", 0);         // ... of launch n + 1 (a warm one)
    const bool do_stamps = stamps_env && !stamps_done && stamps_skip-- <= 0;
    fa.stamps = nullptr;
    if (do_stamps) PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&fa.stamps), (size_t)n_wg * 12 * 8 + 8));   // rows of 8, then rows of 4 (PVQ_END_STAMPS)
    if (do_stamps) PVQ_HIP(hipMemset(fa.stamps, 0, (size_t)n_wg * 12 * 8 + 8));
    // flop the GEMM's matrix instructions issue in this launch: tiles x rows x 64 real columns x depth x 2
    // (depth hop / 2 in the mirrored fp32 form, hop in the split-bf16 form, where it counts fp32-equivalent products; fp32: what the
    // list's entries issue: a wide entry two whole tiles, a lone half tile half a tile)
    const double eff_tiles = use_bf ? fused_tile_count(t->groups, segs, fused_bm, use_bf) : tl->eff_tiles;
    last_gemm_flop_ = eff_tiles * fused_bm * (2 * CB_C) * (use_bf ? (double)hop : (double)hop / 2) * 2.0;
    fa.clk = nullptr;
    if (profiling_ && !use_bf) {
        const size_t need = ((size_t)n_wg / 64 + 1) * 4 * sizeof(unsigned long long);
        bool grown = false;
        if ((ls = grow(&t->d_clk, &t->clk_cap, need, &grown)) != PVQ_OK) return ls;
        if (grown) PVQ_HIP(hipMemset(t->d_clk, 0, need));   // once: every sampled workgroup rewrites its slot at every launch (a fill per launch cost the stream 3 us)
        t->clk_n = n_wg / 64 + 1;
        fa.clk = t->d_clk;
    }
    slot_begin(SLOT_BLOCKDFT_GEMM, stream);
    if (t->general) {
        // the remainder tiles first (their results wait in Y), then the whole-block tiles; flop: both launches' K loops
        double flop = 0.0;
        for (int kind = 1; kind <= 2; ++kind) {
            const BlockDftTables::TileList* list = kind == 1 ? tl_r : tl;
            if (list->blocks == 0 || list->eff_tiles == 0.0) continue;
            GemmTreeArgs ga = fa;
            ga.tile_list = list->d;
            ga.segs = L.multi ? list->d_segs : nullptr;
            ga.gen_kind = kind;
            ga.stamps = nullptr;
            ga.clk = nullptr;
            if (fused_bm == 256)
                hipLaunchKernelGGL(blockdft_gemm_gen<256>, dim3(list->blocks), dim3(512), 0, stream, ga);
            else
                hipLaunchKernelGGL(blockdft_gemm_gen<128>, dim3(list->blocks), dim3(256), 0, stream, ga);
            flop += list->eff_flop;
        }
        last_gemm_flop_ = flop;
    } else if (use_bf)
        hipLaunchKernelGGL(blockdft_gemm_tree_bf16x3<256>, dim3(n_wg), dim3(512), 0, stream, fa);
    else if (fused_bm == 256 && fa.K == 256 && dev_knob("PVQ_KFIX", 1))   // the instantiations that know the hop: 2 % fewer cycles (its strides and trip counts fold)
        hipLaunchKernelGGL((blockdft_gemm_tree<256, 256>), dim3(n_wg), dim3(512), 0, stream, fa);
    else if (fused_bm == 256)
        hipLaunchKernelGGL(blockdft_gemm_tree<256>, dim3(n_wg), dim3(512), 0, stream, fa);
    else
        hipLaunchKernelGGL(blockdft_gemm_tree<128>, dim3(n_wg), dim3(256), 0, stream, fa);
    slot_end(SLOT_BLOCKDFT_GEMM, stream);
    if (do_stamps) {
        stamps_done = true;
        return dump_stamps(stamps_env, fa.stamps, (size_t)n_wg * 12, stream);
    }
    return PVQ_OK;
}

// the last one or two tree levels of the windows of more than 64 hop blocks: Y (64-block partial sums) -> X
void Vqt::launch_blockdft_tree_finish(const BlockLaunch& L, hipStream_t stream) {
    BlockDftTables* t = dev_->block;
    slot_begin(SLOT_BLOCKDFT_COMBINE, stream);
    for (int g = 0; g < t->n_groups; ++g) {
        const BlockGroup& G = t->groups[g];
        if (G.nb <= G.nb_f) continue;
        FinishArgs fin;
        fin.Y = t->d_Y;
        fin.X = t->d_X;
        fin.xcp = L.xcp;
        fin.n_frames = (int)L.nf;
        fin.col0 = G.tile0 * CB_C;
        fin.n_cols = G.n_tiles * CB_C;
        fin.n_real = G.n_cols;
        fin.levels_f = G.levels_f;
        fin.levels = G.levels;
        fin.tw = t->d_comb_tw + G.tw_off;
        fin.xmap = L.d_xmap;
        hipLaunchKernelGGL(blockdft_tree_finish, dim3((unsigned)((L.nf + 63) / 64), (unsigned)((fin.n_real + 3) / 4)), dim3(256), 0,
                           stream, fin);
    }
    slot_end(SLOT_BLOCKDFT_COMBINE, stream);
}

// GEMM and tree as two kernels with P in memory (more than 8 window groups, or PVQ_NO_FUSE in the developer library): one stream
void Vqt::launch_blockdft_gemm_unfused(const BlockLaunch& L, hipStream_t stream) {
    BlockDftTables* t = dev_->block;
    const size_t hop = t->hop, nf = L.nf;
    const int n_rows = (int)(nf + t->nb_max - 1);
    GemmArgs ga;
    ga.pcm_base = L.pcm_base;
    ga.pcm_bytes = L.shape->segs[0].pcm_bytes;
    ga.E = t->d_E;
    ga.ld = L.ntot;
    ga.P = t->d_P;
    ga.n_rows = n_rows;
    ga.K = (int)hop;
    ga.tile_s = t->d_tile_s;
    ga.base = L.shape->segs[0].base;
    ga.n_col_tiles = t->n_tiles;
    ga.p_rows = (int)L.rows_cap;
    const int m_tiles8 = (((n_rows + 255) / 256) + 7) / 8 * 8;
    last_gemm_flop_ = (double)ga.n_col_tiles * ((n_rows + 255) / 256) * 256.0 * FT_BN * ((double)hop / 2) * 2.0;
    slot_begin(SLOT_BLOCKDFT_GEMM, stream);
    hipLaunchKernelGGL(blockdft_gemm_rows<256>, dim3(ga.n_col_tiles * m_tiles8), dim3(512), 0, stream, ga);
    slot_end(SLOT_BLOCKDFT_GEMM, stream);
    CombineArgs ca;
    ca.P = t->d_P;
    ca.p_rows = (int)L.rows_cap;
    ca.X = t->d_X;
    ca.xcp = L.xcp;
    ca.n_frames = (int)nf;
    ca.n_rows = n_rows;
    ca.tile_group = t->d_tile_group;
    ca.groups = t->d_groups;
    ca.comb_tw = t->d_comb_tw;
    slot_begin(SLOT_BLOCKDFT_COMBINE, stream);
    if (t->nb_max <= 64)
        hipLaunchKernelGGL((blockdft_combine<128, 16, 64>), dim3(t->n_tiles * 2, (unsigned)((nf + 127) / 128)), dim3(256), 0,
                           stream, ca);
    else
        hipLaunchKernelGGL((blockdft_combine<CB_T, 16, 256>), dim3(t->n_tiles * 2, (unsigned)((nf + CB_T - 1) / CB_T)), dim3(256),
                           0, stream, ca);
    slot_end(SLOT_BLOCKDFT_COMBINE, stream);
}

}  // namespace pvq
