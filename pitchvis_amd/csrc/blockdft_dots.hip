// blockdft_dots.hip — the kernel product + power_to_db stage of the block-DFT path (vqt_blockdft.hip has the map), with its launcher.
//
// Kernels:  blockdft_banddots4c_db / blockdft_banddots_db[_bf16x3] (kernel product as a banded MFMA GEMM + power_to_db);
//           developer library only: blockdft_banddots4c_blocks_db, blockdft_banddots_db<2, 8>
#include <type_traits>

#include "blockdft_device.hpp"

namespace pvq {

// ------------------------------------------------------------------------------------------------
// kernel product + dB:  x_vqt[k] = sum_c K[k][c] X[c] (+ conjugate part), then power_to_db (vqt.rs:889-954)
//
// The rows of a window group's spectral kernel are band-limited wavelets: consecutive bins read
// overlapping, nearly contiguous column ranges (27 % of a 16-bin x 70-column block is non-zero).  A block
// of 16 bins is therefore a small dense real GEMM per frame tile,
//     [32 frames x 2 kb] . [2 kb x 32]   (columns: Xr, Xi of kb spectrum columns; outputs: 16 x re, 16 x im),
// one v_mfma_f32_32x32x2_f32 per spectrum column, with both operands read straight from memory in lane
// order (X is column-major, so the 32 frames of a column are 256 contiguous bytes; the coefficient table
// is stored as B operands and stays in L2).  The conjugate part (negative_filter_bank) lands in the same
// B matrix with the signs of the Xi row flipped.  A workgroup owns FT frames and all bins: its four waves
// walk disjoint lists of blocks, drop the dB values into LDS, and the frame-wide max / floor / shift of
// power_to_db is applied from there.
// ------------------------------------------------------------------------------------------------
struct BandArgs {
    const float* X;            // complex spectrum columns, as floats: [frame / 64][column][frame % 64][re, im]
    int xcp;                   // columns per 64-frame tile of X (incl. pad)
    int n_frames;
    int n_bins;
    int ldb;                   // LDS row stride of the dB tile
    const BandBlock* blocks;
    const float* B;
    const __bf16* B3;          // split-bf16 coefficient planes
    const int* list;           // [waves][per_wave]: count, then the blocks of that wave
    int per_wave;
    const BandStage* stages;   // 8-bin stream form: [8][stage_stride], a wave's stages end to end (blockdft_plan.hpp)
    int stage_stride;
    int stage_count[8];        // stages wave w multiplies: a multiple of BD8_NS
    float* out_db;             // [n_frames][n_bins]
    float2* out_cplx;          // optional
    unsigned* status;          // the handle's sticky flag word: bit 0 <- a live frame holds a non-finite power value
    const XTile* xmap;         // many-streams launches: per X tile, its output rows and how many of its frames exist (nullptr: tile t holds rows 64 t ...)
    unsigned long long* stamps;   // developer knob PVQ_STAMPS_DOTS: [workgroup][8] 100 MHz clock: 0 start, 1 wave 0 done with its blocks, 2 all waves done, 3 end
};

#define PVQ_REF_POWER (0.3f * 0.3f)
#define PVQ_A_MIN (1e-6f * 1e-6f)
#define PVQ_TOP_DB 60.0f

// gfx950 lane-row swaps.  Inline asm: this compiler's two-result builtins (__builtin_amdgcn_permlane16_swap /
// permlane32_swap) were seen to hand the same register to both results once inlined into a larger kernel.
// x' = [x.rows 0, y.rows 0, x.rows 2, y.rows 2],  y' = [x.rows 1, y.rows 1, x.rows 3, y.rows 3]   (rows of 16 lanes)
__device__ __forceinline__ void permlane16_swap(float& x, float& y) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
}
// x' = [x.lo, y.lo],  y' = [x.hi, y.hi]   (halves of 32 lanes)
__device__ __forceinline__ void permlane32_swap(float& x, float& y) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
}

// wave-wide max / min by DPP (within rows of 16 lanes) and the gfx950 row / half swaps (across rows)
#define PVQ_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (ctrl), 0xf, 0xf, true))
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, PVQ_DPP(v, 0xB1));    // quad_perm(1,0,3,2)
    v = fmaxf(v, PVQ_DPP(v, 0x4E));    // quad_perm(2,3,0,1)
    v = fmaxf(v, PVQ_DPP(v, 0x141));   // row_half_mirror
    v = fmaxf(v, PVQ_DPP(v, 0x140));   // row_mirror
    float x = v, y = v;
    permlane16_swap(x, y);
    v = fmaxf(x, y);
    x = v;
    y = v;
    permlane32_swap(x, y);
    return fmaxf(x, y);
}
__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// results of one block (C layout: column n = lane & 31: bin row = n & 15, re / im = n >> 4; frame =
// (q&3) + 8(q>>2) + 4(lane>>5)) -> |x_vqt|^2 into the LDS tile (+ the optional complex output).
// v_permlane16_swap brings the im column's value into the re column's lane.
// LDB: compile-time row stride of the tile (0: a.ldb) — with it every LDS address below is one base plus an immediate
// offset; the optional complex output recomputes its addresses per block (the row stride is laundered through an
// asm so that 32 loop-invariant 64-bit addresses are not kept live across the whole block loop).
template <int MT, int LDB>
__device__ __forceinline__ void band_writeout(const f32x16 (&acc)[MT], float* dbs, const BandArgs& a, long long row0, int n_live, int rstep, int bin0, int nrows,
                                              int lane) {
    const int ldb = LDB ? LDB : a.ldb;
    const int n = lane & 31, kx = lane >> 5;
    const int row = n & 15, part = n >> 4;
    const bool mine = part == 0 && row < nrows;
    const int bin = bin0 + row;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        float im[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float re = acc[mt][q], o = 0.0f;
            permlane16_swap(re, o);   // o: rows 0 / 2 now hold the im columns' values
            im[q] = o;
        }
        if (mine) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int fr = mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * kx;
                dbs[fr * ldb + bin] = acc[mt][q] * acc[mt][q] + im[q] * im[q];
            }
            if (a.out_cplx) {
                int row_stride = a.n_bins;
                asm volatile("" : "+s"(row_stride));
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int fr = mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * kx;
                    if (fr < n_live) a.out_cplx[(size_t)(row0 + (long long)fr * rstep) * row_stride + bin] = make_float2(acc[mt][q], im[q]);
                }
            }
        }
    }
}

// power_to_db per frame (vqt.rs:922-954): a wave per frame, lanes over bins.  Up to 512 bins: four (two) frames at a
// time with their dB values in registers, so the read -> log -> reduce -> rescale chains of the frames overlap
// (the phase is latency-bound at two waves per SIMD); more bins: one frame at a time through LDS.
template <int MT, int NW, int LDB = (MT == 2 ? BAND_LDB2 : 0)>
__device__ __forceinline__ void band_finish(float* dbs, const BandArgs& a, long long row0, int n_live, int rstep, int wave, int lane) {
    const int ldb = LDB ? LDB : a.ldb;
    const float ref_db = 10.0f * log10f(PVQ_REF_POWER);
    // 10 log10(p) = 10 log10(2) * log2(p) on the hardware log2 (1 ulp): within 2e-5 dB of the libm route
    auto to_db = [&](float p) { return 3.01029995663981f * __log2f(fmaxf(p, PVQ_A_MIN)) - ref_db; };
    // non-finite input (a NaN / Inf sample inside one of the frame's windows) reaches every bin of the frame as a NaN or Inf
    // power; fmaxf would silently turn it into the A_MIN floor, so it is flagged instead (Vqt::input_status)
    bool bad = false;
    auto flag = [&]() {
        if (a.status && __builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(a.status, 1u);
    };
    auto in_registers = [&](auto fu_c, auto nkb_c) {
        constexpr int FU = decltype(fu_c)::value, NKB = decltype(nkb_c)::value;
        for (int fr0 = wave; fr0 < MT * 32; fr0 += NW * FU) {
            float d[FU][NKB], mx[FU], mn[FU];
#pragma unroll
            for (int u = 0; u < FU; ++u) {
                mx[u] = -3.40282347e+38f;
                mn[u] = 3.40282347e+38f;
                const bool live = fr0 + NW * u < n_live;
#pragma unroll
                for (int kk = 0; kk < NKB; ++kk) {
                    const int k = lane + 64 * kk;
                    const bool in = k < a.n_bins;
                    const float p = in ? dbs[(fr0 + NW * u) * ldb + k] : 1.0f;
                    bad |= live && !(p <= 3.40282347e+38f);
                    d[u][kk] = to_db(p);
                    mx[u] = fmaxf(mx[u], in ? d[u][kk] : -3.40282347e+38f);
                    mn[u] = fminf(mn[u], in ? d[u][kk] : 3.40282347e+38f);
                }
            }
#pragma unroll
            for (int u = 0; u < FU; ++u) {
                mx[u] = wave_max(mx[u]);
                mn[u] = wave_min(mn[u]);
            }
#pragma unroll
            for (int u = 0; u < FU; ++u) {
                const int fr = fr0 + NW * u;
                if (fr >= n_live) continue;
                const float floor_db = mx[u] - PVQ_TOP_DB;
                const float m2 = fmaxf(mn[u], floor_db);
                float* dst = a.out_db + (size_t)(row0 + (long long)fr * rstep) * a.n_bins;
#pragma unroll
                for (int kk = 0; kk < NKB; ++kk) {
                    const int k = lane + 64 * kk;
                    const float c = fmaxf(d[u][kk], floor_db);
                    if (k < a.n_bins) dst[k] = (m2 > 0.0f) ? (c - m2) : fmaxf(c, 0.0f);
                }
            }
        }
    };
    if (a.n_bins <= 256) {
        in_registers(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
        flag();
        return;
    }
    if (a.n_bins <= 512) {
        in_registers(std::integral_constant<int, 2>{}, std::integral_constant<int, 8>{});
        flag();
        return;
    }
    for (int fr = wave; fr < MT * 32; fr += NW) {
        if (fr >= n_live) break;
        float* rowp = dbs + fr * ldb;
        float mx = -3.40282347e+38f, mn = 3.40282347e+38f;
        for (int k = lane; k < a.n_bins; k += 64) {
            bad |= !(rowp[k] <= 3.40282347e+38f);
            const float d = to_db(rowp[k]);
            rowp[k] = d;
            mx = fmaxf(mx, d);
            mn = fminf(mn, d);
        }
        mx = wave_max(mx);
        mn = wave_min(mn);
        const float floor_db = mx - PVQ_TOP_DB;
        const float m2 = fmaxf(mn, floor_db);
        float* dst = a.out_db + (size_t)(row0 + (long long)fr * rstep) * a.n_bins;
        for (int k = lane; k < a.n_bins; k += 64) {
            const float c = fmaxf(rowp[k], floor_db);
            dst[k] = (m2 > 0.0f) ? (c - m2) : fmaxf(c, 0.0f);
        }
    }
    flag();
}

template <int MT, int NW>   // 32-frame MFMA row tiles per workgroup, waves per workgroup
__global__ __launch_bounds__(64 * NW, NW / 2) void blockdft_banddots_db(BandArgs a) {
    const int stamp_slot = blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) float dbs[];   // [MT * 32][ldb]: |x_vqt|^2, then dB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * (MT * 32);
    const int n = lane & 31, kx = lane >> 5;
    constexpr int col_stride = 128;   // floats between consecutive X columns of a 64-frame tile
    const float* xtile = a.X + ((size_t)(f0 >> 6) * a.xcp) * col_stride + (f0 & 63) * 2;   // this workgroup's frames
    // the output rows of this workgroup's frames: rows f0 ... of a single stream, or what the X tile's entry of the map says
    long long row0 = f0;
    int n_live = a.n_frames - f0, rstep = 1;
    if (a.xmap) {   // (uniform)
        const XTile xt = a.xmap[f0 >> 6];
        rstep = xt.live_step >> 8;
        row0 = xt.out_row0 + (long long)(f0 & 63) * rstep;
        n_live = (xt.live_step & 255) - (f0 & 63);
        if (n_live <= 0) return;   // (uniform) a staged buffer's gap frames: nothing of this tile is wanted (Vqt::batch_streams_device)
    }
    PVQ_STAMP(0);
    const int* my_list = a.list + wave * a.per_wave;
    const int n_blocks = __builtin_amdgcn_readfirstlane(my_list[0]);
    // MT == 2: a lane loads (Re, Im) of one of 64 frames; a half swap then leaves Re of frames 0..31 / Im of frames
    // 0..31 in the two lane halves of one register (the A operand of row tile 0) and frames 32..63 in the other.
    // MT == 1: a lane loads the one float it feeds to the MFMA.
    const float* xa = nullptr;
    const float2* bp = nullptr;   // column pairs
    float2 av[BD_NS][BD_KU], bv[BD_NS][BD_KU / 2];
    auto fetch = [&](int s, int c) {
#pragma unroll
        for (int u = 0; u < BD_KU / 2; ++u) bv[s][u] = bp[(size_t)(c / 2 + u) * 64];
#pragma unroll
        for (int u = 0; u < BD_KU; ++u) {
            if (MT == 2)
                av[s][u] = *reinterpret_cast<const float2*>(xa + (size_t)(c + u) * col_stride);
            else
                av[s][u].x = xa[(size_t)(c + u) * col_stride];
        }
    };
    // point the operand streams at a block and put its first BD_NS - 1 stages in flight
    auto open_block = [&](const BandBlock& blk) {
        xa = MT == 2 ? xtile + (size_t)blk.x0 * col_stride + lane * 2 : xtile + (size_t)blk.x0 * col_stride + n * 2 + kx;
        bp = reinterpret_cast<const float2*>(a.B) + (size_t)blk.boff * 32 + lane;
#pragma unroll
        for (int s = 0; s < BD_NS - 1; ++s) fetch(s, s * BD_KU);
    };
    BandBlock blk{};
    if (n_blocks > 0) {
        blk = a.blocks[__builtin_amdgcn_readfirstlane(my_list[1])];
        open_block(blk);
    }
    for (int bi = 0; bi < n_blocks; ++bi) {
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mt][q] = 0.0f;
        auto mul = [&](int s) {
#pragma unroll
            for (int u = 0; u < BD_KU; ++u) {
                const float b = (u & 1) ? bv[s][u / 2].y : bv[s][u / 2].x;
                if (MT == 2) {
                    float t0 = av[s][u].x, t1 = av[s][u].y;
                    permlane32_swap(t0, t1);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(t0, b, acc[0], 0, 0, 0);
                    acc[MT - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(t1, b, acc[MT - 1], 0, 0, 0);
                } else {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][u].x, b, acc[0], 0, 0, 0);
                }
            }
        };
        // ring of BD_NS stages of BD_KU columns: BD_NS - 1 stages of operands in flight while one is multiplied.
        // kb is a multiple of BD_KU; the fetches run up to (BD_NS - 1) * BD_KU columns past the block (in bounds
        // by construction, never multiplied).
        const int kb = __builtin_amdgcn_readfirstlane(blk.kb);
        const int kb_full = kb - kb % (BD_NS * BD_KU);
        int c = 0;
        for (; c < kb_full; c += BD_NS * BD_KU) {   // steady state: no branches, exact load counting
#pragma unroll
            for (int s = 0; s < BD_NS; ++s) {
                fetch((s + BD_NS - 1) % BD_NS, c + (s + BD_NS - 1) * BD_KU);
                mul(s);
                // keep a stage's lane swaps (and the waits on its operands) inside the stage: the scheduler would
                // otherwise hoist the swaps of later stages to the top and wait for the whole ring
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int s = 0; s < BD_NS - 1; ++s)         // remainder: the operands are already in flight
            if (c + s * BD_KU < kb) mul(s);
        // the next block's first operands fly while this block's results are written out
        const int bin0 = blk.bin0, nrows = blk.nrows;
        if (bi + 1 < n_blocks) {
            blk = a.blocks[__builtin_amdgcn_readfirstlane(my_list[bi + 2])];
            open_block(blk);
        }
        band_writeout<MT, MT == 2 ? BAND_LDB2 : 0>(acc, dbs, a, row0, n_live, rstep, bin0, nrows, lane);
    }
    PVQ_STAMP(1);
    __syncthreads();
    PVQ_STAMP(2);
    band_finish<MT, NW>(dbs, a, row0, n_live, rstep, wave, lane);
    if (a.stamps) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        PVQ_STAMP(3);
    }
}

// 16x16x4 form of the fp32 kernel product (64-frame tiles, up to 304 bins: the default): blocks of 8 bins, so a block walks the union
// of only 8 rows' columns (about 35 instead of 57) — the same products in 39 % fewer matrix-pipe cycles than the 32x32x2 form above.
// Its first version (round 2) fetched 8 bytes per lane — one complex value of one column — and turned four such registers into the
// MFMA operands of the four 16-frame tiles with two v_permlane32_swap + two v_permlane16_swap per column pair: 133-150 us per
// 65 536 frames, bound by its vector-memory instructions.  This form needs NO lane swaps and issues half the loads (16 bytes each):
// 113-125 us on the same boxes.
typedef float f32x4v __attribute__((ext_vector_type(4)));
// Lane (i = lane & 15, kq = lane >> 4) loads 16 bytes of column c + kq: (Re, Im) of the frame PAIR 16 u + i of the tile (frames 32 u + 2 i and + 1), and each
// of its four registers IS an A operand of v_mfma_f32_16x16x4_f32 as it stands: the k slots of an MFMA are the four columns
// c .. c + 3 (Re parts for register 0 / 2, Im parts for 1 / 3), its rows the 16 even (registers 0, 1) or odd (2, 3) frames of the
// half tile u; the B operand of lane (n, kq) is the coefficient of column c + kq for output n (n < 8: re of bin row n, else im),
// one register for the Re parts and one for the Im parts.  Per four columns: two 16-byte X loads and one 8-byte B load per lane
// instead of four 8-byte loads + one, eight MFMAs as before, no swaps.  C layout: output n = lane & 15, frame 32 u + 2 (4 (lane >> 4) + r) + p.
typedef const __attribute__((address_space(4))) i32x4 stage_desc_c;   // a BandStage as the scalar unit loads it
static_assert(sizeof(BandStage) == sizeof(i32x4) && alignof(BandStage) == alignof(i32x4), "blockdft_plan.hpp: BandStage must be one 16-byte load");
template <int NW, int NS, int LDB, int NU>   // LDB: row stride of the LDS tile (4 mod 16, >= bins); NU: half tiles of 32 frames per workgroup (2: a whole X tile; 1 — half a tile, 4 waves, four workgroups per CU — was measured slower: 141-150 against 121 us)
__global__ __launch_bounds__(64 * NW, NU == 2 || NW == 8 ? NW / 2 : NW) void blockdft_banddots4c_db(BandArgs a) {   // (four waves per SIMD)
    // the bin counts an LDS row stride serves (the host's choice of the instantiation): the finish's other size classes fold away
    if constexpr (LDB == 260) __builtin_assume(a.n_bins <= 256);
    else if constexpr (LDB == 308) __builtin_assume(a.n_bins > 256 && a.n_bins <= 304);
    else if constexpr (LDB == 372) __builtin_assume(a.n_bins > 256 && a.n_bins <= 368);   // (257 ... 304 bins come here with the developer knob PVQ_DOTS_F32 behind the split-bf16 GEMM)
    else if constexpr (LDB == 596) __builtin_assume(a.n_bins > 368 && a.n_bins <= 592);
    else if constexpr (LDB == 852) __builtin_assume(a.n_bins > 592 && a.n_bins <= 848);
    else if constexpr (LDB == 1028) __builtin_assume(a.n_bins > 848 && a.n_bins <= 1024);
    const int stamp_slot = blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) float dbs[];   // [64][LDB]: |x_vqt|^2, then dB
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f0 = blockIdx.x * (32 * NU);
    constexpr int col_stride = 128;   // floats between consecutive X columns of a 64-frame tile
    const float* xtile = a.X + ((size_t)(f0 >> 6) * a.xcp) * col_stride + (f0 & 63) * 2;   // (a half-tile workgroup starts at frame pair 16 of its tile)
    // the output rows of this workgroup's frames: rows f0 ... of a single stream, or what the X tile's entry of the map says
    long long row0 = f0;
    int n_live = a.n_frames - f0, rstep = 1;
    if (a.xmap) {   // (uniform)
        const XTile xt = a.xmap[f0 >> 6];
        rstep = xt.live_step >> 8;
        row0 = xt.out_row0 + (long long)(f0 & 63) * rstep;
        n_live = (xt.live_step & 255) - (f0 & 63);
        if (n_live <= 0) return;   // (uniform) a staged buffer's gap frames: nothing of this tile is wanted (Vqt::batch_streams_device)
    }
    PVQ_STAMP(0);
    // The wave's stage stream (BandStage, blockdft_plan.hpp): its blocks' 4-column stages end to end, null stages after the last.  The
    // descriptors are scalar loads through the constant cache, issued two rounds of NS stages before the stage they describe is
    // fetched; the count travels in the kernel arguments.  One operand ring runs over the whole stream: a block boundary is a
    // wave-uniform branch (write-out + accumulator reset) with no load in it, and nothing is fetched that is not multiplied except
    // the null stages (zeroed pad columns of X, zero coefficients: they add +0 to an accumulator that is never written out).
    const stage_desc_c* sl = reinterpret_cast<const stage_desc_c*>(reinterpret_cast<uintptr_t>(a.stages)) + (size_t)wave * a.stage_stride;
    const int n_rounds = a.stage_count[wave] / NS;
    const int n = lane & 15, kq = lane >> 4;
    const unsigned xlane = (unsigned)(kq * col_stride + n * 4);   // a lane's 16 bytes within a stage's four columns
    const float2* bcoef = reinterpret_cast<const float2*>(a.B);
    f32x4 av[NS][NU];
    float2 bv[NS];
    auto fetch = [&](int s, const i32x4& d) {   // uniform base + lane offset: the stage's columns d.x .. d.x + 3, coefficient group d.y
        bv[s] = (bcoef + (size_t)(unsigned)d.y * 64)[(unsigned)lane];
        const float* xs = xtile + (size_t)(unsigned)d.x * col_stride;
#pragma unroll
        for (int u = 0; u < NU; ++u) av[s][u] = *reinterpret_cast<const f32x4*>(xs + u * 64 + xlane);
    };
    i32x4 cur[NS], nxt[NS], far[NS];   // descriptors of this round's stages, of the next round's, of the one after
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        cur[s] = sl[s];
        nxt[s] = sl[NS + s];
    }
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) {
        fetch(s, cur[s]);
        __builtin_amdgcn_sched_barrier(0);   // in ring order: the first round's waits count the loads behind a stage's own
    }
    f32x4v acc[NU][2];   // [half tile u][p: even / odd frames]
    auto reset = [&] {
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[u][p][q] = 0.0f;
    };
    auto mul = [&](int s) {   // independent accumulators between two uses of one
#pragma unroll
        for (int part = 0; part < 2; ++part) {   // Re parts of the four columns, then Im parts
            const float b = part ? bv[s].y : bv[s].x;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][u][part], b, acc[u][0], 0, 0, 0);
                acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][u][2 + part], b, acc[u][1], 0, 0, 0);
            }
        }
    };
    auto writeout = [&](int bin0, int nrows) {
        const bool mine = n < nrows;                  // re columns of live rows
        const int bin = bin0 + n;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float im[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {   // row_ror:8: lane n <- lane n ^ 8 (through a scalar copy: the DPP of a vector element was seen merged across q)
                    const float re_q = acc[u][p][q];
                    im[q] = PVQ_DPP(re_q, 0x128);
                }
                if (mine) {
#pragma unroll
                    // re^2 rounded, then im^2 fused on top: spelled out, so that every instantiation rounds as the block loop's did
                    for (int q = 0; q < 4; ++q) dbs[(32 * u + 8 * kq + 2 * q + p) * LDB + bin] = __builtin_fmaf(im[q], im[q], acc[u][p][q] * acc[u][p][q]);
                    if (a.out_cplx) {
                        int row_stride = a.n_bins;
                        asm volatile("" : "+s"(row_stride));
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int fr = 32 * u + 8 * kq + 2 * q + p;
                            if (fr < n_live) a.out_cplx[(size_t)(row0 + (long long)fr * rstep) * row_stride + bin] = make_float2(acc[u][p][q], im[q]);
                        }
                    }
                }
            }
    };
    reset();
    for (int r = 0; r < n_rounds; ++r) {   // a round: NS stages, ring slots fixed at compile time
        sl += NS;
#pragma unroll
        for (int s = 0; s < NS; ++s) far[s] = sl[NS + s];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            fetch((s + NS - 1) % NS, s == 0 ? cur[NS - 1] : nxt[s - 1]);   // the stage NS - 1 ahead
            mul(s);
            __builtin_amdgcn_sched_barrier(0);   // keep the waits on a stage's operands inside the stage
            if (cur[s].w) {                      // (uniform) the block's last stage
                writeout(cur[s].z, cur[s].w & (BAND_STAGE_LAST - 1));
                reset();
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            cur[s] = nxt[s];
            nxt[s] = far[s];
        }
    }
    PVQ_STAMP(1);
    __syncthreads();
    PVQ_STAMP(2);
    band_finish<NU, NW, LDB>(dbs, a, row0, n_live, rstep, wave, lane);
    if (a.stamps) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        PVQ_STAMP(3);
    }
}


#ifdef PVQ_DEV_KNOBS
// The block loop this kernel had before the stage stream: per block, two dependent descriptor loads, a ring restart and NS - 1
// stages fetched past the block's end.  Same MFMAs in the same order: what the stream form is compared against, bit for bit
// (developer knob PVQ_DOTS_BLOCKS; tests/test_dots_stream_gpu.py, scripts/dev_ab_knob.py).
template <int NW, int NS, int LDB, int NU>
__global__ __launch_bounds__(64 * NW, NU == 2 || NW == 8 ? NW / 2 : NW) void blockdft_banddots4c_blocks_db(BandArgs a) {   // (four waves per SIMD)
    // the bin counts an LDS row stride serves (the host's choice of the instantiation): the finish's other size classes fold away
    if constexpr (LDB == 260) __builtin_assume(a.n_bins <= 256);
    else if constexpr (LDB == 308) __builtin_assume(a.n_bins > 256 && a.n_bins <= 304);
    else if constexpr (LDB == 372) __builtin_assume(a.n_bins > 256 && a.n_bins <= 368);   // (257 ... 304 bins come here with the developer knob PVQ_DOTS_F32 behind the split-bf16 GEMM)
    else if constexpr (LDB == 596) __builtin_assume(a.n_bins > 368 && a.n_bins <= 592);
    else if constexpr (LDB == 852) __builtin_assume(a.n_bins > 592 && a.n_bins <= 848);
    else if constexpr (LDB == 1028) __builtin_assume(a.n_bins > 848 && a.n_bins <= 1024);
    const int stamp_slot = blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) float dbs[];   // [64][LDB]: |x_vqt|^2, then dB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * (32 * NU);
    constexpr int col_stride = 128;   // floats between consecutive X columns of a 64-frame tile
    const float* xtile = a.X + ((size_t)(f0 >> 6) * a.xcp) * col_stride + (f0 & 63) * 2;   // (a half-tile workgroup starts at frame pair 16 of its tile)
    // the output rows of this workgroup's frames: rows f0 ... of a single stream, or what the X tile's entry of the map says
    long long row0 = f0;
    int n_live = a.n_frames - f0, rstep = 1;
    if (a.xmap) {   // (uniform)
        const XTile xt = a.xmap[f0 >> 6];
        rstep = xt.live_step >> 8;
        row0 = xt.out_row0 + (long long)(f0 & 63) * rstep;
        n_live = (xt.live_step & 255) - (f0 & 63);
        if (n_live <= 0) return;   // (uniform) a staged buffer's gap frames: nothing of this tile is wanted (Vqt::batch_streams_device)
    }
    PVQ_STAMP(0);
    const int* my_list = a.list + wave * a.per_wave;
    const int n_blocks = __builtin_amdgcn_readfirstlane(my_list[0]);
    const int n = lane & 15, kq = lane >> 4;
    const float* xa = nullptr;
    const float2* bp = nullptr;
    f32x4 av[NS][NU];
    float2 bv[NS];
    auto fetch = [&](int s, int c) {   // stage: columns c .. c + 3 of the block
        bv[s] = bp[(size_t)(c / 4) * 64];
#pragma unroll
        for (int u = 0; u < NU; ++u) av[s][u] = *reinterpret_cast<const f32x4*>(xa + (size_t)c * col_stride + u * 64);
    };
    auto open_block = [&](const BandBlock& blk) {
        xa = xtile + (size_t)(blk.x0 + kq) * col_stride + n * 4;
        bp = reinterpret_cast<const float2*>(a.B) + (size_t)blk.boff3 * 64 + lane;
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) fetch(s, s * 4);
    };
    BandBlock blk{};
    if (n_blocks > 0) {
        blk = a.blocks[__builtin_amdgcn_readfirstlane(my_list[1])];
        open_block(blk);
    }
    for (int bi = 0; bi < n_blocks; ++bi) {
        f32x4v acc[NU][2];   // [half tile u][p: even / odd frames]
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[u][p][q] = 0.0f;
        auto mul = [&](int s) {   // independent accumulators between two uses of one
#pragma unroll
            for (int part = 0; part < 2; ++part) {   // Re parts of the four columns, then Im parts
                const float b = part ? bv[s].y : bv[s].x;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][u][part], b, acc[u][0], 0, 0, 0);
                    acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][u][2 + part], b, acc[u][1], 0, 0, 0);
                }
            }
        };
        const int kb = __builtin_amdgcn_readfirstlane(blk.kb);
        const int kb_full = kb - kb % (NS * 4);
        int c = 0;
        for (; c < kb_full; c += NS * 4) {   // steady state: no branches, exact load counting
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                fetch((s + NS - 1) % NS, c + (s + NS - 1) * 4);
                mul(s);
                __builtin_amdgcn_sched_barrier(0);   // keep the waits on a stage's operands inside the stage
            }
        }
#pragma unroll
        for (int s = 0; s < NS - 1; ++s)          // remainder: the operands are already in flight
            if (c + s * 4 < kb) mul(s);
        const int bin0 = blk.bin0, nrows = blk.nrows;
        if (bi + 1 < n_blocks) {                      // the next block's first operands fly during the write-out
            blk = a.blocks[__builtin_amdgcn_readfirstlane(my_list[bi + 2])];
            open_block(blk);
        }
        const bool mine = n < nrows;                  // re columns of live rows
        const int bin = bin0 + n;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float im[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {   // row_ror:8: lane n <- lane n ^ 8 (through a scalar copy: the DPP of a vector element was seen merged across q)
                    const float re_q = acc[u][p][q];
                    im[q] = PVQ_DPP(re_q, 0x128);
                }
                if (mine) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) dbs[(32 * u + 8 * kq + 2 * q + p) * LDB + bin] = acc[u][p][q] * acc[u][p][q] + im[q] * im[q];
                    if (a.out_cplx) {
                        int row_stride = a.n_bins;
                        asm volatile("" : "+s"(row_stride));
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int fr = 32 * u + 8 * kq + 2 * q + p;
                            if (fr < n_live) a.out_cplx[(size_t)(row0 + (long long)fr * rstep) * row_stride + bin] = make_float2(acc[u][p][q], im[q]);
                        }
                    }
                }
            }
    }
    PVQ_STAMP(1);
    __syncthreads();
    PVQ_STAMP(2);
    band_finish<NU, NW, LDB>(dbs, a, row0, n_live, rstep, wave, lane);
    if (a.stamps) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        PVQ_STAMP(3);
    }
}
#endif

// Split-bf16 form of the kernel product (the default, with the split-bf16 GEMM): the fp32 MFMA above runs at 1/16
// of the bf16 matrix rate, and a 16-bin block is 73 % zeros, so the stage is matrix-bound.  Here X and the
// coefficients are written as hi + mid + lo bf16 (exact 3-way split, see blockdft_gemm_tree_bf16x3) and eight
// spectrum columns (16 real k) go through six v_mfma_f32_32x32x16_bf16: 6 x 32 cycles instead of 8 x 64.  A lane
// (frame m, half kh) loads (Re, Im) of columns 4 kh .. 4 kh + 3 of its frame — the same bytes per lane as the fp32
// form — and splits them in registers; the coefficient planes come pre-split in B-operand order.

template <int MT, int NW>
__global__ __launch_bounds__(64 * NW, NW / 2) void blockdft_banddots_db_bf16x3(BandArgs a) {
    const int stamp_slot = blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) float dbs[];   // [MT * 32][ldb]: |x_vqt|^2, then dB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * (MT * 32);
    const int n = lane & 31, kx = lane >> 5;
    constexpr int col_stride = 128;   // floats between consecutive X columns of a 64-frame tile
    const float* xtile = a.X + ((size_t)(f0 >> 6) * a.xcp) * col_stride + (f0 & 63) * 2;   // this workgroup's frames
    // the output rows of this workgroup's frames: rows f0 ... of a single stream, or what the X tile's entry of the map says
    long long row0 = f0;
    int n_live = a.n_frames - f0, rstep = 1;
    if (a.xmap) {   // (uniform)
        const XTile xt = a.xmap[f0 >> 6];
        rstep = xt.live_step >> 8;
        row0 = xt.out_row0 + (long long)(f0 & 63) * rstep;
        n_live = (xt.live_step & 255) - (f0 & 63);
        if (n_live <= 0) return;   // (uniform) a staged buffer's gap frames: nothing of this tile is wanted (Vqt::batch_streams_device)
    }
    PVQ_STAMP(0);
    const int* my_list = a.list + wave * a.per_wave;
    const int n_blocks = __builtin_amdgcn_readfirstlane(my_list[0]);
    const float* xa = nullptr;
    const bf16x8* bp = nullptr;
    float2 av[B3_NS][MT][4];
    bf16x8 bv[B3_NS][3];
    auto fetch = [&](int s, int g) {
#pragma unroll
        for (int p = 0; p < 3; ++p) bv[s][p] = bp[((size_t)g * 3 + p) * 64];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) av[s][mt][q] = *reinterpret_cast<const float2*>(xa + (size_t)(8 * g + q) * col_stride + mt * 64);
    };
    auto open_block = [&](const BandBlock& blk) {
        xa = xtile + (size_t)(blk.x0 + 4 * kx) * col_stride + n * 2;
        bp = reinterpret_cast<const bf16x8*>(a.B3) + (size_t)blk.boff3 * 3 * 64 + lane;
#pragma unroll
        for (int s = 0; s < B3_NS - 1; ++s) fetch(s, s);
    };
    BandBlock blk{};
    if (n_blocks > 0) {
        blk = a.blocks[__builtin_amdgcn_readfirstlane(my_list[1])];
        open_block(blk);
    }
    for (int bi = 0; bi < n_blocks; ++bi) {
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mt][q] = 0.0f;
        auto mul = [&](int s) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                bf16x8 vh, vm, vl;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int part = 0; part < 2; ++part) {
                        const float x = part ? av[s][mt][q].y : av[s][mt][q].x;
                        const __bf16 hi = (__bf16)x;
                        const float r1 = x - (float)hi;
                        const __bf16 mid = (__bf16)r1;
                        vh[2 * q + part] = hi;
                        vm[2 * q + part] = mid;
                        vl[2 * q + part] = (__bf16)(r1 - (float)mid);
                    }
                }
                // smallest terms first
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vm, bv[s][1], acc[mt], 0, 0, 0);  // mid*mid
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, bv[s][2], acc[mt], 0, 0, 0);  // hi*lo
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl, bv[s][0], acc[mt], 0, 0, 0);  // lo*hi
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, bv[s][1], acc[mt], 0, 0, 0);  // hi*mid
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vm, bv[s][0], acc[mt], 0, 0, 0);  // mid*hi
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, bv[s][0], acc[mt], 0, 0, 0);  // hi*hi
            }
        };
        const int kg = __builtin_amdgcn_readfirstlane(blk.kg);
        const int kg_full = kg - kg % B3_NS;
        int g = 0;
        for (; g < kg_full; g += B3_NS) {   // steady state: no branches, exact load counting
#pragma unroll
            for (int s = 0; s < B3_NS; ++s) {
                fetch((s + B3_NS - 1) % B3_NS, g + s + B3_NS - 1);
                mul(s);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int s = 0; s < B3_NS - 1; ++s)         // remainder: the operands are already in flight
            if (g + s < kg) mul(s);
        // the next block's first operands fly while this block's results are written out
        const int bin0 = blk.bin0, nrows = blk.nrows;
        if (bi + 1 < n_blocks) {
            blk = a.blocks[__builtin_amdgcn_readfirstlane(my_list[bi + 2])];
            open_block(blk);
        }
        band_writeout<MT, MT == 2 ? BAND_LDB2 : 0>(acc, dbs, a, row0, n_live, rstep, bin0, nrows, lane);
    }
    PVQ_STAMP(1);
    __syncthreads();
    PVQ_STAMP(2);
    band_finish<MT, NW>(dbs, a, row0, n_live, rstep, wave, lane);
    if (a.stamps) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        PVQ_STAMP(3);
    }
}

// kernel product + power_to_db over the launch's X tiles: the form follows the bin count and the GEMM arithmetic
pvq_status Vqt::launch_blockdft_dots(const BlockLaunch& L, float* d_out_db, float* d_out_cplx, hipStream_t stream) {
    BlockDftTables* t = dev_->block;
    const int nb = (int)n_bins();
    const size_t nf = L.nf;
    BandArgs da;
    da.X = reinterpret_cast<const float*>(t->d_X);
    da.xcp = L.xcp;
    da.n_frames = (int)nf;
    da.n_bins = nb;
    // 4 rows apart (the two lane halves of a C tile) land 16 banks apart; the 64-frame form has the stride compiled in
    // more than 256 bins (32-frame tiles): the smallest stride >= n_bins that is 4 mod 16, so that up to 596 bins still fit two workgroups per CU
    // 64-frame tiles while two 64-row tiles fit a CU: up to 256 bins (stride 260) or up to 304 (stride 308; fp32 8-bin form only)
    const bool wide308 = !gemm_split_bf16_ && t->n_bins_pad > 256 && nb <= BAND_LDB3 - 4;
    const bool wide = t->n_bins_pad <= 256 || wide308;
    da.ldb = wide308 ? BAND_LDB3 : wide ? BAND_LDB2 : ((nb + 11) / 16 * 16 + 4);
    da.blocks = t->d_band;
    da.B = t->d_band_B;
    da.B3 = t->d_band_B3;
    da.list = t->d_band_list;
    da.per_wave = t->band_per_wave;
    da.stages = nullptr;
    da.stage_stride = 0;
    std::fill(da.stage_count, da.stage_count + 8, 0);
    // one run: its rows follow each other from its first output row; several: the X-tile map names every tile's rows
    da.xmap = L.d_xmap;
    const size_t row_first = L.multi ? 0 : (size_t)L.shape->segs[0].out_row0;
    da.out_db = d_out_db + row_first * nb;
    da.out_cplx = d_out_cplx ? reinterpret_cast<float2*>(d_out_cplx) + row_first * nb : nullptr;
    da.status = dev_->d_status;
    static const char* dstamps_env = dev_knob_str("PVQ_STAMPS_DOTS");   // dump per-workgroup phase stamps of the first launch
    static bool dstamps_done = false;
    const bool do_dstamps = dstamps_env && !dstamps_done;
    da.stamps = nullptr;
    const size_t n_wg = (nf + 63) / 32;   // upper bound of the grid
    if (do_dstamps) PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&da.stamps), n_wg * 8 * 8));
    if (do_dstamps) PVQ_HIP(hipMemset(da.stamps, 0, n_wg * 8 * 8));
    slot_begin(SLOT_BLOCKDFT_DOTS, stream);
    const int mt = wide ? 2 : 1;
    static const int dots_f32_env = dev_knob("PVQ_DOTS_F32", 0);
    const bool dots_split = gemm_split_bf16_ && !dots_f32_env;   // the kernel product follows the GEMM arithmetic
#ifdef PVQ_DEV_KNOBS
    static const int dots16_env = dev_knob("PVQ_DOTS_16BIN", 0);   // the 16-bin 32x32x2 form wherever it fits
    static const int dots_blocks_env = dev_knob("PVQ_DOTS_BLOCKS", 0);   // the 8-bin form's block loop instead of its stage stream (A/B, bit identity)
#else
    constexpr int dots16_env = 0;
#endif
    const size_t lds = sizeof(float) * 32 * mt * da.ldb;
    const dim3 grid((unsigned)((nf + 32 * mt - 1) / (32 * mt)));
    auto use_8bin_blocks = [&] {   // 8-bin blocks, 16x16x4 MFMAs, the no-swap coefficient order
        da.blocks = t->d_band8;
        da.list = t->d_band_list8;
        da.per_wave = t->band_per_wave8;
        da.B = t->d_band_B4;
        da.stages = t->d_band_stages8;
        da.stage_stride = t->band_stage_stride8;
        std::copy(t->band_stage_count8, t->band_stage_count8 + 8, da.stage_count);
    };
    if (dots_split) {
        da.list = t->d_band_list + (size_t)t->band_waves * t->band_per_wave;   // the 4-wave lists
        if (mt == 2)
            hipLaunchKernelGGL((blockdft_banddots_db_bf16x3<2, 4>), grid, dim3(256), lds, stream, da);
        else
            hipLaunchKernelGGL((blockdft_banddots_db_bf16x3<1, 4>), grid, dim3(256), lds, stream, da);
#ifdef PVQ_DEV_KNOBS
    } else if (mt == 2 && dots16_env && !wide308) {
        hipLaunchKernelGGL((blockdft_banddots_db<2, 8>), grid, dim3(512), lds, stream, da);
#endif
    } else if (mt == 2) {
        use_8bin_blocks();
#ifdef PVQ_DEV_KNOBS
        if (dots_blocks_env) {
            if (wide308)
                hipLaunchKernelGGL((blockdft_banddots4c_blocks_db<8, BD8_NS, BAND_LDB3, 2>), grid, dim3(512), lds, stream, da);
            else
                hipLaunchKernelGGL((blockdft_banddots4c_blocks_db<8, BD8_NS, BAND_LDB2, 2>), grid, dim3(512), lds, stream, da);
        } else
#endif
        if (wide308)
            hipLaunchKernelGGL((blockdft_banddots4c_db<8, BD8_NS, BAND_LDB3, 2>), grid, dim3(512), lds, stream, da);
        else
            hipLaunchKernelGGL((blockdft_banddots4c_db<8, BD8_NS, BAND_LDB2, 2>), grid, dim3(512), lds, stream, da);
    } else if (dots16_env || nb > 1024 - 4) {
        hipLaunchKernelGGL((blockdft_banddots_db<1, 8>), grid, dim3(512), lds, stream, da);
    } else {
        // more than 304 bins (the reference's default 588, 360, 840): the 8-bin / 16x16x4 / no-swap form on HALF tiles (32 frames x all bins
        // per workgroup, 8 waves), its LDS row stride compiled in per class of bin counts — round 5; before, these geometries ran the
        // 16-bin 32x32x2 form (PVQ_DOTS_16BIN=1 in the developer library)
        use_8bin_blocks();
        const int ldb_c = nb <= 368 ? 372 : nb <= 592 ? 596 : nb <= 848 ? 852 : 1028;
        da.ldb = ldb_c;
        const size_t lds_c = sizeof(float) * 32 * ldb_c;
        auto launch_c = [&](auto kern) -> pvq_status {
            if (lds_c > 64 * 1024) PVQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c));
            hipLaunchKernelGGL(kern, grid, dim3(512), lds_c, stream, da);
            return PVQ_OK;
        };
#ifdef PVQ_DEV_KNOBS
        if (dots_blocks_env) {
            pvq_status lbs = ldb_c == 372 ? launch_c(blockdft_banddots4c_blocks_db<8, BD8_NS, 372, 1>) : ldb_c == 596 ? launch_c(blockdft_banddots4c_blocks_db<8, BD8_NS, 596, 1>)
                             : ldb_c == 852 ? launch_c(blockdft_banddots4c_blocks_db<8, BD8_NS, 852, 1>) : launch_c(blockdft_banddots4c_blocks_db<8, BD8_NS, 1028, 1>);
            if (lbs != PVQ_OK) return lbs;
        } else
#endif
        {
            pvq_status lcs = ldb_c == 372 ? launch_c(blockdft_banddots4c_db<8, BD8_NS, 372, 1>) : ldb_c == 596 ? launch_c(blockdft_banddots4c_db<8, BD8_NS, 596, 1>)
                             : ldb_c == 852 ? launch_c(blockdft_banddots4c_db<8, BD8_NS, 852, 1>) : launch_c(blockdft_banddots4c_db<8, BD8_NS, 1028, 1>);
            if (lcs != PVQ_OK) return lcs;
        }
    }
    slot_end(SLOT_BLOCKDFT_DOTS, stream);
    if (do_dstamps) {
        dstamps_done = true;
        return dump_stamps(dstamps_env, da.stamps, n_wg * 8, stream);
    }
    return PVQ_OK;
}

}  // namespace pvq
