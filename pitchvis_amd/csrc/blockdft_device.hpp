// blockdft_device.hpp — what the three units of the block-DFT path share (vqt_blockdft.hip: host side; blockdft_gemm.hip: hop-DFT
// GEMM + combine tree; blockdft_dots.hip: kernel product + power_to_db).  Included by those three only; nothing here is a kernel.
#pragma once

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "blockdft_plan.hpp"
#include "device_tables.hpp"
#include "vqt_engine.hpp"

namespace pvq {

static_assert(sizeof(Float2) == sizeof(float2) && alignof(Float2) == alignof(float2), "blockdft_plan.hpp: Float2 must match float2");
static_assert(sizeof(Float4) == sizeof(float4) && alignof(Float4) == alignof(float4), "blockdft_plan.hpp: Float4 must match float4");
static_assert(sizeof(Int4) == sizeof(int4) && alignof(Int4) == alignof(int4), "blockdft_plan.hpp: Int4 must match int4");

constexpr int CB_T = 128;    // frames per combine workgroup
constexpr int FT_BM = 128, FT_BN = 64;   // rows of a fused GEMM tile (the kernels' default), floats per column tile
constexpr int BAND_LDB2 = 260;   // the 64-frame form: up to 256 bins + 4 (rows 4 apart land 16 banks apart)
constexpr int BAND_LDB3 = 308;   // the 64-frame 8-bin form up to 304 bins (78.8 KB: still two workgroups per CU)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// developer knobs PVQ_STAMPS / PVQ_STAMPS_DOTS: a workgroup's phase stamp i (the kernel argument struct `a` carries the dump)
#define PVQ_STAMP(i) \
    if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)stamp_slot * 8 + (i)] = wall_clock64();   // stamp_slot: the tile's (workgroup's) row of the dump

struct BlockDftTables {
    size_t hop = 0;
    int n_groups = 0;
    int n_tiles = 0;   // total column tiles; Ntot = n_tiles*64 floats, XC = n_tiles*32 complex
    int nb_max = 0;
    int n_bins_pad = 0;
    std::vector<BlockGroup> groups;
    std::vector<float> h_E;        // host copy of E
    float* d_E = nullptr;          // [hop][Ntot]
    __bf16* d_Et = nullptr;        // [3][Ntot][hop] hi/mid/lo bf16 planes of E^T (split-bf16 GEMM), built on first use
    int* d_tile_group = nullptr;   // [n_tiles]
    long long* d_tile_s = nullptr; // [n_tiles] window begin of the tile's group relative to the buffer end
    BlockGroup* d_groups = nullptr;
    float2* d_comb_tw = nullptr;
    // banded kernel product: blocks of 16 output bins x their union of spectrum columns, as MFMA B operands
    struct BandBlock* d_band = nullptr;
    float* d_band_B = nullptr;     // per block and column: 64 floats in v_mfma_f32_32x32x2_f32 B-operand lane order
    __bf16* d_band_B3 = nullptr;   // per block and 8 columns: 3 planes x 64 lanes x 8 bf16 in v_mfma_f32_32x32x16_bf16 order
    // 8-bin blocks for the 16x16x4 MFMA form of the kernel product (fp32, 64-frame tiles)
    struct BandBlock* d_band8 = nullptr;
    float* d_band_B4 = nullptr;    // per block and 4 columns: 64 x (Re coefficient, Im coefficient): the no-swap form
    int* d_band_list8 = nullptr;   // [8][band_per_wave8]
    int band_per_wave8 = 0;
    struct BandStage* d_band_stages8 = nullptr;   // [8][band_stage_stride8]: the 8-bin blocks as one stage stream per wave
    int band_stage_stride8 = 0;
    int band_stage_count8[8] = {};
    int* d_band_list = nullptr;    // [band_waves][band_per_wave]: per wave of a workgroup, the count and then the blocks it walks
    int band_per_wave = 0;
    int band_waves = 4;            // waves per kernel-product workgroup (8 when the 64-frame form is used)
    float* d_P = nullptr;  size_t p_cap = 0;   // workspace
    float2* d_X = nullptr; size_t x_cap = 0;
    float2* d_Y = nullptr; size_t y_cap = 0;   // 64-block partial sums (windows of more than 64 blocks)
    // frame-stripe tile order of the fused kernels, built per launch shape and kept for the next launch
    struct TileList {
        int4* d = nullptr; size_t cap = 0;            // device: the list, then the launch's segment table and X-tile map
        const struct SegDev* d_segs = nullptr;
        const struct XTile* d_xmap = nullptr;
        std::vector<SegKey> key;                      // the runs the list was built for (stream geometry included: which tiles may pair up / take 16-byte loads)
        int bm = 0, wide = 0, blocks = 0, kind = 0;   // kind: 0 power-of-two hop (GEMM + tree); 1 / 2: R / Q tiles of a general hop
        bool multi = false;
        double eff_tiles = 0.0;                       // MFMA work of the list in whole 32-column tiles
        double eff_flop = 0.0;                        // ... in flop (general hops: the depth differs by tile kind and group)
        std::vector<size_t> slot_data;                // the staged streams' slots the X-tile map was built from (compared by content: the key's slot_hash alone is a hash)
    } tile_lists[8];   // eight slots: a batch's first, middle and last sub-batch alternate without rebuilding; a general hop takes two lists per launch shape
    int tile_list_next = 0;
    unsigned long long* d_clk = nullptr; size_t clk_cap = 0; int clk_n = 0;   // K-loop clock samples of the last profiled launch: 4 slots per sampled tile
    float4* d_E16 = nullptr;       // E in the B-operand order of the 16x16x4 GEMM: [column tile][k < hop / 2][n < 16]; behind the n_tiles column tiles
                                   // the merged slices of the mixed tiles, one per pair of `mixed`
    std::vector<MixedPair> mixed;  // the pairs of groups whose last column tiles share a mixed tile (blockdft_plan.hpp)
    bool general = false;          // the hop does not divide the windows: blockdft_gemm_gen (whole hop blocks + the window's remainder)
    float4* d_E16R = nullptr;      // general hops: per group and column tile [k < rem / 2][n < 16]
    float2* d_gen_tw = nullptr;    // general hops: per group phi, tau (n_tiles * 32 columns each)
};

// grow-only device buffer: freed and allocated anew when `bytes` exceed its capacity
template <typename T>
static pvq_status grow(T** ptr, size_t* cap, size_t bytes, bool* grown = nullptr) {
    if (grown) *grown = false;
    if (*cap >= bytes) return PVQ_OK;
    if (*ptr) PVQ_HIP(hipFree(*ptr));
    *ptr = nullptr;
    *cap = 0;
    PVQ_HIP(hipMalloc(reinterpret_cast<void**>(ptr), bytes));
    *cap = bytes;
    if (grown) *grown = true;
    return PVQ_OK;
}

// What the stages of one launch share.  X is blocked by 64-frame tiles: [tile][column][64 frames], so the kernel-product workgroup
// of a tile streams one contiguous region (and a column step is a constant 512 bytes); X_PAD_COLS zeroed columns close every tile.
struct BlockLaunch {
    const LaunchShape* shape;
    const std::vector<BdRun>* runs;
    const BdStream* streams;
    bool use_bf;               // the split-bf16 GEMM
    bool multi;                // several runs, or one whose rows go through the X-tile map: the launch reads the segment table
    const float* pcm_base;     // the launch's base pointer (a launch of one run: that run's rebased stream pointer, as the single-stream entry point always did)
    size_t nf;                 // frames the per-frame stages of the launch cover
    size_t rows_cap;           // row capacity of the unfused stages' P
    int ntot, xcp;             // floats per row of E; columns per frame tile of X (incl. the zeroed pad columns)
    const XTile* d_xmap;       // set by the fused GEMM stage: the X-tile map of a multi launch (else nullptr)
};

// developer knobs PVQ_STAMPS / PVQ_STAMPS_DOTS: the phase stamps of one launch to a file, once the launch has finished
inline pvq_status dump_stamps(const char* path, unsigned long long* d_stamps, size_t n_words, hipStream_t stream) {
    std::vector<unsigned long long> h(n_words);
    PVQ_HIP(hipStreamSynchronize(stream));
    PVQ_HIP(hipMemcpy(h.data(), d_stamps, h.size() * 8, hipMemcpyDeviceToHost));
    PVQ_HIP(hipFree(d_stamps));
    if (FILE* fp = fopen(path, "wb")) {
        fwrite(h.data(), 8, h.size(), fp);
        fclose(fp);
    }
    return PVQ_OK;
}

}  // namespace pvq
