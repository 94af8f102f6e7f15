// blockdft_plan.hpp — host planning of the block-DFT path (vqt_blockdft.hip): the tables the kernels read, how streams are cut
// into runs and launches, and the fused kernels' tile lists.  Plain data in, plain data out: no HIP, no device pointer, no
// environment.  Compiled by g++ with the other host units and replayed under ASan / UBSan by tests/sanitize/host_main.cpp.
//
// The structs below are read by the kernels as they are laid out here (BlockGroup travels by value in the kernel arguments);
// blockdft_device.hpp asserts that Float2 / Float4 / Int4 have the size and alignment of HIP's float2 / float4 / int4.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "vqt_host.hpp"

namespace pvq {

struct alignas(8) Float2 { float x, y; };
struct alignas(16) Float4 { float x, y, z, w; };
struct alignas(16) Int4 { int x, y, z, w; };

constexpr int GM_BN = 64;   // granularity of the column tiling: 64 floats = 32 complex spectrum columns
constexpr int CB_C = GM_BN / 2;  // complex columns per combine workgroup
constexpr int CB_MAX_NB = 256;  // hop blocks per window the combine tree supports (<= 64: 32-column tiles, else 16)
constexpr int GEN_MAX_NQ = 16;   // general hops: whole blocks per window the combine takes (the P tile's 15 spare rows are its halo)
constexpr int FB_BK = 32;   // K step of the split-bf16 GEMM: the hops it takes are multiples of it
constexpr int BD_RB = 16;   // bins per block: 32 MFMA columns = 16 x (re, im)
constexpr int BD_KU = 4;    // columns per software-pipeline stage
constexpr int BD_NS = 4;    // pipeline stages
constexpr int BD8_RB = 8;   // bins per block of the 16x16x4 form
constexpr int BD8_KU = 4;   // columns per stage (two column pairs = two MFMAs per 16-frame tile)
constexpr int BD8_NS = 4;   // stages in the operand ring
constexpr int B3_NS = 3;    // split-bf16 kernel product: 8-column stages in flight
constexpr int X_PAD_COLS = 32;   // zeroed columns after the last X column (the operand prefetch runs past a block's range)

struct BlockGroup {
    int nb;         // hop blocks per window
    int levels;     // log2(nb)
    int n_cols;     // spectrum columns used
    int tile0;      // first GEMM column tile of this group
    int n_tiles;    // column tiles (of 32 complex columns)
    int tw_off;     // into comb_tw: levels x (n_tiles*32) entries
    long long s_rel;  // window begin relative to the end of the n_fft buffer: w0 - n_fft
    int nb_f;       // blocks summed inside the fused kernel: min(nb, 64); the remaining levels run in blockdft_tree_finish
    int levels_f;   // log2(nb_f)
    // general hops (a multiple of 64 that does not divide the window, blockdft_gemm_gen): window = nq whole hop blocks + rem samples
    int nq, rem;
    int e16r_off;   // Float4 index of the group's slices of E16R (the DFT matrix of the first rem samples of a block)
    int gtw_off;    // Float2 index into gen_tw: phi (n_tiles * 32 columns), then tau
};

// a block of output bins (rows of one window group's kernel) and the contiguous range of X columns they read
struct BandBlock {
    int x0;      // first X column
    int kb;      // columns walked (multiple of the form's K unit; coefficients beyond the true range are zero)
    int boff;    // first column of this block in its coefficient array (units of 64 floats)
    int bin0;    // first output bin
    int nrows;   // 1..16 (8-bin form: 1..8)
    int kg;      // 8-column groups walked by the split-bf16 form
    int boff3;   // 16-bin blocks: first group in band_B3 (units of 3 planes x 64 lanes x 8 bf16); 8-bin blocks: first 4-column group in band_B4
};

// One 4-column stage of an 8-bin block, as blockdft_banddots4c_db walks a wave's blocks: one stream of stages per wave, the
// blocks' stages one after the other in the order the wave was dealt them.  The kernel reads the entries through the constant cache.
constexpr int BAND_STAGE_LAST = 1 << 8;
struct alignas(16) BandStage {
    int x;      // first X column of the stage: x0 + 4 s
    int b;      // its 4-column coefficient group in band_B4: boff3 + s
    int bin0;   // a block's last stage: the block's first output bin (else 0)
    int fin;    // a block's last stage: nrows | BAND_STAGE_LAST (else 0)
};

// MANY streams in one launch (pvq_vqt_*_streams: the trainer's shape, pitchvis_train/src/train.rs:146-163 — many files side by side).
// A launch covers a list of SEGMENTS, each a contiguous run of frames of one stream; a tile list entry names its segment
// (.x bits 16..31), the segment table gives the tile its stream (offset from the launch's base pointer, readable bytes, where
// frame 0 of the run ends) and the run's first 64-frame tile in X / Y; XTile maps an X tile back to the output rows it holds.
struct alignas(16) SegDev {
    long long pcm_off;    // samples from the launch's base pointer to the segment's rebased stream pointer
    long long base;       // index, relative to that pointer, of the end of the segment's frame 0
    unsigned pcm_bytes;   // bytes readable from that pointer
    int n_frames;         // frames of the segment
    int x_tile0, y_tile0; // its first 64-frame tile in X / in Y
};
struct XTile {
    long long out_row0;   // output row (of out_db, masks, ...) of the tile's frame 0
    int live_step;        // bits 0..7: frames of the tile that exist (<= 64); bits 8..: output rows between consecutive frames (1, or r
                          // for a run that holds every r-th frame of its stream: Vqt::run_batch's interleaved block grids)
    int y_tile;           // the Y tile that holds the same frames' 64-block partial sums
};

// one run of a launch on the host: what decides its tiles, where its frames go
struct SegKey {
    long long pcm_off, base, out_row0;
    unsigned pcm_bytes;
    int nf, x_tile0, y_tile0, row_step;
    unsigned long long slot_hash;   // a run over a staged buffer of many streams: hash of its slots (0: none), its grid offset and first frame
    long long grid_i, fbeg;
    bool operator==(const SegKey& o) const {
        return pcm_off == o.pcm_off && base == o.base && out_row0 == o.out_row0 && pcm_bytes == o.pcm_bytes && nf == o.nf && x_tile0 == o.x_tile0 && y_tile0 == o.y_tile0 &&
               row_step == o.row_step && slot_hash == o.slot_hash && grid_i == o.grid_i && fbeg == o.fbeg;
    }
};

// Two window groups whose partial last column tiles share one MIXED tile of the fp32 fused kernel: one 32-column tile whose columns
// [0, n1) are the last column tile of g1 and whose columns [n1, n1 + n2) are the last column tile of g2 — one K loop over the PCM
// rows both groups read, one epilogue, instead of a workgroup life each.  A pair forms only where both groups run the fused
// power-of-two path without Y partial sums (nb == nb_f), their windows begin a whole number of hops apart and n1 + n2 <= 32.
struct MixedPair {
    int g1, g2;   // g1: the group of more hop blocks, on whose row grid (stride 257 - nb_1) the mixed tile lives
    int n1, n2;   // columns the two last tiles hold
    int d;        // (s_rel_1 - s_rel_2) / hop: row j of a mixed tile at f0 is frame f0 + j of g1 and frame f0 + j + d of g2
};
constexpr int MIXED_MAX_PAIRS = 4;        // (the fused path takes at most 8 window groups)
constexpr int TILE_MIXED = 1 << 9;        // tile list entry .x: bit 9 a mixed entry, bits 10..12 its second group, bits 13..15 the pair
constexpr int TILE_MIXED_G2_SHIFT = 10, TILE_MIXED_PAIR_SHIFT = 13;

// ---- tables ----------------------------------------------------------------------------------------------------------------------
bool blockdft_plan_applicable(const HostPlan& plan, size_t hop);   // whether the path's kernels take this geometry at this hop

struct BlockDftHostTables {
    bool general = false;          // the hop does not divide the windows: blockdft_gemm_gen (whole hop blocks + the window's remainder)
    int n_tiles = 0;               // total column tiles; Ntot = n_tiles*64 floats, XC = n_tiles*32 complex
    int nb_max = 0;
    int n_bins_pad = 0;
    std::vector<BlockGroup> groups;
    std::vector<float> E;          // [hop][Ntot], (cos, sin) interleaved per column
    std::vector<Float4> E16;       // E in the B-operand order of the 16x16x4 GEMM: [column tile][k < hop / 2][n < 16]
    std::vector<Float4> E16R;      // general hops: per group and column tile [k < rem / 2][n < 16]
    std::vector<MixedPair> mixed;  // the pairs of groups whose last column tiles may share a mixed tile (plan_mixed_pairs)
    std::vector<Float4> E16M;      // per pair one merged slice in the format of E16: its columns [0, n1) g1's last tile, [n1, n1 + n2) g2's, zeros
                                   // behind them; on the device it follows the regular column tiles of E16 (pair m is column tile n_tiles + m)
    std::vector<Float2> comb_tw;   // tree twiddles: per group [level][n_tiles * 32]
    std::vector<Float2> gen_tw;    // general hops: per group phi, tau (n_tiles * 32 columns each)
    std::vector<int> tile_group;   // [n_tiles]
    std::vector<long long> tile_s; // [n_tiles] window begin of the tile's group relative to the buffer end
    // banded kernel product: blocks of 16 output bins x their union of spectrum columns, as MFMA B operands
    std::vector<BandBlock> band;
    std::vector<float> band_B;        // per block and column: 64 floats in v_mfma_f32_32x32x2_f32 B-operand lane order
    std::vector<uint16_t> band_B3;    // per block and 8 columns: 3 planes x 64 lanes x 8 bf16 in v_mfma_f32_32x32x16_bf16 order
    std::vector<int> band_list;       // [band_waves + 4][band_per_wave]: per wave of a workgroup, the count and then the blocks it walks
    int band_per_wave = 0;
    int band_waves = 8;               // waves per workgroup of the fp32 forms (the split-bf16 form's 4-wave lists follow them)
    // 8-bin blocks for the 16x16x4 MFMA form of the kernel product
    std::vector<BandBlock> band8;
    std::vector<float> band_B4;       // per block and 4 columns: 64 x (Re coefficient, Im coefficient): the no-swap form
    std::vector<int> band_list8;      // [8][band_per_wave8]
    int band_per_wave8 = 0;
    // the same blocks as one stage stream per wave: row w holds the stages of wave w's blocks of band_list8, then null stages (the
    // zeroed pad columns of X times the zero pad of band_B4) up to band_stage_count8[w], a multiple of BD8_NS, and on to the end of
    // the row: the ring's last BD8_NS - 1 operand fetches and the descriptor reads two rounds ahead stay inside it
    std::vector<BandStage> band_stages8;   // [8][band_stage_stride8]
    int band_stage_stride8 = 0;            // max count + 2 BD8_NS
    int band_stage_count8[8] = {};         // stages wave w multiplies
};
// false (with the text in *err): the geometry has too many spectrum columns for the path
bool build_blockdft_tables(const HostPlan& plan, size_t hop, bool twiddle_fp16, BlockDftHostTables& out, std::string* err);
// Which groups pair up (MixedPair), greedily among the partial last tiles that stay single entries of the tile list (at most 16 columns,
// or the odd tile of a group), nearest block counts first and of those the longer windows first; nothing for a general hop
std::vector<MixedPair> plan_mixed_pairs(const std::vector<BlockGroup>& groups, size_t hop, bool general);
// hi / mid / lo bf16 planes of E^T, [3][Ntot][hop] (the split-bf16 GEMM's operand)
std::vector<uint16_t> build_Et_bf16x3(const std::vector<float>& E, int ntot, size_t hop);

// ---- streams -> runs -> launches -------------------------------------------------------------------------------------------------
struct BdSlot { size_t vframe0, n_frames, out_row0; };   // frames [vframe0, vframe0 + n_frames) of a staged buffer -> rows out_row0 ...
// One run of frames as the planner sees it (StreamRun, batch_plan.hpp, with the stream pointer as a sample offset from the launch's base pointer)
struct BdStream {
    long long pcm_off;
    size_t first_end, n_samples, n_frames, out_row0, row_step;
    const BdSlot* slots;
    size_t n_slots, grid_i;
    uint64_t slot_hash;
};
struct BdRun { size_t stream, fbeg, nf; };
// every stream cut into runs of at most `chunk` frames; a launch holds runs of whole 64-frame tiles up to `chunk` frames
std::vector<std::vector<BdRun>> pack_runs(const BdStream* st, size_t n_st, size_t chunk);

struct LaunchShape {
    std::vector<SegKey> segs;               // one per run, each stream rebased so that every byte offset of the launch fits 32 bits
    size_t x_tiles = 0, y_tiles = 0;        // 64-frame tiles of X / Y the launch fills
    size_t n_frames = 0;
    bool strided = false;                   // a run holds every r-th frame of its stream, or reads a staged buffer: its rows go through the X-tile map
    std::vector<size_t> slot_data;          // the staged streams' slots by content (runs of one buffer share one slot list: taken once)
};
LaunchShape launch_shape(const BdStream* st, const std::vector<BdRun>& runs, size_t hop, size_t n_fft, int nb_max);
void build_segment_map(const BdStream* st, const std::vector<BdRun>& runs, const LaunchShape& shape, std::vector<SegDev>& segs, std::vector<XTile>& xmap);

// ---- tile lists of the fused kernels ---------------------------------------------------------------------------------------------
struct TileListOptions {
    int fs = 2048;       // frames per stripe
    int balance = 1;     // 0: queues as the stripes fall
    int tail = 128;      // narrow entries at the end of every queue (wide_mode 1)
    std::vector<MixedPair> mixed;   // the pairs whose last tiles share mixed entries (kind 0, 256-row fp32 kernel only); empty: none
};
struct HostTileList {
    std::vector<Int4> list;    // (group | wide << 8 | mixed bits 9..15 | segment << 16, column tile, first frame, position); length a multiple of 8
    double eff_tiles = 0.0;    // MFMA work of the list in whole 32-column tiles
    double eff_flop = 0.0;     // ... in flop (general hops: the depth differs by tile kind and group)
};
// kind 0: the tiles of a power-of-two hop (GEMM + tree); 1 / 2: the remainder / whole-block tiles of a general hop
bool tile_inside_stream(const BlockGroup& G, const SegKey& seg, int f0, size_t hop, int bm, int kind);
HostTileList build_tile_list(const std::vector<BlockGroup>& groups, const std::vector<SegKey>& segs, size_t hop, int bm, int wide_mode, int kind,
                             const TileListOptions& opt);
// matrix work of a launch of the fused GEMM + tree kernels in whole-tile units, for tiles of bm rows (mixed: the pairs whose last
// tiles share mixed entries — g2's last tile then issues nothing of its own, g1's a whole tile, or half of one up to 16 columns)
double fused_tile_count(const std::vector<BlockGroup>& groups, const std::vector<SegKey>& segs, int bm, bool split_bf16,
                        const std::vector<MixedPair>* mixed = nullptr);

}  // namespace pvq
