// blockdft_plan.cpp — host planning of the block-DFT path: see blockdft_plan.hpp.
#include "blockdft_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace pvq {

// round-to-nearest-even bf16 of a finite float
static inline uint16_t host_to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float host_from_bf16(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// x = hi + mid + lo in bf16 (each the nearest bf16 of what the ones before it left over)
static inline void split_bf16x3(float x, uint16_t& hi, uint16_t& mid, uint16_t& lo) {
    hi = host_to_bf16(x);
    const float r1 = x - host_from_bf16(hi);
    mid = host_to_bf16(r1);
    lo = host_to_bf16(r1 - host_from_bf16(mid));
}
// the nearest fp16 (ties to even) of a twiddle factor, as a float: what device_tables' round_to_half gives for |x| <= 1
static float round_to_half(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t sign = u & 0x80000000u;
    u &= 0x7fffffffu;
    if (u < 0x38800000u) {   // below 2^-14: fp16 subnormals, multiples of 2^-24 = the spacing of floats in [0.5, 1)
        float a;
        std::memcpy(&a, &u, 4);
        volatile float s = a + 0.5f;
        a = s - 0.5f;
        std::memcpy(&u, &a, 4);
    } else {
        u += 0xfffu + ((u >> 13) & 1u);
        u &= ~0x1fffu;
    }
    u |= sign;
    std::memcpy(&x, &u, 4);
    return x;
}

bool blockdft_plan_applicable(const HostPlan& plan, size_t hop) {
    if (hop < 64 || hop % 64 != 0 || hop > 4096) return false;   // the mirrored K loop walks hop / 2 in stages of 32
    if (plan.params.range.n_buckets() > 1024) return false;
    const auto& groups = plan.kernel.window_groups;
    bool divides = (hop & (hop - 1)) == 0;
    for (const WindowGroup& g : groups) divides = divides && g.window_size() % hop == 0;
    if (divides) {   // power-of-two hop dividing every window: hop-block GEMM + doubling tree
        for (const WindowGroup& g : groups)
            if (g.window_size() / hop > (size_t)CB_MAX_NB) return false;
        return true;
    }
    // general hop (a multiple of 64): whole hop blocks + the window's remainder, combined by Horner's rule over at most GEN_MAX_NQ blocks;
    // the fused kernel only (at most 8 window groups), windows a multiple of 64 samples
    if (groups.size() > 8) return false;
    for (const WindowGroup& g : groups) {
        const size_t ws = g.window_size();
        if (ws % 64 != 0 || ws / hop > (size_t)GEN_MAX_NQ) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// tables
// ------------------------------------------------------------------------------------------------
namespace {

// Only the spectrum columns some kernel row actually reads are computed (e.g. 602 of 871 at 48 kHz / 7x36):
// col_of[g][i] is the i-th used column of group g, idx_of[g][c] its compressed index, rho[g][i] the phase the GEMM stages leave out.
struct Columns {
    std::vector<std::vector<uint32_t>> col_of;
    std::vector<std::vector<int>> idx_of;
    std::vector<std::vector<std::pair<double, double>>> rho;
};

// element (column c, lane l) of a 16-bin block: columns are stored in pairs, at [(c / 2) * 64 + l] * 2 + (c & 1);
// lane l = kk * 32 + part * 16 + row (kk: 0 multiplies Re X, 1 Im X; part: 0 -> re, 1 -> im of the output)
inline size_t band16_lane_index(int c, int l) { return ((size_t)(c >> 1) * 64 + l) * 2 + (c & 1); }
inline size_t band16_index(int c, int kk, int part, int row) { return band16_lane_index(c, kk * 32 + part * 16 + row); }
// an 8-bin block in the order of blockdft_banddots4c_db: per 4 columns and lane (column of the group, n = part * 8 + row) a pair
// (coefficient of Re X, coefficient of Im X)
inline size_t band8_index(int c, int kk, int part, int row) { return ((size_t)(c >> 2) * 64 + (c & 3) * 16 + part * 8 + row) * 2 + kk; }

// Banded kernel product tables: per window group, blocks of `rb` consecutive bins; a block walks the union of its rows' (compressed)
// columns, rounded up to `ku`, and holds `floats_per_col` coefficients per column at index(column, kk, part, row):
//     y += v X        : re += vr Xr - vi Xi,  im += vi Xr + vr Xi      (filter_bank, vqt.rs:889-895)
//     y += conj(w X)  : re += wr Xr - wi Xi,  im += -wi Xr - wr Xi     (negative_filter_bank, vqt.rs:896-910)
// with v, w the reference's coefficients times rho_c (the GEMM stages deliver X' = X / rho_c).
template <typename Index>
void build_band(const std::vector<WindowGroup>& groups, const std::vector<BlockGroup>& bg, const Columns& cols, int rb, int ku, int floats_per_col,
                Index index, std::vector<BandBlock>& band, std::vector<float>& B) {
    for (size_t g = 0; g < groups.size(); ++g) {
        const CsrMatrix& A = groups[g].filter_bank;
        const CsrMatrix& Bm = groups[g].negative_filter_bank;
        const std::vector<int>& idx = cols.idx_of[g];
        const auto& rho = cols.rho[g];
        const int xoff = bg[g].tile0 * CB_C;
        for (uint32_t r0 = 0; r0 < A.rows; r0 += (uint32_t)rb) {
            const uint32_t r1 = std::min<uint32_t>(A.rows, r0 + (uint32_t)rb);
            int lo = 1 << 30, hi = -1;
            for (uint32_t r = r0; r < r1; ++r) {
                for (uint32_t q = A.row_ptr[r]; q < A.row_ptr[r + 1]; ++q) {
                    lo = std::min(lo, idx[A.col_idx[q]]);
                    hi = std::max(hi, idx[A.col_idx[q]]);
                }
                if (Bm.nnz() > 0)
                    for (uint32_t q = Bm.row_ptr[r]; q < Bm.row_ptr[r + 1]; ++q) {
                        lo = std::min(lo, idx[Bm.col_idx[q]]);
                        hi = std::max(hi, idx[Bm.col_idx[q]]);
                    }
            }
            if (hi < 0) {   // rows without coefficients: one all-zero stage
                lo = 0;
                hi = 0;
            }
            BandBlock bb{};
            bb.bin0 = (int)(groups[g].first_bin + r0);
            bb.nrows = (int)(r1 - r0);
            bb.boff = (int)(B.size() / 64);
            bb.boff3 = (int)(B.size() / 128);   // (8-bin form; the 16-bin blocks get theirs with the bf16 planes)
            bb.x0 = xoff + lo;
            bb.kb = ((hi - lo + 1) + ku - 1) / ku * ku;
            const size_t first = B.size();
            B.resize(first + (size_t)bb.kb * floats_per_col, 0.0f);
            float* Bp = B.data() + first;
            for (uint32_t r = r0; r < r1; ++r) {
                const int row = (int)(r - r0);
                for (uint32_t q = A.row_ptr[r]; q < A.row_ptr[r + 1]; ++q) {
                    const int ci = idx[A.col_idx[q]];
                    const int cc = ci - lo;
                    // v * rho_c, in double, rounded once
                    const double ar_ = A.values[q].re, ai_ = A.values[q].im;
                    const float vr = (float)(ar_ * rho[ci].first - ai_ * rho[ci].second);
                    const float vi = (float)(ar_ * rho[ci].second + ai_ * rho[ci].first);
                    Bp[index(cc, 0, 0, row)] += vr;    // Re X -> re
                    Bp[index(cc, 1, 0, row)] += -vi;   // Im X -> re
                    Bp[index(cc, 0, 1, row)] += vi;    // Re X -> im
                    Bp[index(cc, 1, 1, row)] += vr;    // Im X -> im
                }
                if (Bm.nnz() > 0)
                    for (uint32_t q = Bm.row_ptr[r]; q < Bm.row_ptr[r + 1]; ++q) {
                        const int ci = idx[Bm.col_idx[q]];
                        const int cc = ci - lo;
                        const double br_ = Bm.values[q].re, bi_ = Bm.values[q].im;
                        const float wr = (float)(br_ * rho[ci].first - bi_ * rho[ci].second);
                        const float wi = (float)(br_ * rho[ci].second + bi_ * rho[ci].first);
                        Bp[index(cc, 0, 0, row)] += wr;
                        Bp[index(cc, 1, 0, row)] += -wi;
                        Bp[index(cc, 0, 1, row)] += -wi;
                        Bp[index(cc, 1, 1, row)] += -wr;
                    }
            }
            band.push_back(bb);
        }
    }
}

// blocks to waves: dealt round robin in bin order, so that the waves of a workgroup walk neighbouring blocks (whose column ranges
// overlap) at the same time and share the X columns through L1 / L2 (balancing by cost instead was measured no faster).
// Row w of the list: the count, then the blocks of wave w.
void deal_blocks(size_t n_blocks, int waves, int per_wave, int* rows) {
    for (int w = 0; w < waves; ++w) {
        int* row = rows + (size_t)w * per_wave;
        int n = 0;
        for (size_t i = (size_t)w; i < n_blocks; i += (size_t)waves) row[1 + n++] = (int)i;
        row[0] = n;
    }
}

}  // namespace

std::vector<MixedPair> plan_mixed_pairs(const std::vector<BlockGroup>& groups, size_t hop, bool general) {
    std::vector<MixedPair> pairs;
    if (general || groups.size() > 8) return pairs;   // (a tile list entry names a group in 3 bits: the fused path's limit)
    // a group's last tile is a candidate if it is partial and a single entry of the tile list whatever the wide mode: at most 16
    // columns (never paired up), or the odd tile of its group
    auto last_cols = [](const BlockGroup& G) { return G.n_cols - (G.n_tiles - 1) * CB_C; };
    auto candidate = [&](const BlockGroup& G) {
        const int n = last_cols(G);
        return G.n_tiles > 0 && G.nb == G.nb_f && n < CB_C && (n <= 16 || G.n_tiles % 2 == 1);
    };
    struct Cand { int a, b, dist, nb; };
    std::vector<Cand> cands;
    for (size_t i = 0; i < groups.size(); ++i)
        for (size_t k = i + 1; k < groups.size(); ++k) {
            const BlockGroup &A = groups[i], &B = groups[k];
            if (!candidate(A) || !candidate(B) || last_cols(A) + last_cols(B) > CB_C) continue;
            if ((A.s_rel - B.s_rel) % (long long)hop != 0) continue;
            cands.push_back(Cand{(int)i, (int)k, std::abs(A.levels - B.levels), std::max(A.nb, B.nb)});
        }
    std::stable_sort(cands.begin(), cands.end(), [](const Cand& x, const Cand& y) { return x.dist != y.dist ? x.dist < y.dist : x.nb > y.nb; });
    std::vector<char> used(groups.size(), 0);
    for (const Cand& c : cands) {
        if (used[c.a] || used[c.b] || (int)pairs.size() == MIXED_MAX_PAIRS) continue;
        used[c.a] = used[c.b] = 1;
        const bool a_first = groups[c.a].nb >= groups[c.b].nb;
        const int g1 = a_first ? c.a : c.b, g2 = a_first ? c.b : c.a;
        pairs.push_back(MixedPair{g1, g2, last_cols(groups[g1]), last_cols(groups[g2]), (int)((groups[g1].s_rel - groups[g2].s_rel) / (long long)hop)});
    }
    return pairs;
}

bool build_blockdft_tables(const HostPlan& plan, size_t hop, bool twiddle_fp16, BlockDftHostTables& t, std::string* err) {
    t = BlockDftHostTables();
    const auto& groups = plan.kernel.window_groups;
    const double pi = 3.14159265358979323846;
    Columns cols;
    cols.col_of.resize(groups.size());
    cols.idx_of.resize(groups.size());
    cols.rho.resize(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) {
        std::vector<char> used(groups[g].filter_bank.cols + 1, 0);
        for (uint32_t c : groups[g].filter_bank.col_idx) used[c] = 1;
        for (uint32_t c : groups[g].negative_filter_bank.col_idx) used[c] = 1;
        cols.idx_of[g].assign(used.size(), -1);
        for (uint32_t c = 0; c < used.size(); ++c)
            if (used[c]) {
                cols.idx_of[g][c] = (int)cols.col_of[g].size();
                cols.col_of[g].push_back(c);
            }
    }
    {
        bool divides = (hop & (hop - 1)) == 0;
        for (const WindowGroup& g : groups) divides = divides && g.window_size() % hop == 0;
        t.general = !divides;
    }
    int tile = 0, tw_off = 0, e16r_off = 0, gtw_off = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        BlockGroup B{};
        if (t.general) {   // window = nq whole hop blocks + rem samples; no tree
            B.nq = (int)(groups[g].window_size() / hop);
            B.rem = (int)(groups[g].window_size() % hop);
            B.nb = B.nb_f = 1;
            B.levels = B.levels_f = 0;
        } else {
            B.nb = (int)(groups[g].window_size() / hop);
            B.levels = 0;
            while ((1 << B.levels) < B.nb) ++B.levels;
            B.nb_f = std::min(B.nb, 64);
            B.levels_f = std::min(B.levels, 6);
        }
        B.n_cols = (int)cols.col_of[g].size();
        B.tile0 = tile;
        B.n_tiles = (B.n_cols + CB_C - 1) / CB_C;
        B.tw_off = tw_off;
        B.s_rel = (long long)groups[g].window_begin - (long long)plan.params.n_fft;  // + n_lead + hop at launch
        B.e16r_off = e16r_off;
        B.gtw_off = gtw_off;
        e16r_off += B.n_tiles * (B.rem / 2) * 16;
        gtw_off += 2 * B.n_tiles * CB_C;
        tile += B.n_tiles;
        tw_off += B.levels * B.n_tiles * CB_C;
        t.nb_max = std::max(t.nb_max, B.nb);
        t.groups.push_back(B);
    }
    if (tile * CB_C >= 0x8000) {
        if (err) *err = "unsupported: too many spectrum columns for the block-DFT path";
        return false;
    }
    t.n_tiles = tile;
    const int ntot = tile * GM_BN;
    auto tq = [&](double v) { const float f = (float)v; return twiddle_fp16 ? round_to_half(f) : f; };   // config 4: fp16 twiddles
    // The hop DFT is taken about the centre of the hop block (see blockdft_gemm_tree): E[m][c] = e^{-i th_c u_m},
    // u_m = m - (hop-1)/2, th_c = 2 pi c / W.  Every GEMM form therefore yields P' = P / rho_c, rho_c = e^{-i th_c (hop-1)/2},
    // and the tree X' = X / rho_c; rho_c goes into the kernel-product coefficients below.
    //   E [hop][Ntot], (cos, sin) interleaved per column; the mirrored fp32 form reads its first hop/2 rows
    t.E.assign((size_t)hop * ntot, 0.0f);
    t.tile_group.assign(tile, 0);
    t.tile_s.assign(tile, 0);
    t.comb_tw.assign((size_t)std::max(tw_off, 1), Float2{0.0f, 0.0f});
    for (size_t g = 0; g < groups.size(); ++g) {
        const BlockGroup& B = t.groups[g];
        const long long W2 = 2ll * (long long)groups[g].window_size();
        for (int tt = 0; tt < B.n_tiles; ++tt) {
            t.tile_group[B.tile0 + tt] = (int)g;
            t.tile_s[B.tile0 + tt] = B.s_rel;
        }
        cols.rho[g].resize(B.n_cols);
        for (int ci = 0; ci < B.n_cols; ++ci) {
            const long long c = (long long)cols.col_of[g][ci];  // actual spectrum column
            {   // the phase of the centred block DFT whose results the kernel product sees: the hop block's, or — a window shorter than a
                // general hop, where the transform is the remainder GEMM alone — the window's
                const long long D = t.general && B.nq == 0 ? (long long)B.rem : (long long)hop;
                const long long prod = (c * (D - 1)) % W2;
                const double ang = -2.0 * pi * (double)prod / (double)W2;
                cols.rho[g][ci] = {std::cos(ang), std::sin(ang)};
            }
            for (size_t m = 0; m < hop; ++m) {
                // reduce the angle exactly: c * (2m - hop + 1) mod 2W in integers
                long long prod = (c * (2ll * (long long)m - (long long)hop + 1ll)) % W2;
                if (prod < 0) prod += W2;
                const double ang = -2.0 * pi * (double)prod / (double)W2;
                const float er = tq(std::cos(ang)), ei = tq(std::sin(ang));
                t.E[m * ntot + (size_t)B.tile0 * GM_BN + 2 * ci] = er;
                t.E[m * ntot + (size_t)B.tile0 * GM_BN + 2 * ci + 1] = ei;
            }
            for (int l = 0; l < B.levels; ++l) {
                const long long prod = (c * (1ll << l)) % (long long)B.nb;
                const double ang = -2.0 * pi * (double)prod / (double)B.nb;
                t.comb_tw[B.tw_off + l * (B.n_tiles * CB_C) + ci] = Float2{tq(std::cos(ang)), tq(std::sin(ang))};
            }
        }
    }
    const int nb = (int)plan.params.range.n_buckets();
    t.n_bins_pad = (nb + 63) / 64 * 64;
    // 16-bin blocks (32 MFMA columns = 16 x (re, im)): B operand of column c, lane l (n = l & 31 = part * 16 + row, k = l >> 5)
    build_band(groups, t.groups, cols, BD_RB, BD_KU, 64, band16_index, t.band, t.band_B);
    t.band_B.resize(t.band_B.size() + (size_t)BD_NS * BD_KU * 64, 0.0f);   // the prefetch of the last block runs on past it
    // The same coefficients for the 16x16x4 MFMA form: blocks of BD8_RB = 8 bins (16 output columns = 8 x (re, im)) walk the
    // union of 8 rows' columns — about 35 instead of 57 columns per block, so 39 % fewer matrix operations for the same products.
    build_band(groups, t.groups, cols, BD8_RB, BD8_KU, 32, band8_index, t.band8, t.band_B4);
    t.band_B4.resize(t.band_B4.size() + (size_t)8 * 128, 0.0f);   // the prefetch of the last block runs on past it
    t.band_per_wave8 = (int)t.band8.size() + 2;
    t.band_list8.assign((size_t)8 * t.band_per_wave8, 0);
    deal_blocks(t.band8.size(), 8, t.band_per_wave8, t.band_list8.data());
    // ... and as one stage stream per wave (BandStage): a wave's blocks end to end, so the kernel's operand ring never restarts
    {
        const BandStage null_stage{t.n_tiles * CB_C, (int)(t.band_B4.size() / 128) - 8, 0, 0};   // zeroed X columns x zero coefficients
        int longest = 0;
        for (int w = 0; w < 8; ++w) {
            const int* row = t.band_list8.data() + (size_t)w * t.band_per_wave8;
            int n = 0;
            for (int i = 0; i < row[0]; ++i) n += t.band8[row[1 + i]].kb / BD8_KU;
            t.band_stage_count8[w] = (n + BD8_NS - 1) / BD8_NS * BD8_NS;
            longest = std::max(longest, t.band_stage_count8[w]);
        }
        t.band_stage_stride8 = longest + 2 * BD8_NS;
        t.band_stages8.assign((size_t)8 * t.band_stage_stride8, null_stage);
        for (int w = 0; w < 8; ++w) {
            const int* row = t.band_list8.data() + (size_t)w * t.band_per_wave8;
            BandStage* st = t.band_stages8.data() + (size_t)w * t.band_stage_stride8;
            for (int i = 0; i < row[0]; ++i) {
                const BandBlock& bb = t.band8[row[1 + i]];
                const int ns = bb.kb / BD8_KU;
                for (int s = 0; s < ns; ++s) *st++ = BandStage{bb.x0 + BD8_KU * s, bb.boff3 + s, 0, 0};
                st[-1].bin0 = bb.bin0;
                st[-1].fin = bb.nrows | BAND_STAGE_LAST;
            }
        }
    }
    // split-bf16 planes of the 16-bin coefficients, 8 columns (16 real k) per MFMA: lane (n = l & 31, kh = l >> 5)
    // holds k = 8 kh + t, t = 0..7  <->  column 4 kh + t / 2, Re / Im row t & 1
    for (BandBlock& bb : t.band) {
        bb.kg = (bb.kb + 7) / 8;
        bb.boff3 = (int)(t.band_B3.size() / (3 * 64 * 8));
        t.band_B3.resize(t.band_B3.size() + (size_t)bb.kg * 3 * 64 * 8, 0);
        const float* Bp = t.band_B.data() + (size_t)bb.boff * 64;
        for (int g = 0; g < bb.kg; ++g)
            for (int l = 0; l < 64; ++l)
                for (int tt = 0; tt < 8; ++tt) {
                    const int col = 8 * g + 4 * (l >> 5) + (tt >> 1);
                    const float x = col < bb.kb ? Bp[band16_lane_index(col, (tt & 1) * 32 + (l & 31))] : 0.0f;
                    const size_t base = ((size_t)(bb.boff3 + g) * 3) * 64 * 8 + (size_t)l * 8 + tt;
                    split_bf16x3(x, t.band_B3[base], t.band_B3[base + 64 * 8], t.band_B3[base + 2 * 64 * 8]);
                }
    }
    t.band_B3.resize(t.band_B3.size() + (size_t)B3_NS * 3 * 64 * 8, 0);
    // two sets of lists: for band_waves waves per workgroup (fp32 forms: 4 waves per SIMD when two workgroups fit a CU) and for 4
    // (split-bf16 form, whose register budget does not fit four waves per SIMD)
    t.band_waves = 8;
    t.band_per_wave = (int)t.band.size() + 2;
    t.band_list.assign((size_t)(t.band_waves + 4) * t.band_per_wave, 0);
    deal_blocks(t.band.size(), t.band_waves, t.band_per_wave, t.band_list.data());
    deal_blocks(t.band.size(), 4, t.band_per_wave, t.band_list.data() + (size_t)t.band_waves * t.band_per_wave);
    {   // E in the B-operand order of the 16x16x4 GEMM: [column tile][k < hop / 2][n < 16]: (cos c_n, cos c_{n+16}, -sin c_n, -sin c_{n+16})
        const size_t K2 = hop / 2;
        t.E16.resize((size_t)tile * K2 * 16);
        for (int tt = 0; tt < tile; ++tt)
            for (size_t m = 0; m < K2; ++m)
                for (int n = 0; n < 16; ++n) {
                    const float* e = t.E.data() + m * ntot + (size_t)tt * GM_BN;
                    t.E16[((size_t)tt * K2 + m) * 16 + n] = Float4{e[2 * n], e[2 * (n + 16)], e[2 * n + 1], e[2 * (n + 16) + 1]};
                }
    }
    {   // mixed tiles: per pair one merged slice, g1's last column tile and then g2's, columns taken from E as E16 takes them
        const size_t K2 = hop / 2;
        t.mixed = plan_mixed_pairs(t.groups, hop, t.general);
        t.E16M.assign(t.mixed.size() * K2 * 16, Float4{0.0f, 0.0f, 0.0f, 0.0f});
        for (size_t p = 0; p < t.mixed.size(); ++p) {
            const MixedPair& mp = t.mixed[p];
            for (int c = 0; c < mp.n1 + mp.n2; ++c) {
                const BlockGroup& B = t.groups[c < mp.n1 ? mp.g1 : mp.g2];
                const size_t col = ((size_t)(B.tile0 + B.n_tiles - 1) * CB_C + (c < mp.n1 ? c : c - mp.n1)) * 2;   // float index of the column's cosine in a row of E
                for (size_t m = 0; m < K2; ++m) {
                    Float4& dst = t.E16M[(p * K2 + m) * 16 + (c & 15)];
                    const float er = t.E[m * ntot + col], ei = t.E[m * ntot + col + 1];
                    if (c < 16) { dst.x = er; dst.z = ei; } else { dst.y = er; dst.w = ei; }
                }
            }
        }
    }
    t.E16R.assign((size_t)std::max(e16r_off, 1), Float4{0.0f, 0.0f, 0.0f, 0.0f});
    t.gen_tw.assign((size_t)std::max(gtw_off, 1), Float2{1.0f, 0.0f});
    if (t.general) {
        for (size_t g = 0; g < groups.size(); ++g) {
            const BlockGroup& B = t.groups[g];
            const long long W = (long long)groups[g].window_size(), W2 = 2 * W;
            auto cs = [&](long long num, long long den) {   // e^{-2 pi i num / den}, the angle reduced exactly
                long long r = num % den;
                if (r < 0) r += den;
                const double ang = -2.0 * pi * (double)r / (double)den;
                return Float2{tq(std::cos(ang)), tq(std::sin(ang))};
            };
            for (int ci = 0; ci < B.n_cols; ++ci) {
                const long long c = (long long)cols.col_of[g][ci];
                const int tt = ci / CB_C, n32 = ci % CB_C;
                // E_R[m][c] = e^{-i th_c (m - (rem - 1) / 2)}, m < rem / 2 (the mirrored form reads the first half), B-operand order of E16
                for (int m = 0; m < B.rem / 2; ++m) {
                    const Float2 e = cs(c * (2ll * m - (long long)B.rem + 1ll), W2);
                    Float4& dst = t.E16R[(size_t)B.e16r_off + ((size_t)tt * (B.rem / 2) + m) * 16 + (n32 & 15)];
                    if (n32 < 16) { dst.x = e.x; dst.z = e.y; } else { dst.y = e.x; dst.w = e.y; }
                }
                // phi_c = e^{-2 pi i c hop / W};  tau_c = phi_c^nq rho_R / rho_Q = e^{-i th_c (nq hop + (rem - hop) / 2)}
                t.gen_tw[(size_t)B.gtw_off + ci] = cs(c * (long long)hop, W);
                t.gen_tw[(size_t)B.gtw_off + B.n_tiles * CB_C + ci] = B.nq > 0 ? cs(c * (2ll * B.nq * (long long)hop + (long long)B.rem - (long long)hop), W2) : Float2{1.0f, 0.0f};
            }
        }
    }
    return true;
}

std::vector<uint16_t> build_Et_bf16x3(const std::vector<float>& E, int ntot, size_t hop) {
    std::vector<uint16_t> Et((size_t)3 * ntot * hop);
    for (int n = 0; n < ntot; ++n)
        for (size_t m = 0; m < hop; ++m)
            split_bf16x3(E[m * ntot + n], Et[((size_t)0 * ntot + n) * hop + m], Et[((size_t)1 * ntot + n) * hop + m], Et[((size_t)2 * ntot + n) * hop + m]);
    return Et;
}

// ------------------------------------------------------------------------------------------------
// streams -> runs -> launches
// ------------------------------------------------------------------------------------------------
std::vector<std::vector<BdRun>> pack_runs(const BdStream* st, size_t n_st, size_t chunk) {
    std::vector<std::vector<BdRun>> launches;
    const size_t budget = (chunk + 63) / 64;   // tiles per launch
    size_t used = 0;
    for (size_t i = 0; i < n_st; ++i) {
        size_t fbeg = 0, left = st[i].n_frames;
        while (left > 0) {
            const size_t nf = std::min(left, chunk);
            const size_t tiles = (nf + 63) / 64;
            if (launches.empty() || used + tiles > budget || launches.back().size() >= 0xFFFFu) {   // (a tile-list entry names its run in 16 bits)
                launches.emplace_back();
                used = 0;
            }
            launches.back().push_back(BdRun{i, fbeg, nf});
            used += tiles;
            fbeg += nf;
            left -= nf;
        }
    }
    return launches;
}

LaunchShape launch_shape(const BdStream* st, const std::vector<BdRun>& runs, size_t hop, size_t n_fft, int nb_max) {
    LaunchShape sh;
    sh.segs.resize(runs.size());
    const BdSlot* seen = nullptr;
    for (size_t u = 0; u < runs.size(); ++u) {
        const BdRun& r = runs[u];
        const BdStream& S = st[r.stream];
        // rebase the run's stream so that every byte offset of the launch fits 32 bits
        const long long n_samples = (long long)S.n_samples;
        const long long first_needed = (long long)S.first_end + (long long)r.fbeg * (long long)hop - (long long)n_fft;
        const long long rebase = std::max<long long>(0, std::min<long long>(first_needed, n_samples));
        const long long extent = std::min<long long>(n_samples - rebase, (long long)(r.nf + 2) * (long long)hop + (long long)n_fft + 4096);
        SegKey& k = sh.segs[u];
        k.pcm_off = S.pcm_off + rebase;
        k.pcm_bytes = (unsigned)std::min<long long>(extent * 4, 0xFFFFF000ll);
        k.base = (long long)S.first_end + (long long)r.fbeg * (long long)hop - rebase;
        k.nf = (int)r.nf;
        k.x_tile0 = (int)sh.x_tiles;
        k.y_tile0 = (int)sh.y_tiles;
        k.out_row0 = (long long)(S.out_row0 + r.fbeg * S.row_step);
        k.row_step = (int)S.row_step;
        k.slot_hash = S.slots ? (S.slot_hash | 1ull) : 0ull;
        k.grid_i = (long long)S.grid_i;
        k.fbeg = (long long)r.fbeg;
        sh.strided |= S.row_step != 1 || S.slots != nullptr;
        sh.x_tiles += (r.nf + 63) / 64;
        sh.y_tiles += (r.nf + (size_t)std::max(nb_max - 64, 0) + 63) / 64;
        sh.n_frames += r.nf;
        if (S.slots && S.slots != seen) {
            seen = S.slots;
            sh.slot_data.push_back(S.n_slots);
            for (size_t i = 0; i < S.n_slots; ++i) {
                sh.slot_data.push_back(S.slots[i].vframe0);
                sh.slot_data.push_back(S.slots[i].n_frames);
                sh.slot_data.push_back(S.slots[i].out_row0);
            }
        }
    }
    return sh;
}

void build_segment_map(const BdStream* st, const std::vector<BdRun>& runs, const LaunchShape& shape, std::vector<SegDev>& hsegs, std::vector<XTile>& hmap) {
    const std::vector<SegKey>& segs = shape.segs;
    hsegs.assign(segs.size(), SegDev{});
    hmap.assign(shape.x_tiles, XTile{});
    for (size_t u = 0; u < segs.size(); ++u) {
        hsegs[u] = SegDev{segs[u].pcm_off, segs[u].base, segs[u].pcm_bytes, segs[u].nf, segs[u].x_tile0, segs[u].y_tile0};
        const int tiles = (segs[u].nf + 63) / 64;
        const BdStream& S = st[runs[u].stream];
        for (int i = 0; i < tiles; ++i) {
            XTile xt{segs[u].out_row0 + 64ll * i * segs[u].row_step, std::min(64, segs[u].nf - 64 * i) | (segs[u].row_step << 8), segs[u].y_tile0 + i};
            if (S.slots) {   // frame t of the run = frame grid_i + row_step * t of the staged buffer: the slot it falls into names its rows
                const size_t rs = S.row_step, t0 = runs[u].fbeg + 64 * (size_t)i, v0 = S.grid_i + rs * t0;
                const BdSlot* lo = S.slots;   // the last slot that starts at or before v0 (slots ascend; they start on multiples of 64 row_step frames)
                size_t n = S.n_slots;
                while (n > 1) {
                    const size_t h = n / 2;
                    if (lo[h].vframe0 <= v0) { lo += h; n -= h; } else n = h;
                }
                long long live = 0;
                if (S.n_slots && lo->vframe0 <= v0 && v0 < lo->vframe0 + lo->n_frames)
                    live = std::min<long long>((long long)((lo->vframe0 + lo->n_frames - v0 + rs - 1) / rs), std::min(64, segs[u].nf - 64 * i));
                xt.out_row0 = S.n_slots ? (long long)(lo->out_row0 + (v0 - std::min(v0, lo->vframe0))) : 0;
                xt.live_step = (int)live | ((int)rs << 8);
            }
            hmap[segs[u].x_tile0 + i] = xt;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// tile lists of the fused kernels
// ------------------------------------------------------------------------------------------------
double fused_tile_count(const std::vector<BlockGroup>& groups, const std::vector<SegKey>& segs, int bm, bool split_bf16,
                        const std::vector<MixedPair>* mixed) {
    double n = 0.0;
    for (const SegKey& k : segs)
        for (size_t g = 0; g < groups.size(); ++g) {
            const BlockGroup& G = groups[g];
            const int S = bm - G.nb_f + 1;
            const int rows_g = k.nf + G.nb - G.nb_f;
            // a last tile of at most 16 columns runs half the MFMAs (fp32 kernel; the few tiles at the stream's ends run the full
            // loop: counted as half all the same)
            const bool half_last = !split_bf16 && G.n_cols - (G.n_tiles - 1) * CB_C <= 16;
            double last = half_last ? 0.5 : 1.0;
            // mixed tiles: g1's last tile carries g2's (a whole tile, or half of one up to 16 columns together); g2's last tile issues
            // nothing of its own (its few cover entries at the streams' ends are not counted)
            if (mixed && !split_bf16)
                for (const MixedPair& mp : *mixed) {
                    if (mp.g1 == (int)g) last = mp.n1 + mp.n2 <= 16 ? 0.5 : 1.0;
                    if (mp.g2 == (int)g) last = 0.0;
                }
            n += (G.n_tiles - 1 + last) * ((rows_g + S - 1) / S);
        }
    return n;
}

// Whether every sample a tile's K loop reads lies inside its stream's readable bytes: then the kernel takes 16-byte loads without
// range checks, and only such tiles may pair up into wide entries.  This MIRRORS the device-side test — `inside` in
// blockdft_gemm_tree / _tree_bf16x3 (tile_lo >= 0 && tile_hi * 4 <= pcm_bytes over bm rows of hop samples) and in
// blockdft_gemm_gen (bm - 1 whole hops + the tile kind's depth) — and must change with it: an entry marked wide here whose tile the
// kernel would range-check reads past the stream's end.
bool tile_inside_stream(const BlockGroup& G, const SegKey& seg, int f0, size_t hop, int bm, int kind) {
    if (kind == 0) {
        const long long tile_lo = seg.base + G.s_rel + (long long)f0 * (long long)hop, tile_hi = tile_lo + (long long)bm * (long long)hop;
        return tile_lo >= 0 && tile_hi * 4ll <= (long long)seg.pcm_bytes;
    }
    const long long depth = kind == 1 ? G.rem : (long long)hop;
    const long long tile_lo = seg.base + G.s_rel + (long long)(f0 + (kind == 1 ? G.nq : 0)) * (long long)hop;
    const long long tile_hi = tile_lo + (long long)(bm - 1) * (long long)hop + depth;
    return tile_lo >= 0 && tile_hi * 4ll <= (long long)seg.pcm_bytes;
}

// Frame-stripe tile order: the launch's frames are cut into stripes of opt.fs, stripe s belongs to XCD queue s & 7 (workgroup b
// runs on the XCD of all b' = b mod 8), and a queue takes its stripes in order, within a stripe every group's row tiles with
// all their column tiles.  All window groups then read a stripe's PCM rows from that XCD's L2 while they are resident (once
// per stripe, not once per group).  Entry: (group | wide << 8 | segment << 16, column tile, first frame, position i * 8 + queue).
// wide_mode 0: narrow tiles only; 1: wide tiles, the last opt.tail entries of every queue narrow; 2: wide tiles to the very end.
HostTileList build_tile_list(const std::vector<BlockGroup>& groups, const std::vector<SegKey>& segs, size_t hop, int bm, int wide_mode, int kind,
                             const TileListOptions& opt) {
    auto grp = [](const Int4& e) { return e.x & 255; };
    auto is_wide = [](const Int4& e) { return ((e.x >> 8) & 1) != 0; };
    auto seg_of = [](const Int4& e) { return (int)((unsigned)e.x >> 16); };
    auto inside = [&](const Int4& e) { return tile_inside_stream(groups[grp(e)], segs[seg_of(e)], e.z, hop, bm, kind); };
    auto is_mixed = [](const Int4& e) { return (e.x & TILE_MIXED) != 0; };
    auto pair_of = [&](const Int4& e) -> const MixedPair& { return opt.mixed[(e.x >> TILE_MIXED_PAIR_SHIFT) & 7]; };
    auto half_tile = [&](const Int4& e) {   // a group's last tile of at most 16 columns (a mixed tile: both parts together): half the K loop
        if (is_mixed(e)) return pair_of(e).n1 + pair_of(e).n2 <= 16;
        const BlockGroup& G = groups[grp(e)];
        return e.y == G.n_tiles - 1 && G.n_cols - e.y * CB_C <= 16;
    };
    // mixed tiles (kind 0): the pair a group is the first / the second member of
    std::vector<int> as_g1(groups.size(), -1), as_g2(groups.size(), -1);
    if (kind == 0)
        for (size_t p = 0; p < opt.mixed.size(); ++p) {
            as_g1[opt.mixed[p].g1] = (int)p;
            as_g2[opt.mixed[p].g2] = (int)p;
        }
    std::vector<std::vector<Int4>> q(8);
    for (size_t u = 0; u < segs.size(); ++u)
        for (size_t g = 0; g < groups.size(); ++g) {
            const BlockGroup& G = groups[g];
            if ((kind == 1 && G.rem == 0) || (kind == 2 && G.nq == 0)) continue;
            const int S = kind == 0 ? bm - G.nb_f + 1 : kind == 1 ? bm : bm - (G.nq > 1 ? G.nq - 1 : 0);
            const int rows_g = kind == 0 ? segs[u].nf + G.nb - G.nb_f : segs[u].nf;
            const bool half_last = G.n_cols - (G.n_tiles - 1) * CB_C <= 16;
            auto stripe_of = [&](int f0) { return (segs[u].x_tile0 * 64 + f0) / opt.fs; };   // position in the launch's frame order
            if (as_g2[g] >= 0) {
                // The second member of a pair: its last column tile rides in g1's mixed entries, which lie on g1's row grid and exist
                // where g1's tile is inside the stream.  Row j < S1 of the mixed tile at f1 is this group's frame f1 + j + d; the frames
                // those leave uncovered (next to g1's range-checked edge tiles, before the offset at the segment's start, the last
                // frames) get ordinary entries of the last tile at the first uncovered frame (S frames each: they may overlap what a
                // mixed entry or another cover entry stores — the same bits).
                const MixedPair& mp = opt.mixed[as_g2[g]];
                const BlockGroup& G1 = groups[mp.g1];
                const int S1 = bm - G1.nb_f + 1, nf = segs[u].nf;
                auto cover = [&](int from, int to) {   // ordinary entries over the frames [from, to)
                    for (int f = from; f < to; f += S) {
                        const int s = stripe_of(f);
                        q[s & 7].push_back(Int4{(int)g | (int)((unsigned)u << 16), G.n_tiles - 1, f, s});
                    }
                };
                int done = 0;   // frames [0, done) are stored
                for (int f1 = 0; f1 < nf; f1 += S1) {
                    if (!tile_inside_stream(G1, segs[u], f1, hop, bm, kind)) continue;
                    const int lo = std::max(f1 + mp.d, 0), hi = std::min(f1 + mp.d + S1, nf);
                    if (lo >= hi) continue;
                    if (done < lo) cover(done, lo);
                    done = std::max(done, hi);
                }
                if (done < nf) cover(done, nf);
            }
            for (int f0 = 0; f0 < rows_g; f0 += S)
                for (int ntl = 0; ntl < G.n_tiles; ++ntl) {
                    if (ntl == G.n_tiles - 1 && as_g2[g] >= 0) continue;   // (above)
                    if (ntl == G.n_tiles - 1 && as_g1[g] >= 0 && tile_inside_stream(G, segs[u], f0, hop, bm, kind)) {
                        const MixedPair& mp = opt.mixed[as_g1[g]];
                        const int s = stripe_of(f0);
                        q[s & 7].push_back(Int4{(int)g | TILE_MIXED | (mp.g2 << TILE_MIXED_G2_SHIFT) | (as_g1[g] << TILE_MIXED_PAIR_SHIFT) | (int)((unsigned)u << 16), ntl, f0, s});
                        continue;
                    }
                    // two neighbouring column tiles as one WIDE entry (.x bit 8; fp32 kernel, 256-row tiles)
                    // (a last tile of at most 16 columns keeps its own entry and its half-depth loop: pairing it up too was measured
                    // at the same time for more MFMAs)
                    const bool pair = wide_mode && tile_inside_stream(G, segs[u], f0, hop, bm, kind) && ntl + 1 < G.n_tiles && !(half_last && ntl + 1 == G.n_tiles - 1);
                    const int stripe = (segs[u].x_tile0 * 64 + f0) / opt.fs;   // position in the launch's frame order
                    q[stripe & 7].push_back(Int4{(int)g | (pair ? 256 : 0) | (int)((unsigned)u << 16), ntl, f0, stripe});
                    if (pair) ++ntl;
                }
        }
    // what a tile costs its workgroup, roughly in us: K loop (half for a last tile of at most 16 columns) + tree levels
    auto tile_cost = [&](const Int4& e) {
        const BlockGroup& G = groups[grp(e)];
        const bool half = half_tile(e);
        if (kind != 0) {   // a general hop's tiles: the K loop's depth decides
            const int depth = kind == 1 ? G.rem : (int)hop;
            return (inside(e) ? (half ? 1 : 2) : 4) * (depth / 32) + 8 + (kind == 2 ? G.nq : 0);
        }
        if (!inside(e)) return 2 * 16 + G.levels_f;   // the range-checked loop: dword loads
        return ((half ? 8 : 16) + G.levels_f) * (is_wide(e) ? 2 : 1);
    };
    auto longer = [&](const Int4& x, const Int4& y) { return tile_cost(x) > tile_cost(y); };
    for (auto& v : q)   // by stripe, the wide tiles of a stripe before its narrow ones; (segment, group, row tile, column tile) order kept
        std::stable_sort(v.begin(), v.end(), [&](const Int4& x, const Int4& y) {
            if (x.w != y.w) return x.w < y.w;
            return is_wide(x) > is_wide(y);
        });
    // Even queues: stripes are dealt round robin, but the stream's first and last stripe carry extra tiles (the range-checked
    // ones at the ends, which do not pair up, and the long windows' partial-sum rows past the last frame) — queue 0 ran 28 us
    // longer than the rest of a 290 us launch.  The heaviest queue hands entries of its last stripe to the lightest until they
    // differ by less than a tile (those read their PCM rows through another XCD's L2: a few dozen tiles per launch).
    if (opt.balance) {
        long long cost[8];
        for (int x = 0; x < 8; ++x) {
            cost[x] = 0;
            for (const Int4& e : q[x]) cost[x] += tile_cost(e);
        }
        for (int it = 0; it < 4096; ++it) {
            int h = 0, l = 0;
            for (int x = 1; x < 8; ++x) {
                if (cost[x] > cost[h]) h = x;
                if (cost[x] < cost[l]) l = x;
            }
            if (q[h].empty()) break;
            Int4 e = q[h].back();
            const int c = tile_cost(e);
            if (cost[h] - cost[l] <= c) break;
            q[h].pop_back();
            if (!q[l].empty()) e.w = q[l].back().w;   // it joins the receiving queue's last stripe
            q[l].push_back(e);
            cost[h] -= c;
            cost[l] += c;
        }
    }
    size_t longest = 0;
    for (auto& v : q) {
        // the queue's last stripe: long tiles first, so that what is still running when the queues run dry is short
        if (!v.empty()) {
            const int last = v.back().w;
            auto first_of_last = std::find_if(v.begin(), v.end(), [&](const Int4& e) { return e.w == last; });
            std::stable_sort(first_of_last, v.end(), longer);
            if (wide_mode == 1) {
                // ... and the queue's last entries narrow again (two per workgroup slot of the XCD): what is still running when the
                // queues run dry sets the launch's tail
                const size_t lo = first_of_last - v.begin();
                std::vector<Int4> tail;
                while (v.size() > lo && tail.size() < (size_t)opt.tail) {
                    const Int4 e = v.back();
                    v.pop_back();
                    if (is_wide(e)) {
                        tail.push_back(Int4{e.x & ~256, e.y, e.z, e.w});
                        tail.push_back(Int4{e.x & ~256, e.y + 1, e.z, e.w});
                    } else
                        tail.push_back(e);
                }
                std::stable_sort(tail.begin(), tail.end(), longer);
                v.insert(v.end(), tail.begin(), tail.end());
            }
        }
        longest = std::max(longest, v.size());
    }
    HostTileList out;
    for (auto& v : q)
        for (const Int4& e : v) {
            const double et = is_wide(e) ? 2.0 : (half_tile(e) ? 0.5 : 1.0);   // (the few range-checked tiles run the full loop: counted as half all the same)
            out.eff_tiles += et;
            out.eff_flop += et * bm * (2 * CB_C) * ((kind == 1 ? (double)groups[grp(e)].rem : (double)hop) / 2) * 2.0;   // (mirrored fp32 form: half depth)
        }
    out.list.assign(8 * std::max<size_t>(longest, 1), Int4{0, 0, 0x3FFFFFFF, 0});   // padding entries: past every group's rows
    for (int x = 0; x < 8; ++x)
        for (size_t i = 0; i < q[x].size(); ++i) {
            out.list[i * 8 + x] = q[x][i];
            out.list[i * 8 + x].w = (int)(i * 8 + x);
        }
    return out;
}

}  // namespace pvq
