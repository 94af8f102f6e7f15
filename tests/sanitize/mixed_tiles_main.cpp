// ASan / UBSan driver for the mixed column tiles of the fused GEMM's tile lists (blockdft_plan.hpp: MixedPair; built and run by
// tests/test_mixed_tiles_plan.py, CPU only).  Over the six test geometries at hop 256 (and hop 128 at 96 kHz) and the launch shapes
// tests/sanitize/host_main.cpp uses — one 20 011-frame stream in sub-batches, 64 short unequal streams, the same streams staged with
// slots — it checks, with mixing on:
//   1. every frame of every column tile of every group and segment is stored by at least one entry, and by exactly one outside the
//      overlap of the cover entries (ordinary entries of a second member's last tile, which may store again what a mixed entry or
//      another cover entry stores);
//   2. mixed entries occur only for pairs that meet the four conditions and where the tile lies inside the stream;
//   3. no stored frame is negative or beyond the group's rows;
//   4. eff_tiles / eff_flop equal a recount;
//   5. an interior row tile at 48 kHz / 252 bins has 11 entries (13 with mixing off) and the pairs are (32, 16) and (8, 4) blocks; at
//      288 bins 14 (16: its six groups give 1 + 3 + 4 + 3 + 3 + 2 entries today); at 22 050 Hz / 588 bins the 2- and 11-column tiles
//      share one half tile;
// and, with mixing off, 6. that the lists are the ones the planner gave before mixed tiles existed: their hashes are printed
// ("OFF <hash>", one line per list) and compared by the Python test with tests/golden/mixed_tiles_off_lists.txt, which was recorded
// from the planner of the commit before (this file compiled with -DMIXED_TILES_RECORD_ONLY against those sources).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "batch_plan.hpp"
#include "blockdft_plan.hpp"
#include "vqt_host.hpp"

using namespace pvq;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(2); } } while (0)

// ---- stream sets, as tests/sanitize/host_main.cpp builds them ----------------------------------------------------------------------
struct StreamTable {
    std::vector<const float*> pcm;
    std::vector<size_t> lead, n_frames;
    size_t stride = 0;
};
static StreamTable stream_table(const std::vector<size_t>& n_frames, const std::vector<size_t>& leads, size_t hop) {
    StreamTable t;
    t.n_frames = n_frames;
    uintptr_t at = 0x100000;
    for (size_t k = 0; k < n_frames.size(); ++k) {
        t.stride = std::max(t.stride, n_frames[k]);
        t.lead.push_back(leads[k % leads.size()]);
        t.pcm.push_back(reinterpret_cast<const float*>(at));
        at += (t.lead[k] + n_frames[k] * hop + 7) * sizeof(float);
    }
    return t;
}
struct StreamSet {
    StreamStaging plan;
    std::vector<BdStream> st;
    size_t chunk = 0;
};
static StreamSet stream_set(const StreamTable& t, size_t hop, size_t window_union, bool staged, size_t chunk) {
    StreamSet s;
    s.plan = plan_stream_staging(t.pcm.data(), t.lead.data(), t.n_frames.data(), (uint32_t)t.pcm.size(), t.stride, hop, 1, window_union, staged ? ~(size_t)0 : 0);
    std::vector<StreamRun> runs = s.plan.longs;
    if (staged) {
        CHECK(s.plan.longs.empty() && s.plan.buffers.size() == 1);
        append_staged_runs(runs, s.plan.buffers[0], reinterpret_cast<const float*>((uintptr_t)0x40), hop, 1);
        chunk = (s.plan.buffers[0].frames + 63) / 64 * 64;
    }
    const float* base = nullptr;
    s.st = rebase_runs(runs.data(), runs.size(), &base);
    s.chunk = chunk;
    return s;
}

static unsigned long long list_hash(const std::vector<Int4>& list) {   // FNV-1a over the entries' words
    unsigned long long h = 1469598103934665603ull;
    for (const Int4& e : list)
        for (int v : {e.x, e.y, e.z, e.w})
            for (int b = 0; b < 4; ++b) {
                h ^= (unsigned long long)(((unsigned)v >> (8 * b)) & 255u);
                h *= 1099511628211ull;
            }
    return h;
}

#ifndef MIXED_TILES_RECORD_ONLY
// the four conditions, from the groups alone
static bool may_pair(const BlockDftHostTables& t, size_t hop, const BlockGroup& A, const BlockGroup& B, int n1, int n2) {
    return !t.general && A.nb == A.nb_f && B.nb == B.nb_f && (A.s_rel - B.s_rel) % (long long)hop == 0 && n1 + n2 <= CB_C;
}

struct ListStats { int mixed = 0, cover = 0; };
static ListStats check_mixed_list(const BlockDftHostTables& t, const LaunchShape& sh, size_t hop, int bm, int wide_mode, const HostTileList& tl) {
    ListStats stats;
    CHECK(!tl.list.empty() && tl.list.size() % 8 == 0);
    auto last_cols = [](const BlockGroup& G) { return G.n_cols - (G.n_tiles - 1) * CB_C; };
    std::vector<int> second_of(t.groups.size(), -1);
    for (size_t p = 0; p < t.mixed.size(); ++p) second_of[t.mixed[p].g2] = (int)p;
    // stores[u][g][column tile][frame]: by any entry / by mixed entries / by cover entries
    struct Cnt { std::vector<int> all, mixed, cover; };
    std::vector<std::vector<std::vector<Cnt>>> cnt(sh.segs.size(), std::vector<std::vector<Cnt>>(t.groups.size()));
    for (size_t u = 0; u < sh.segs.size(); ++u)
        for (size_t g = 0; g < t.groups.size(); ++g) {
            const int rows = sh.segs[u].nf + t.groups[g].nb - t.groups[g].nb_f;
            cnt[u][g].assign(t.groups[g].n_tiles, Cnt{std::vector<int>(rows, 0), std::vector<int>(rows, 0), std::vector<int>(rows, 0)});
        }
    double eff = 0.0, flop = 0.0;
    for (size_t i = 0; i < tl.list.size(); ++i) {
        const Int4& e = tl.list[i];
        if (e.z == 0x3FFFFFFF) {
            CHECK(e.x == 0 && e.y == 0);
            continue;
        }
        CHECK(e.w == (int)i);
        const size_t u = (unsigned)e.x >> 16, g = e.x & 255;
        const bool wide = (e.x >> 8) & 1, mixed = (e.x & TILE_MIXED) != 0;
        CHECK(u < sh.segs.size() && g < t.groups.size());
        const BlockGroup& G = t.groups[g];
        const int S = bm - G.nb_f + 1, rows = sh.segs[u].nf + G.nb - G.nb_f;
        CHECK(e.z >= 0 && e.z < rows && e.y >= 0 && e.y + (wide ? 1 : 0) < G.n_tiles);   // 3. (what the kernel stores is clipped to the rows below, as the kernel clips it)
        double et;
        if (mixed) {
            ++stats.mixed;
            const int p = (e.x >> TILE_MIXED_PAIR_SHIFT) & 7, g2 = (e.x >> TILE_MIXED_G2_SHIFT) & 7;
            CHECK(!wide && bm == 256 && (size_t)p < t.mixed.size());
            const MixedPair& mp = t.mixed[p];
            const BlockGroup& G2 = t.groups[mp.g2];
            // 2. the pair's conditions, the tile on g1's row grid and inside the stream
            CHECK(mp.g1 == (int)g && mp.g2 == g2 && mp.g1 != mp.g2 && G.nb >= G2.nb && mp.n1 == last_cols(G) && mp.n2 == last_cols(G2));
            CHECK(may_pair(t, hop, G, G2, mp.n1, mp.n2) && (long long)mp.d * (long long)hop == G.s_rel - G2.s_rel);
            CHECK(e.y == G.n_tiles - 1 && e.z % S == 0 && tile_inside_stream(G, sh.segs[u], e.z, hop, bm, 0));
            for (int j = 0; j < S; ++j) {   // the kernel's store predicates (fused_tree_store_mixed)
                const int f1 = e.z + j, f2 = e.z + j + mp.d;
                if (f1 < rows) {
                    ++cnt[u][g][e.y].all[f1];
                    ++cnt[u][g][e.y].mixed[f1];
                }
                if (f2 >= 0 && f2 < sh.segs[u].nf) {
                    ++cnt[u][mp.g2][G2.n_tiles - 1].all[f2];
                    ++cnt[u][mp.g2][G2.n_tiles - 1].mixed[f2];
                }
            }
            et = mp.n1 + mp.n2 <= 16 ? 0.5 : 1.0;
        } else {
            CHECK((e.x & 0xFE00) == 0);
            const bool is_cover = second_of[g] >= 0 && e.y == G.n_tiles - 1;
            stats.cover += is_cover;
            if (!is_cover) CHECK(e.z % S == 0);
            for (int ct = e.y; ct <= e.y + (wide ? 1 : 0); ++ct)
                for (int f = e.z; f < std::min(e.z + S, rows); ++f) {
                    ++cnt[u][g][ct].all[f];
                    if (is_cover) ++cnt[u][g][ct].cover[f];
                }
            if (wide) {
                const bool half_last = last_cols(G) <= 16;
                CHECK(wide_mode != 0 && tile_inside_stream(G, sh.segs[u], e.z, hop, bm, 0) && !(half_last && e.y + 1 == G.n_tiles - 1));
            }
            et = wide ? 2.0 : (e.y == G.n_tiles - 1 && last_cols(G) <= 16) ? 0.5 : 1.0;
        }
        eff += et;
        flop += et * bm * (2 * CB_C) * ((double)hop / 2) * 2.0;
    }
    // 1. coverage
    for (size_t u = 0; u < sh.segs.size(); ++u)
        for (size_t g = 0; g < t.groups.size(); ++g)
            for (int ct = 0; ct < t.groups[g].n_tiles; ++ct) {
                const Cnt& c = cnt[u][g][ct];
                const bool second_last = second_of[g] >= 0 && ct == t.groups[g].n_tiles - 1;
                for (size_t f = 0; f < c.all.size(); ++f) {
                    CHECK(c.all[f] >= 1 && c.mixed[f] <= 1);
                    if (c.all[f] > 1) CHECK(second_last && c.cover[f] >= 1);   // only where a cover entry overlaps
                    if (!second_last) CHECK(c.cover[f] == 0);
                }
            }
    CHECK(eff == tl.eff_tiles && flop == tl.eff_flop);   // 4.
    return stats;
}

// entries of the row tiles at k = 1 of every group's own grid (group g: f0 = S_g), mixed entries counted with their first group
static int row_tile_entries(const BlockDftHostTables& t, const HostTileList& tl, int bm) {
    int n = 0;
    for (const Int4& e : tl.list) {
        if (e.z == 0x3FFFFFFF) continue;
        const BlockGroup& G = t.groups[e.x & 255];
        n += e.z == bm - G.nb_f + 1;
    }
    return n;
}
#endif

int main() {
    struct Geom { float sr; float f0; unsigned oct, bpo; float q; } geoms[] = {
        {22050.0f, 55.0f, 7, 84, 1.6f}, {48000.0f, 55.0f, 7, 36, 1.6f}, {48000.0f, 55.0f, 8, 36, 1.6f},
        {96000.0f, 27.5f, 10, 36, 1.6f}, {96000.0f, 27.5f, 10, 84, 1.6f}, {22050.0f, 55.0f, 5, 36, 1.8f}};
    int lists_with_mixed = 0;
    for (const Geom& g : geoms) {
        VqtParameters p;
        p.sr = g.sr; p.range.min_freq = g.f0; p.range.octaves = g.oct; p.range.buckets_per_octave = g.bpo; p.quality = g.q;
        HostPlan plan;
        CHECK(build_plan(p, plan).kind == VqtError::None);
        const uint32_t n_bins = p.range.n_buckets();
        std::vector<size_t> hops = {256};
        if (g.sr > 90000.0f) hops.push_back(128);
        for (size_t hop : hops) {
            if (!blockdft_plan_applicable(plan, hop)) continue;
            BlockDftHostTables t;
            std::string err;
            CHECK(build_blockdft_tables(plan, hop, false, t, &err));
            if (t.general) continue;
#ifndef MIXED_TILES_RECORD_ONLY
            // the pairs: disjoint, within the conditions, their merged slices the two last tiles' columns of E16 side by side
            CHECK(t.mixed.size() <= (size_t)MIXED_MAX_PAIRS && t.E16M.size() == t.mixed.size() * (hop / 2) * 16);
            std::vector<int> member(t.groups.size(), 0);
            for (size_t pi = 0; pi < t.mixed.size(); ++pi) {
                const MixedPair& mp = t.mixed[pi];
                CHECK(mp.g1 >= 0 && mp.g2 >= 0 && (size_t)mp.g1 < t.groups.size() && (size_t)mp.g2 < t.groups.size() && mp.g1 < 8 && mp.g2 < 8);
                CHECK(++member[mp.g1] == 1 && ++member[mp.g2] == 1);
                const BlockGroup &A = t.groups[mp.g1], &B = t.groups[mp.g2];
                CHECK(may_pair(t, hop, A, B, mp.n1, mp.n2) && mp.n1 > 0 && mp.n2 > 0);
                for (size_t m = 0; m < hop / 2; ++m)
                    for (int c = 0; c < CB_C; ++c) {
                        const Float4& q = t.E16M[(pi * (hop / 2) + m) * 16 + (c & 15)];
                        const float re = c < 16 ? q.x : q.y, im = c < 16 ? q.z : q.w;
                        float wr = 0.0f, wi = 0.0f;
                        if (c < mp.n1 + mp.n2) {
                            const BlockGroup& S = c < mp.n1 ? A : B;
                            const int cs = c < mp.n1 ? c : c - mp.n1;
                            const Float4& s = t.E16[((size_t)(S.tile0 + S.n_tiles - 1) * (hop / 2) + m) * 16 + (cs & 15)];
                            wr = cs < 16 ? s.x : s.y;
                            wi = cs < 16 ? s.z : s.w;
                        }
                        CHECK(re == wr && im == wi);
                    }
            }
            if (n_bins == 252 && hop == 256) {   // 5.
                CHECK(t.mixed.size() == 2);
                CHECK(t.groups[t.mixed[0].g1].nb == 32 && t.groups[t.mixed[0].g2].nb == 16 && t.groups[t.mixed[1].g1].nb == 8 && t.groups[t.mixed[1].g2].nb == 4);
                CHECK(t.mixed[0].n1 + t.mixed[0].n2 == 30 && t.mixed[1].n1 + t.mixed[1].n2 == 29);
            }
            if (n_bins == 588 && hop == 256) {
                bool found = false;
                for (const MixedPair& mp : t.mixed) found = found || ((mp.n1 == 2 && mp.n2 == 11) || (mp.n1 == 11 && mp.n2 == 2));
                CHECK(found);
            }
            if (g.sr > 90000.0f && hop == 128)   // no pair may form with the groups that leave Y partial sums
                for (const MixedPair& mp : t.mixed) CHECK(t.groups[mp.g1].nb <= 64 && t.groups[mp.g2].nb <= 64);
#endif
            std::vector<size_t> shorts(64);
            for (size_t k = 0; k < shorts.size(); ++k) shorts[k] = 1 + (k * 37) % 300 + (k % 7 == 0 ? 700 : 0);
            const StreamTable one = stream_table({20011}, {plan.window_union}, hop), many = stream_table(shorts, {plan.window_union}, hop);
            const StreamSet sets[] = {stream_set(one, hop, plan.window_union, false, 8192), stream_set(many, hop, plan.window_union, false, 1 << 17),
                                      stream_set(many, hop, plan.window_union, true, 0)};
            for (size_t si = 0; si < 3; ++si) {
                const StreamSet& set = sets[si];
                const auto launches = pack_runs(set.st.data(), set.st.size(), set.chunk);
                for (size_t li = 0; li < launches.size(); ++li) {
                    const LaunchShape sh = launch_shape(set.st.data(), launches[li], hop, plan.params.n_fft, t.nb_max);
                    for (int wide : {0, 1, 2})
                        for (int balance = 0; balance < 2; ++balance) {
                            TileListOptions opt;
                            opt.balance = balance;
                            const HostTileList off = build_tile_list(t.groups, sh.segs, hop, 256, wide, 0, opt);
                            std::printf("OFF %u %zu %zu %zu %d %d %016llx %.1f\n", n_bins, hop, si, li, wide, balance, list_hash(off.list), off.eff_tiles);   // 6.
#ifndef MIXED_TILES_RECORD_ONLY
                            for (const Int4& e : off.list) CHECK((e.x & 0xFE00) == 0);
                            opt.mixed = t.mixed;
                            const HostTileList on = build_tile_list(t.groups, sh.segs, hop, 256, wide, 0, opt);
                            const ListStats st = check_mixed_list(t, sh, hop, 256, wide, on);
                            lists_with_mixed += st.mixed > 0;
                            if (t.mixed.empty()) CHECK(list_hash(on.list) == list_hash(off.list));
                            // 5. an interior row tile of the long stream's middle sub-batch (every group's tile at k = 1 lies inside the stream; wide tiles to the very end: no entries split for the tail)
                            if (si == 0 && li == 1 && wide == 2 && hop == 256 && (n_bins == 252 || n_bins == 288)) {
                                CHECK(row_tile_entries(t, off, 256) == (n_bins == 252 ? 13 : 16));
                                CHECK(row_tile_entries(t, on, 256) == (n_bins == 252 ? 11 : 14));
                            }
#endif
                        }
                }
            }
        }
    }
#ifndef MIXED_TILES_RECORD_ONLY
    CHECK(lists_with_mixed > 0);
#endif
    std::puts("MIXED_TILES_OK");
    return 0;
}
