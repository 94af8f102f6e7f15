// ASan / UBSan driver for the host side of libpvq (test infrastructure; built and run by tests/test_sanitize_cpu.py, CPU only — GPU
// AddressSanitizer is not available on this pool).  Replays, through the instrumented objects, what tests/test_host_plan.py,
// tests/test_analysis_state.py, tests/test_consumers.py and tests/test_multi_device.py feed them: kernel construction for every test
// geometry (including the two constructor errors and a reference panic), the AnalysisState recurrence in three smoothing modes, the
// peak helpers on crafted frames, the AGC / dataset / LED / .npy consumers, the shard planner, the block-DFT path's planner
// (tables, run packing, tile lists, segment tables and X-tile maps: structural invariants over every test geometry and launch shape)
// and the batch planner above it (route, interleaved runs, staging of short streams), whose stream sets feed the former.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "analysis_host.hpp"
#include "batch_plan.hpp"
#include "blockdft_plan.hpp"
#include "consumers_host.hpp"
#include "multi_host.hpp"
#include "vqt_host.hpp"

using namespace pvq;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float frand() {   // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (float)((rng_state * 2685821657736338717ull) >> 40) / 16777216.0f;
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(2); } } while (0)

// ---- stream sets (batch_plan.cpp) ------------------------------------------------------------------------------------------------
// A stream table as pvq_vqt_*_streams gets it.  The addresses are made up, each stream a region of its own: the planners measure
// distances between them and never read through them.
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
// One set of streams as Vqt::batch_streams_device / run_batch hand them to the block-DFT path, built by the planner they use:
// `r` interleaved runs per stream (hop H = r * hop), or the r runs over ONE staged buffer.
struct StreamSet {
    StreamStaging plan;
    std::vector<BdStream> st;      // the runs rebased on the lowest stream pointer, as launch_blockdft_streams hands them on
    size_t rows_total = 0, chunk = 0;
};
static StreamSet stream_set(const StreamTable& t, size_t r, size_t hop, size_t window_union, bool staged, size_t chunk) {
    StreamSet s;
    s.plan = plan_stream_staging(t.pcm.data(), t.lead.data(), t.n_frames.data(), (uint32_t)t.pcm.size(), t.stride, hop, r, window_union, staged ? ~(size_t)0 : 0);
    std::vector<StreamRun> runs = s.plan.longs;
    if (staged) {
        CHECK(s.plan.longs.empty() && s.plan.buffers.size() == 1);
        append_staged_runs(runs, s.plan.buffers[0], reinterpret_cast<const float*>((uintptr_t)0x40), hop, r);
        CHECK(runs.size() == r);
        chunk = (s.plan.buffers[0].frames + 63) / 64 * 64;
    } else
        CHECK(s.plan.buffers.empty());
    const float* base = nullptr;
    s.st = rebase_runs(runs.data(), runs.size(), &base);
    for (size_t i = 0; i < runs.size(); ++i) CHECK(base <= runs[i].pcm && s.st[i].pcm_off >= 0 && s.st[i].n_frames == runs[i].n_frames && s.st[i].slots == runs[i].slots);
    s.rows_total = t.stride * t.pcm.size();
    s.chunk = chunk;
    return s;
}

// the runs of one stream: its frames once each, run i the frames i, i + r, ... on the rows row0 + i + r t
static void check_interleaved_runs(const StreamRun* runs, size_t n_runs, const float* pcm, size_t lead, size_t n_frames, size_t hop, size_t r, size_t row0) {
    CHECK(n_runs == std::min(r, n_frames));
    std::vector<int> seen(n_frames, 0);
    for (size_t i = 0; i < n_runs; ++i) {
        const StreamRun& S = runs[i];
        CHECK(S.pcm == pcm && S.row_step == r && S.out_row0 == row0 + i && S.n_samples == lead + n_frames * hop && S.slots == nullptr && S.n_frames > 0);
        for (size_t t = 0; t < S.n_frames; ++t) {
            const size_t end = S.first_end + t * hop * r;   // (the run's hop is r * hop)
            CHECK(end > lead && (end - lead) % hop == 0);
            const size_t f = (end - lead) / hop - 1;
            CHECK(f < n_frames && f == i + r * t && S.out_row0 + t * S.row_step == row0 + f);
            ++seen[f];
        }
    }
    for (int c : seen) CHECK(c == 1);
}

// plan_stream_staging over one stream table: every stream once, slots on whole tiles with their history gap, pieces that tile the buffer
static std::vector<uint64_t> check_staging(const StreamTable& t, size_t hop, size_t r, size_t window_union, size_t stage_max) {
    const StreamStaging plan = plan_stream_staging(t.pcm.data(), t.lead.data(), t.n_frames.data(), (uint32_t)t.pcm.size(), t.stride, hop, r, window_union, stage_max);
    const size_t G = staging_history_frames(window_union, hop), A = 64 * r;
    const size_t cap = std::min<size_t>(147456, ((size_t)512 << 20) / (hop * sizeof(float)));
    CHECK(G * hop + hop >= window_union && (G == 0 || (G - 1) * hop + hop < window_union));
    std::vector<int> seen(t.pcm.size(), 0);
    size_t at = 0;
    while (at < plan.longs.size()) {   // a long stream: its runs side by side
        CHECK(t.stride > 0);
        const size_t s = plan.longs[at].out_row0 / t.stride;
        CHECK(s < t.pcm.size() && t.n_frames[s] > 0);
        const size_t n_runs = std::min(r, t.n_frames[s]);
        CHECK(at + n_runs <= plan.longs.size());
        check_interleaved_runs(&plan.longs[at], n_runs, t.pcm[s], t.lead[s], t.n_frames[s], hop, r, s * t.stride);
        ++seen[s];
        at += n_runs;
    }
    std::vector<uint64_t> hashes;
    for (const StagedBuffer& b : plan.buffers) {
        CHECK(!b.slots.empty() && b.pieces.size() == b.slots.size() && (b.slots.size() == 1 || b.frames <= cap));
        size_t prev_end = 0;       // frames: the end of the slot before
        long long written = 0;     // samples: everything before is a stream's data or zeroed
        long long longest = 0;
        for (size_t i = 0; i < b.slots.size(); ++i) {
            const BdSlot& sl = b.slots[i];
            const StagePiece& pc = b.pieces[i];
            const size_t s = sl.out_row0 / t.stride;
            CHECK(s < t.pcm.size() && sl.out_row0 == s * t.stride && sl.n_frames == t.n_frames[s] && sl.n_frames > 0 && sl.n_frames <= stage_max);
            ++seen[s];
            CHECK(sl.vframe0 % A == 0 && sl.vframe0 >= prev_end + G);
            prev_end = sl.vframe0 + sl.n_frames;
            // the piece: the stream's frames from the slot's first sample on, before them what of its lead the gap holds
            const long long h = (long long)(sl.vframe0 * hop) - pc.dst_off;
            CHECK(h >= 0 && (size_t)h <= t.lead[s] && (size_t)h <= G * hop && pc.src == t.pcm[s] + (t.lead[s] - (size_t)h));
            CHECK(pc.count == h + (long long)(sl.n_frames * hop) && pc.src + pc.count == t.pcm[s] + t.lead[s] + sl.n_frames * hop);
            CHECK((size_t)h == std::min(t.lead[s], G * hop) || pc.dst_off == 0);   // (all the history a frame reads, unless the buffer begins there)
            CHECK(pc.zero_from == written && pc.dst_off >= pc.zero_from && pc.zero_to >= pc.dst_off + pc.count);
            CHECK(i + 1 == b.slots.size() ? pc.zero_to == (long long)(b.frames * hop) : pc.zero_to == pc.dst_off + pc.count);
            written = pc.zero_to;
            longest = std::max(longest, pc.count);
        }
        CHECK(written == (long long)(b.frames * hop) && b.frames % A == 0 && b.frames >= prev_end && longest == b.longest);
        std::vector<StreamRun> runs;
        append_staged_runs(runs, b, reinterpret_cast<const float*>((uintptr_t)0x40), hop, r);
        CHECK(runs.size() == r);
        size_t frames = 0;
        for (size_t i = 0; i < r; ++i) {
            CHECK(runs[i].grid_i == i && runs[i].row_step == r && runs[i].first_end == (i + 1) * hop && runs[i].n_samples == b.frames * hop);
            CHECK(runs[i].slots == b.slots.data() && runs[i].n_slots == b.slots.size() && runs[i].slot_hash == b.hash);
            frames += runs[i].n_frames;
        }
        CHECK(frames == b.frames);
        hashes.push_back(b.hash);
    }
    for (size_t s = 0; s < seen.size(); ++s) CHECK(seen[s] == (t.n_frames[s] > 0 ? 1 : 0));
    return hashes;
}

static void check_batch_plan(const HostPlan& plan, bool bench_geometry) {
    const size_t wu = plan.window_union;
    auto hop_factor = [&](size_t hop) -> size_t {   // Vqt::blockdft_hop_factor
        for (size_t r = 1; r <= 16; r *= 2)
            if (blockdft_plan_applicable(plan, hop * r)) return r;
        return 0;
    };
    // ---- route: one function for the run functions and for Vqt::resolve_algo; what it may answer, per setting
    const size_t counts[] = {1, 63, 64, 383, 384, 1700, 3500, 65536, (size_t)1 << 20};
    for (size_t hop : {(size_t)64, (size_t)256, (size_t)1024, (size_t)800, (size_t)1600, (size_t)320, (size_t)735}) {
        const size_t r = hop_factor(hop);
        const size_t thr = r ? auto_block_min_frames(plan, hop, r) : 0;
        CHECK(r == 0 || thr >= 64 * r);
        for (int takes = 0; takes < 2; ++takes) {
            if (r == 0 && takes) continue;
            bool block_before = false;
            for (size_t n : counts) {
                CHECK(route_batch(PVQ_ALGO_FFT, r, takes != 0, n, thr) == BatchRoute::Fft);
                const BatchRoute forced = route_batch(PVQ_ALGO_BLOCKDFT, r, takes != 0, n, thr), au = route_batch(PVQ_ALGO_AUTO, r, takes != 0, n, thr);
                CHECK(forced == (r == 0 ? BatchRoute::RefuseNoHop : takes ? BatchRoute::BlockStreams : r == 1 ? BatchRoute::BlockPerStream : BatchRoute::RefuseUnfusedHop));
                // AUTO never refuses; it takes the block-DFT path where the forced setting runs it, from the threshold on
                const bool runs_forced = forced == BatchRoute::BlockStreams || forced == BatchRoute::BlockPerStream;
                CHECK(au == (runs_forced && n >= thr ? forced : BatchRoute::Fft));
                CHECK(!block_before || au != BatchRoute::Fft);
                block_before = au != BatchRoute::Fft;
            }
        }
    }
    if (bench_geometry) {   // tests/test_handles_gpu.py: test_resolve_algo_is_a_pure_query (general hops: the fused kernels take streams)
        CHECK(hop_factor(800) == 2 && hop_factor(735) == 0 && hop_factor(320) != 0);
        CHECK(route_batch(PVQ_ALGO_AUTO, 2, true, 100000, auto_block_min_frames(plan, 800, 2)) == BatchRoute::BlockStreams);
        CHECK(route_batch(PVQ_ALGO_AUTO, 2, true, 64, auto_block_min_frames(plan, 800, 2)) == BatchRoute::Fft);
        CHECK(route_batch(PVQ_ALGO_AUTO, hop_factor(320), true, 100000, auto_block_min_frames(plan, 320, hop_factor(320))) == BatchRoute::BlockStreams);
        CHECK(route_batch(PVQ_ALGO_AUTO, 0, false, 100000, 0) == BatchRoute::Fft);
    }
    // ---- runs and staging
    const struct { size_t hop, r; } hops[] = {{64, 1}, {256, 1}, {1024, 1}, {800, 2}, {1600, 1}};
    const size_t stage_max = 2048;
    const std::vector<size_t> leads = {0, 777, wu, 3 * wu + 5};
    std::vector<size_t> many(80);
    for (size_t k = 0; k < many.size(); ++k) many[k] = stage_max - k % 3;   // more than one buffer's worth of frames
    const std::vector<std::vector<size_t>> sets = {{300}, {0, 17}, {5, 0, stage_max, stage_max + 1, 63, 64, 65, 700, 1}, many, {0, 0}};
    for (const auto& hr : hops) {
        std::vector<uint64_t> hashes;
        for (const auto& n_frames : sets) {
            const StreamTable t = stream_table(n_frames, leads, hr.hop);
            const std::vector<uint64_t> h = check_staging(t, hr.hop, hr.r, wu, stage_max);
            size_t n_short = 0;
            for (size_t n : n_frames) n_short += n > 0 && n <= stage_max && n_frames.size() > 1;
            CHECK(h.empty() == (n_short < 2));   // (a single short stream goes as it is)
            if (n_frames.size() == many.size()) CHECK(h.size() >= 2);
            hashes.insert(hashes.end(), h.begin(), h.end());
            CHECK(check_staging(t, hr.hop, hr.r, wu, 0).empty());
        }
        for (size_t i = 0; i < hashes.size(); ++i)   // different slot layouts, different hashes
            for (size_t k = 0; k < i; ++k) CHECK(hashes[i] != hashes[k]);
    }
}

// ---- block-DFT planner (blockdft_plan.cpp) ---------------------------------------------------------------------------------------
static void check_tables(const BlockDftHostTables& t, size_t hop, uint32_t n_bins) {
    const size_t xcp = (size_t)t.n_tiles * CB_C + X_PAD_COLS, ntot = (size_t)t.n_tiles * GM_BN;
    CHECK(t.E.size() == hop * ntot && t.E16.size() == (size_t)t.n_tiles * (hop / 2) * 16);
    CHECK(t.tile_group.size() == (size_t)t.n_tiles && t.tile_s.size() == (size_t)t.n_tiles);
    int tiles = 0;
    for (const BlockGroup& G : t.groups) {
        CHECK(G.tile0 == tiles && G.n_tiles * CB_C >= G.n_cols && G.nb <= t.nb_max && G.nb_f <= 64 && (1 << G.levels_f) == G.nb_f);
        tiles += G.n_tiles;
        CHECK((size_t)G.tw_off + (size_t)G.levels * G.n_tiles * CB_C <= t.comb_tw.size());
        CHECK((size_t)G.e16r_off + (size_t)G.n_tiles * (G.rem / 2) * 16 <= t.E16R.size());
        CHECK((size_t)G.gtw_off + 2 * (size_t)G.n_tiles * CB_C <= t.gen_tw.size());
        if (t.general) CHECK((size_t)G.nq * hop + G.rem > 0 && G.nq <= GEN_MAX_NQ && G.nb == 1); else CHECK(G.nq == 0 && G.rem == 0 && (1 << G.levels) == G.nb);
    }
    CHECK(tiles == t.n_tiles);
    for (int g : t.tile_group) CHECK(g >= 0 && (size_t)g < t.groups.size());
    // kernel-product blocks: every bin once, in order; the columns a block walks (with the operand ring's prefetch past its range: the
    // stages in flight x columns per stage) lie inside a frame tile of X incl. its zeroed pad columns, its coefficients inside their arrays
    auto check_blocks = [&](const std::vector<BandBlock>& band, int rb, int ku, int ns) {
        int bin = 0;
        for (const BandBlock& b : band) {
            CHECK(b.bin0 == bin && b.nrows >= 1 && b.nrows <= rb && b.kb > 0 && b.kb % ku == 0 && b.x0 >= 0);
            bin += b.nrows;
            CHECK((size_t)b.x0 + b.kb + (size_t)ns * ku <= xcp);
        }
        CHECK(bin == (int)n_bins);
    };
    check_blocks(t.band, BD_RB, BD_KU, BD_NS);
    check_blocks(t.band8, BD8_RB, BD8_KU, BD8_NS);
    for (const BandBlock& b : t.band) {
        CHECK(((size_t)b.boff + b.kb + BD_NS * BD_KU) * 64 <= t.band_B.size());
        CHECK(b.kg * 8 >= b.kb && ((size_t)b.boff3 + b.kg + B3_NS) * 3 * 64 * 8 <= t.band_B3.size() && (size_t)b.x0 + 8 * (size_t)(b.kg + B3_NS) <= xcp);
    }
    for (const BandBlock& b : t.band8) CHECK(((size_t)b.boff3 + b.kb / 4 + 8) * 128 <= t.band_B4.size() && b.boff == 2 * b.boff3);
    // block lists: per set of waves, every block in exactly one wave's row
    auto check_lists = [&](const int* rows, int waves, int per_wave, size_t n_blocks) {
        std::vector<int> seen(n_blocks, 0);
        for (int w = 0; w < waves; ++w) {
            const int* row = rows + (size_t)w * per_wave;
            CHECK(row[0] >= 0 && row[0] < per_wave);
            for (int i = 0; i < row[0]; ++i) {
                CHECK(row[1 + i] >= 0 && (size_t)row[1 + i] < n_blocks);
                ++seen[row[1 + i]];
            }
        }
        for (int c : seen) CHECK(c == 1);
    };
    CHECK(t.band_list.size() == (size_t)(t.band_waves + 4) * t.band_per_wave && t.band_list8.size() == (size_t)8 * t.band_per_wave8);
    check_lists(t.band_list.data(), t.band_waves, t.band_per_wave, t.band.size());
    check_lists(t.band_list.data() + (size_t)t.band_waves * t.band_per_wave, 4, t.band_per_wave, t.band.size());
    check_lists(t.band_list8.data(), 8, t.band_per_wave8, t.band8.size());
}

// every (segment, group, row tile, column tile) the launch needs exactly once, wide entries only where the kernel may take them
static void check_tile_list(const BlockDftHostTables& t, const LaunchShape& sh, size_t hop, int bm, int wide_mode, int kind, const HostTileList& tl) {
    CHECK(!tl.list.empty() && tl.list.size() % 8 == 0);
    std::vector<std::vector<std::vector<int>>> seen(sh.segs.size(), std::vector<std::vector<int>>(t.groups.size()));
    auto stride_of = [&](const BlockGroup& G) { return kind == 0 ? bm - G.nb_f + 1 : kind == 1 ? bm : bm - (G.nq > 1 ? G.nq - 1 : 0); };
    auto skipped = [&](const BlockGroup& G) { return (kind == 1 && G.rem == 0) || (kind == 2 && G.nq == 0); };
    for (size_t u = 0; u < sh.segs.size(); ++u)
        for (size_t g = 0; g < t.groups.size(); ++g) {
            const BlockGroup& G = t.groups[g];
            const int rows = kind == 0 ? sh.segs[u].nf + G.nb - G.nb_f : sh.segs[u].nf, S = stride_of(G);
            CHECK(S > 0);
            seen[u][g].assign(skipped(G) ? 0 : (size_t)((rows + S - 1) / S) * G.n_tiles, 0);
        }
    double eff = 0.0;
    for (size_t i = 0; i < tl.list.size(); ++i) {
        const Int4& e = tl.list[i];
        if (e.z == 0x3FFFFFFF) {   // padding: past every group's rows
            CHECK(e.x == 0 && e.y == 0);
            continue;
        }
        CHECK(e.w == (int)i);
        const size_t u = (unsigned)e.x >> 16, g = e.x & 255;
        const bool wide = (e.x >> 8) & 1;
        CHECK(u < sh.segs.size() && g < t.groups.size() && (e.x & 0xFE00) == 0);
        const BlockGroup& G = t.groups[g];
        const int S = stride_of(G);
        CHECK(e.z >= 0 && e.z % S == 0 && e.y >= 0 && e.y + (wide ? 1 : 0) < G.n_tiles);
        const size_t slot = (size_t)(e.z / S) * G.n_tiles + e.y;
        CHECK(slot + (wide ? 1 : 0) < seen[u][g].size());
        ++seen[u][g][slot];
        if (wide) {
            ++seen[u][g][slot + 1];
            const bool half_last = G.n_cols - (G.n_tiles - 1) * CB_C <= 16;
            CHECK(wide_mode != 0 && tile_inside_stream(G, sh.segs[u], e.z, hop, bm, kind) && !(half_last && e.y + 1 == G.n_tiles - 1));
        }
        eff += wide ? 2.0 : (e.y == G.n_tiles - 1 && G.n_cols - e.y * CB_C <= 16) ? 0.5 : 1.0;
    }
    for (const auto& per_seg : seen)
        for (const auto& per_group : per_seg)
            for (int c : per_group) CHECK(c == 1);
    CHECK(eff == tl.eff_tiles && tl.eff_flop >= 0.0);
}

static void check_blockdft_plan(const HostPlan& plan) {
    const struct { size_t hop, r; } hops[] = {{64, 1}, {256, 1}, {1024, 1}, {800, 2}, {1600, 1}};
    const uint32_t n_bins = plan.params.range.n_buckets();
    for (const auto& hr : hops) {
        const size_t H = hr.hop * hr.r, r = hr.r;
        if (!blockdft_plan_applicable(plan, H)) continue;
        BlockDftHostTables t;
        std::string err;
        CHECK(build_blockdft_tables(plan, H, hr.hop == 256 && n_bins == 252, t, &err));
        check_tables(t, H, n_bins);
        if (!t.general && H % FB_BK == 0 && H <= 256) CHECK(build_Et_bf16x3(t.E, t.n_tiles * GM_BN, H).size() == 3 * t.E.size());
        std::vector<size_t> shorts(64);
        for (size_t k = 0; k < shorts.size(); ++k) shorts[k] = 1 + (k * 37) % 300 + (k % 7 == 0 ? 700 : 0);
        // one long stream in sub-batches (first / middle / last), 64 short unequal streams side by side, the same streams staged into one
        // buffer with slots; r = 2: every stream as two interleaved (strided) runs
        const StreamTable one = stream_table({20011}, {plan.window_union}, hr.hop), many = stream_table(shorts, {plan.window_union}, hr.hop);
        const StreamSet sets[] = {stream_set(one, r, hr.hop, plan.window_union, false, 8192), stream_set(many, r, hr.hop, plan.window_union, false, 1 << 17),
                                  stream_set(many, r, hr.hop, plan.window_union, true, 0)};
        for (const StreamSet& set : sets) {
            const auto launches = pack_runs(set.st.data(), set.st.size(), set.chunk);
            size_t frames = 0;
            for (const auto& runs : launches) {
                CHECK(!runs.empty() && runs.size() <= 0xFFFFu);
                const LaunchShape sh = launch_shape(set.st.data(), runs, H, plan.params.n_fft, t.nb_max);
                CHECK(sh.segs.size() == runs.size() && sh.x_tiles * 64 <= (set.chunk + 63) / 64 * 64 && sh.strided == (r != 1 || set.st[0].slots != nullptr));
                frames += sh.n_frames;
                std::vector<SegDev> segs;
                std::vector<XTile> xmap;
                build_segment_map(set.st.data(), runs, sh, segs, xmap);
                CHECK(segs.size() == runs.size() && xmap.size() == sh.x_tiles);
                for (const SegDev& s : segs)
                    CHECK(s.n_frames > 0 && s.x_tile0 >= 0 && (size_t)s.x_tile0 + (s.n_frames + 63) / 64 <= sh.x_tiles && s.y_tile0 >= 0 && (size_t)s.y_tile0 < sh.y_tiles && s.pcm_off >= 0);
                for (const XTile& x : xmap) {   // the rows a tile's live frames go to lie inside the output
                    const int live = x.live_step & 255, step = x.live_step >> 8;
                    CHECK(live <= 64 && step == (int)r && x.y_tile >= 0 && (size_t)x.y_tile < sh.y_tiles);
                    if (live > 0) CHECK(x.out_row0 >= 0 && (size_t)x.out_row0 + (size_t)(live - 1) * step < set.rows_total);
                }
                for (int bm : {128, 256})
                    for (int wide : {0, 1, 2})
                        for (int kind = t.general ? 1 : 0; kind <= (t.general ? 2 : 0); ++kind)
                            for (int balance = 0; balance < 2; ++balance) {
                                TileListOptions opt;
                                opt.balance = balance;
                                check_tile_list(t, sh, H, bm, wide, kind, build_tile_list(t.groups, sh.segs, H, bm, wide, kind, opt));
                            }
                (void)fused_tile_count(t.groups, sh.segs, 256, false);
            }
            size_t want = 0;
            for (const BdStream& s : set.st) want += s.n_frames;
            CHECK(frames == want);
        }
    }
}

int main() {
    // ---- kernel construction: the six test geometries ----------------------------------------------------------------------
    struct G { float sr; float f0; unsigned oct, bpo; float q; } geoms[] = {
        {22050.0f, 55.0f, 7, 84, 1.6f}, {48000.0f, 55.0f, 7, 36, 1.6f}, {48000.0f, 55.0f, 8, 36, 1.6f},
        {96000.0f, 27.5f, 10, 36, 1.6f}, {96000.0f, 27.5f, 10, 84, 1.6f}, {22050.0f, 55.0f, 5, 36, 1.8f}};
    size_t nnz_default = 0, neg_default = 0;
    for (const G& g : geoms) {
        VqtParameters p;
        p.sr = g.sr; p.range.min_freq = g.f0; p.range.octaves = g.oct; p.range.buckets_per_octave = g.bpo; p.quality = g.q;
        HostPlan plan;
        const VqtError e = build_plan(p, plan);
        CHECK(e.kind == VqtError::None);
        size_t nnz = 0, neg = 0, rows = 0;
        for (const WindowGroup& w : plan.kernel.window_groups) {
            nnz += w.filter_bank.nnz(); neg += w.negative_filter_bank.nnz(); rows += w.filter_bank.rows;
            CHECK(w.filter_bank.row_ptr.size() == w.filter_bank.rows + 1);
            for (uint32_t c : w.filter_bank.col_idx) CHECK(c < w.filter_bank.cols);
        }
        CHECK(rows == p.range.n_buckets());
        CHECK(plan.bandwidth_lo_hz.size() == rows);
        if (g.bpo == 84 && g.sr < 30000.0f) { nnz_default = nnz; neg_default = neg; }
        std::vector<float> lnf;
        bin_log_frequencies(p, lnf);
        CHECK(lnf.size() == rows);
        check_blockdft_plan(plan);
        check_batch_plan(plan, g.sr == 48000.0f && g.oct == 7);
    }
    CHECK(neg_default == 379);                       // VQT_REVIEW.md:369
    CHECK(nnz_default > 15000 && nnz_default < 20000);
    {   // constructor errors (vqt.rs:518-528, :567-573) and a reference panic turned exception
        VqtParameters p; p.sr = 96000.0f; p.range.octaves = 10; p.range.buckets_per_octave = 36;
        HostPlan plan;
        CHECK(build_plan(p, plan).kind == VqtError::AboveNyquist);
        VqtParameters q; q.quality = 40.0f;
        CHECK(build_plan(q, plan).kind == VqtError::WindowExceedsNFft);
        CHECK(!build_plan(q, plan).to_string().empty());
    }
    // ---- AnalysisState: three smoothing modes over noise + tones -------------------------------------------------------------
    for (int mode = 0; mode < 3; ++mode) {
        VqtRange r; r.buckets_per_octave = mode == 2 ? 36 : 84; r.octaves = mode == 2 ? 5 : 7;
        FullAnalysisParameters ap;
        AnalysisState st(r, ap);
        if (mode == 1) st.update_vqt_smoothing_duration(false, Duration{});
        const uint32_t n = r.n_buckets();
        std::vector<float> x(n);
        for (int f = 0; f < 120; ++f) {
            for (uint32_t k = 0; k < n; ++k) x[k] = 8.0f * frand();
            x[(37 + f) % n] = 45.0f; x[(200 + 3 * f) % n] = 38.0f; x[5] = 30.0f;
            if (f == 60) std::fill(x.begin(), x.end(), 0.0f);
            CHECK(st.preprocess(x.data(), n, Duration{(uint64_t)(f % 7 == 0 ? 1100 : 16) * 1000000ull}));
            CHECK(st.x_vqt_peakfiltered.size() == n && st.calmness.size() == n);
            for (const ContinuousPeak& c : st.peaks_continuous) CHECK(std::isfinite(c.center) && std::isfinite(c.size));
            (void)st.bin_to_frequency((uint32_t)f % n);
        }
        CHECK(!st.preprocess(x.data(), n - 1, Duration{16000000ull}));   // analysis.rs:289: wrong length
    }
    {   // peak helpers on crafted frames: plateaus, edges, empty
        VqtRange r; r.buckets_per_octave = 84;
        std::vector<float> x(r.n_buckets(), 0.0f);
        PeakDetectionParameters cfg{5.0f, 3.5f};
        CHECK(find_peaks(cfg, x.data(), (uint32_t)x.size(), 84).empty());
        x[0] = 50.0f; x[x.size() - 1] = 50.0f; x[100] = x[101] = x[102] = 20.0f; x[300] = 40.0f; x[302] = 39.0f;
        std::vector<uint32_t> pk = find_peaks(cfg, x.data(), (uint32_t)x.size(), 84);
        std::vector<ContinuousPeak> cp = enhance_peaks_continuous(pk, x.data(), r);
        promote_bass_peaks_with_harmonics(cp, x.data(), r, 28, 0.3f);
        CHECK(cp.size() == pk.size());
    }
    // ---- consumers -------------------------------------------------------------------------------------------------------------
    {
        std::string why;
        CHECK(MonoAgc::valid(0.07f, 0.0001f, &why));
        CHECK(!MonoAgc::valid(-1.0f, 0.5f, &why));
        MonoAgc agc(0.07f, 0.0001f);
        const size_t chunk = train_chunk_samples(0.0915, 22050.0f), n_chunks = 9;
        CHECK(chunk % 64 == 0 && chunk > 0);
        std::vector<float> L(n_chunks * chunk), R(n_chunks * chunk), mono(n_chunks * chunk), gains(n_chunks);
        for (size_t i = 0; i < L.size(); ++i) { L[i] = 0.3f * (frand() - 0.5f); R[i] = 0.3f * (frand() - 0.5f); }
        std::fill(L.begin() + 2 * chunk, L.begin() + 3 * chunk, 0.0f);   // a silent chunk: gain frozen
        std::fill(R.begin() + 2 * chunk, R.begin() + 3 * chunk, 0.0f);
        train_condition_stream(agc, L.data(), R.data(), n_chunks, chunk, mono.data(), gains.data());
        train_condition_stream(agc, L.data(), nullptr, n_chunks, chunk, mono.data(), gains.data());
        const uint32_t nb = 252, nf = 3;
        std::vector<float> db(nf * nb, 1.0f), rows(nf * (nb + 128));
        std::vector<uint32_t> vptr = {0, 2, 2, 3};
        std::vector<int32_t> vkey = {60, 64, 127};
        std::vector<float> gl = {0.9f, 0.2f, 1.0f}, gr = {0.9f, 0.4f, 1.0f}, ag = {1.0f, 1.0f, 1.0f};
        CHECK(train_rows(db.data(), nf, nb, vptr.data(), vkey.data(), gl.data(), gr.data(), ag.data(), rows.data(), &why));
        vkey[0] = 128;   // (frame 0's voices label frame 1's row)
        CHECK(!train_rows(db.data(), nf, nb, vptr.data(), vkey.data(), gl.data(), gr.data(), ag.data(), rows.data(), &why));
        const char* path = "/tmp/pvq_sanitize_rows.npy";
        CHECK(npy_write_f32(path, rows.data(), rows.size(), &why));
        std::remove(path);
        CHECK(!npy_write_f32("/nonexistent-dir/x.npy", rows.data(), 4, &why));
        float colors[12][3];
        for (int i = 0; i < 12; ++i) for (int c = 0; c < 3; ++c) colors[i][c] = frand();
        float rgb[3];
        for (float b = 0.0f; b < 72.0f; b += 0.37f) calculate_color(36, b, colors, 0.6f, 0.8f, rgb);
        const uint32_t n_b = 180;
        std::vector<float> ctr = {0.2f, 17.5f, 100.9f, 179.4f}, sz = {3.0f, 20.0f, 45.0f, 9.0f};
        std::vector<uint8_t> out(3 + 3 * n_b);
        CHECK(led_frame(n_b, 36, ctr.data(), sz.data(), 4, colors, 0.6f, 0.8f, out.data()) == out.size());
        CHECK(led_frame(n_b, 36, nullptr, nullptr, 0, colors, 0.6f, 0.8f, out.data()) == out.size());
    }
    // ---- shard planner -------------------------------------------------------------------------------------------------------------
    for (uint32_t world = 1; world <= 9; ++world) {
        uint64_t total = 0;
        for (uint32_t r = 0; r < world; ++r) {
            ShardPlan s;
            CHECK(plan_shard(1000003, 256, 16384, r, world, &s));
            CHECK(s.first_frame == total);
            total += s.n_frames;
        }
        CHECK(total == 1000003);
        ShardPlan s;
        CHECK(!plan_shard(10, 256, 16384, world, world, &s));
    }
    std::puts("SANITIZE_HOST_OK");
    return 0;
}
