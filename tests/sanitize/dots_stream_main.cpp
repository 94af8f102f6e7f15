// ASan / UBSan driver for the kernel product's per-wave stage streams (blockdft_plan.cpp: band_stages8; test infrastructure, built
// and run by tests/test_dots_stream_plan.py, CPU only).  Over the six test geometries and a 3-bin range, at their block-path hops:
// every block of band8 in exactly one wave's stream, in the order band_list8 deals them; a block's stages (x0 + 4 s, boff3 + s) with
// the flag, bin0 and nrows on the last one only; counts that are multiples of BD8_NS; every entry of a row — null stages, the ring's
// last BD8_NS - 1 fetches and the descriptor reads two rounds ahead included — inside a frame tile's columns and inside band_B4,
// null stages on zero coefficients and the zeroed pad columns.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "blockdft_plan.hpp"
#include "vqt_host.hpp"

using namespace pvq;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(2); } } while (0)

static int n_checked = 0;

static void check_streams(const HostPlan& plan, size_t hop) {
    CHECK(blockdft_plan_applicable(plan, hop));
    BlockDftHostTables t;
    std::string err;
    CHECK(build_blockdft_tables(plan, hop, false, t, &err));
    const int xcols = t.n_tiles * CB_C, xcp = xcols + X_PAD_COLS;
    const int b_groups = (int)(t.band_B4.size() / 128);
    CHECK(t.band_B4.size() % 128 == 0 && b_groups >= 8);
    const int stride = t.band_stage_stride8;
    CHECK(t.band_stages8.size() == (size_t)8 * stride);
    std::vector<int> seen(t.band8.size(), 0);
    int longest = 0;
    size_t real_stages = 0, walked = 0;
    for (const BandBlock& b : t.band8) real_stages += (size_t)b.kb / BD8_KU;
    for (int w = 0; w < 8; ++w) {
        const BandStage* st = t.band_stages8.data() + (size_t)w * stride;
        const int* row = t.band_list8.data() + (size_t)w * t.band_per_wave8;
        const int count = t.band_stage_count8[w];
        CHECK(count >= 0 && count % BD8_NS == 0);
        // the kernel reads descriptors up to two rounds past the one it multiplies, and fetches BD8_NS - 1 stages past the last
        CHECK(count + 2 * BD8_NS <= stride && count + BD8_NS - 1 <= stride);
        longest = count > longest ? count : longest;
        int at = 0;
        for (int i = 0; i < row[0]; ++i) {   // the wave's blocks in deal order
            const int bi = row[1 + i];
            CHECK(bi >= 0 && (size_t)bi < t.band8.size() && bi == w + 8 * i);
            ++seen[bi];
            const BandBlock& b = t.band8[bi];
            const int ns = b.kb / BD8_KU;
            CHECK(ns >= 1 && at + ns <= count);
            for (int s = 0; s < ns; ++s, ++at) {
                CHECK(st[at].x == b.x0 + BD8_KU * s && st[at].b == b.boff3 + s);
                if (s + 1 < ns)
                    CHECK(st[at].bin0 == 0 && st[at].fin == 0);
                else
                    CHECK(st[at].bin0 == b.bin0 && st[at].fin == (b.nrows | BAND_STAGE_LAST) && b.nrows >= 1 && b.nrows <= BD8_RB);
                CHECK(st[at].x + BD8_KU <= xcols);   // a real stage reads spectrum columns only
            }
        }
        walked += (size_t)at;
        CHECK(count - at < BD8_NS);   // padded to the next multiple, no further
        for (int i = at; i < stride; ++i) {   // null stages: zeroed pad columns x zero coefficients, no flag
            CHECK(st[i].x >= xcols && st[i].b >= b_groups - 8 && st[i].bin0 == 0 && st[i].fin == 0);
            for (size_t k = 0; k < 128; ++k) CHECK(t.band_B4[(size_t)st[i].b * 128 + k] == 0.0f);
        }
        for (int i = 0; i < stride; ++i) {   // every entry in bounds
            CHECK(st[i].x >= 0 && st[i].x + BD8_KU <= xcp);
            CHECK(st[i].b >= 0 && st[i].b < b_groups);
        }
    }
    for (int c : seen) CHECK(c == 1);
    CHECK(walked == real_stages && stride == longest + 2 * BD8_NS);
    ++n_checked;
}

int main() {
    struct G { float sr; float f0; unsigned oct, bpo; float q; size_t hop; } geoms[] = {
        {22050.0f, 55.0f, 7, 84, 1.6f, 256}, {48000.0f, 55.0f, 7, 36, 1.6f, 256}, {48000.0f, 55.0f, 8, 36, 1.6f, 256},
        {96000.0f, 27.5f, 10, 36, 1.6f, 128}, {96000.0f, 27.5f, 10, 84, 1.6f, 128}, {22050.0f, 55.0f, 5, 36, 1.8f, 256},
        {22050.0f, 440.0f, 3, 1, 1.6f, 64}};   // 3 bins (a window group each: at most three blocks): waves without any block
    for (const G& g : geoms) {
        VqtParameters p;
        p.sr = g.sr; p.range.min_freq = g.f0; p.range.octaves = g.oct; p.range.buckets_per_octave = g.bpo; p.quality = g.q; p.gamma = 4.8f * g.q;
        HostPlan plan;
        CHECK(build_plan(p, plan).kind == VqtError::None);
        check_streams(plan, g.hop);
        if (g.bpo == 1) {
            BlockDftHostTables t;
            std::string err;
            CHECK(build_blockdft_tables(plan, g.hop, false, t, &err) && t.band8.size() >= 1 && t.band8.size() <= 3);
            for (size_t w = 0; w < 8; ++w) CHECK((t.band_stage_count8[w] > 0) == (w < t.band8.size()));   // (check_streams: their rows hold null stages only)
        }
    }
    CHECK(n_checked == 7);
    std::printf("SANITIZE_DOTS_STREAM_OK\n");
    return 0;
}
