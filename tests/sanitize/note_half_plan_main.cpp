// note_half_plan_main.cpp — the host planning of the note model's 16-bit path and of every precision's workspace
// (note_model_plan.cpp: note_model_pack_b16, note_model_workspace) behind a command line, for tests/test_note_model_half.py: built with -fsanitize=address,undefined and
// run once per question, in the pattern of note_plan_main.cpp.  Element i of a matrix is fill16(i), exact in bf16 and in f16 and
// never zero, which the test restates.
//
//   pack16 <n> <k> <conv_order 0|1> <o_pool> <precision 1|2> <file>   note_model_pack_b16 of W [n][k] -> file (raw 16-bit words)
//   ws <n_bins> <t_frames> <mlp> <layers> <limit> <stride> [n_frames ...]
//        note_model_tiles of the call, note_model_workspace for them in the 16-bit layout under <limit> bytes: one line
//        "tiles N tab B tile B chunk_tiles N feat_at B h0_at B h1_at B total B kf_pad K mlp_pad K", then one line "t0 nt" per chunk
//   wsp <precision 0|1|2> <n_bins> <t_frames> <mlp> <layers> <limit> <stride> [n_frames ...]      the same for the precision named
//   cap <precision 0|1|2> <n_bins> <t_frames> <mlp> <layers> <n_tiles>
//        chunk_tiles of note_model_workspace for <n_tiles> tiles under no limit: planning only, nothing of that size is made
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "note_model_plan.hpp"

using namespace pvq;

static NoteModelDims dims_of(uint32_t n_bins, uint32_t t_frames, uint32_t mlp, uint32_t layers) {
    NoteModelDims d;
    d.n_bins = n_bins;
    d.t_frames = t_frames;
    d.mlp = mlp;
    d.layers = layers;
    d.L = d.t_frames * d.n_bins;
    d.o_conv = (d.L - NM_KW) / 2 + 1;
    d.o_pool = d.o_conv / 2;
    d.n_features = NM_CH * d.o_pool;
    return d;
}

// (i % 255 + 1) * 2^((i / 255) % 16 - 8): eight significant bits, 2^-8 .. 255 * 2^7
static float fill16(size_t i) { return std::ldexp(static_cast<float>(i % 255u + 1u), static_cast<int>((i / 255u) % 16u) - 8); }

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const std::string cmd = argv[1];
    auto num = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
    if (cmd == "pack16" && argc == 8) {
        const uint32_t n = static_cast<uint32_t>(num(2)), k = static_cast<uint32_t>(num(3)), o_pool = static_cast<uint32_t>(num(5));
        std::vector<float> W(static_cast<size_t>(n) * k);
        for (size_t i = 0; i < W.size(); ++i) W[i] = fill16(i);
        const std::vector<uint16_t> packed = note_model_pack_b16(W.data(), n, k, num(4) != 0, o_pool, static_cast<pvq_note_precision>(num(6)));
        FILE* f = std::fopen(argv[7], "wb");
        if (!f) return 2;
        const size_t wrote = std::fwrite(packed.data(), sizeof(uint16_t), packed.size(), f);
        return (std::fclose(f) == 0 && wrote == packed.size()) ? 0 : 2;
    }
    auto u32 = [&](int i) { return static_cast<uint32_t>(num(i)); };
    const int o = cmd == "wsp" || cmd == "cap" ? 1 : 0;   // the arguments behind a leading <precision>
    const pvq_note_precision precision = o && argc > 2 ? static_cast<pvq_note_precision>(num(2)) : PVQ_NOTE_BF16;
    if ((cmd == "ws" || cmd == "wsp") && argc >= 8 + o) {
        const NoteModelDims d = dims_of(u32(2 + o), u32(3 + o), u32(4 + o), u32(5 + o));
        std::vector<size_t> nf;
        for (int i = 8 + o; i < argc; ++i) nf.push_back(num(i));
        const std::vector<NmTile> tiles = note_model_tiles(d, nf.data(), static_cast<uint32_t>(nf.size()), num(7 + o));
        const NmWorkspace w = note_model_workspace(d, precision, tiles.size(), num(6 + o));
        std::printf("tiles %zu tab %zu tile %zu chunk_tiles %zu feat_at %zu h0_at %zu h1_at %zu total %zu kf_pad %u mlp_pad %u\n", tiles.size(), w.tab_bytes,
                    w.tile_bytes, w.chunk_tiles, w.feat_at, w.h_at[0], w.h_at[1], w.total, w.kf_pad, w.mlp_pad);
        for (size_t t0 = 0; t0 < tiles.size(); t0 += w.chunk_tiles) std::printf("%zu %zu\n", t0, std::min(w.chunk_tiles, tiles.size() - t0));
        return 0;
    }
    if (cmd == "cap" && argc == 8) {
        const NmWorkspace w = note_model_workspace(dims_of(u32(3), u32(4), u32(5), u32(6)), precision, num(7), ~0ull);
        std::printf("%zu\n", w.chunk_tiles);
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of note_half_plan_main.cpp\n");
    return 1;
}
