// note_plan_main.cpp — the host planners of the note model and its trainer (note_model_plan.cpp, note_trainer_plan.cpp) behind a
// command line, for tests/test_note_model.py and tests/test_note_trainer.py: built with -fsanitize=address,undefined and run once
// per question, so that an overrun in a planner aborts the run.  Matrices and weights are not read from files: element i of a
// matrix is fill(i), element i of tensor j of a state_dict fill(1000003 j + i), which the tests restate.
//
//   pack   <n> <k> <conv_order 0|1> <o_pool> <file>     note_model_pack_b of W [n][k] -> file (raw f32)
//   tiles  <t_frames> <stride> [n_frames ...]           note_model_tiles (no counts: every stream has stride; then <n_streams> follows stride as "x<N>")
//   layout <n_bins> <t_frames> <mlp> <layers> <file>    note_trainer_layout ("name at n" lines, then "n_params N") and note_trainer_arena -> file
//   splits <m> <n> <k> [<m> <n> <k> ...]                nt_splits, one number per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "note_model_plan.hpp"
#include "note_trainer_plan.hpp"

using namespace pvq;

static float fill(size_t i) { return static_cast<float>(i % 16777213u + 1u); }   // exact in f32, never zero

static int write_floats(const char* path, const std::vector<float>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return 2;
    const size_t n = std::fwrite(v.data(), sizeof(float), v.size(), f);
    return (std::fclose(f) == 0 && n == v.size()) ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const std::string cmd = argv[1];
    auto num = [&](int i) { return static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10)); };
    if (cmd == "pack" && argc == 7) {
        const uint32_t n = num(2), k = num(3), o_pool = num(5);
        std::vector<float> W(static_cast<size_t>(n) * k);
        for (size_t i = 0; i < W.size(); ++i) W[i] = fill(i);
        return write_floats(argv[6], note_model_pack_b(W.data(), n, k, num(4) != 0, o_pool));
    }
    if (cmd == "tiles" && argc >= 4) {
        NoteModelDims d;
        d.t_frames = num(2);
        const size_t stride = num(3);
        std::vector<size_t> nf;
        uint32_t n_streams = 0;
        if (argc == 5 && argv[4][0] == 'x') n_streams = static_cast<uint32_t>(std::strtoul(argv[4] + 1, nullptr, 10));
        else
            for (int i = 4; i < argc; ++i) nf.push_back(num(i));
        const std::vector<NmTile> tiles = note_model_tiles(d, nf.empty() ? nullptr : nf.data(), nf.empty() ? n_streams : static_cast<uint32_t>(nf.size()), stride);
        for (const NmTile& t : tiles) std::printf("%u %u %u %u\n", t.stream, t.f0, t.n_valid, t.pad);
        return 0;
    }
    if (cmd == "layout" && argc == 7) {
        pvq_note_model_params p{};
        p.n_bins = num(2);
        p.t_frames = num(3);
        p.mlp_size = num(4);
        p.mlp_layers = num(5);
        // sizes first (a placeholder stands for every weight pointer: note_model_check reads none), then the tensors
        float one = 0.0f;
        std::vector<float*> lw(8, &one), lb(8, &one);
        pvq_note_model_weights w{};
        w.conv_weight = w.conv_bias = w.fc1_weight = w.fc1_bias = w.output_weight = w.output_bias = &one;
        w.layer_weight = lw.data();
        w.layer_bias = lb.data();
        NoteModelDims d;
        std::string err;
        const pvq_status st = note_model_check(&p, &w, d, err);
        if (st != PVQ_OK) {
            std::printf("refused %d %s\n", static_cast<int>(st), err.c_str());
            return 0;
        }
        const NoteTrainerLayout lay = note_trainer_layout(d);
        std::vector<std::pair<std::string, NtTensor>> order = {{"conv1.weight", lay.conv_w}, {"conv1.bias", lay.conv_b}, {"fc1.weight", lay.fc1_w}, {"fc1.bias", lay.fc1_b}};
        for (uint32_t i = 0; i < d.layers; ++i) {
            order.push_back({"layers." + std::to_string(i) + ".weight", lay.layer_w[i]});
            order.push_back({"layers." + std::to_string(i) + ".bias", lay.layer_b[i]});
        }
        order.push_back({"output.weight", lay.out_w});
        order.push_back({"output.bias", lay.out_b});
        std::vector<std::vector<float>> data(order.size());
        for (size_t j = 0; j < order.size(); ++j) {
            data[j].resize(order[j].second.n);
            for (size_t i = 0; i < data[j].size(); ++i) data[j][i] = fill(1000003u * j + i);
            std::printf("%s %zu %zu\n", order[j].first.c_str(), order[j].second.at, order[j].second.n);
        }
        std::printf("n_params %zu\n", lay.n_params);
        w.conv_weight = data[0].data();
        w.conv_bias = data[1].data();
        w.fc1_weight = data[2].data();
        w.fc1_bias = data[3].data();
        for (uint32_t i = 0; i < d.layers; ++i) {
            lw[i] = data[4 + 2 * i].data();
            lb[i] = data[5 + 2 * i].data();
        }
        w.output_weight = data[4 + 2 * d.layers].data();
        w.output_bias = data[5 + 2 * d.layers].data();
        return write_floats(argv[6], note_trainer_arena(lay, w));
    }
    if (cmd == "splits" && argc >= 5 && (argc - 2) % 3 == 0) {
        for (int i = 2; i + 2 < argc; i += 3) std::printf("%u\n", nt_splits(num(i), num(i + 1), num(i + 2)));
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of note_plan_main.cpp\n");
    return 1;
}
