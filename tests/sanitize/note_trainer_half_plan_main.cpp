// note_trainer_half_plan_main.cpp — the host side of the note trainer's bf16 step (note_trainer_plan.cpp: nth_splits,
// note_trainer_half_plan, note_trainer_check_precision) behind a command line, for tests/test_note_trainer_half.py: built with
// -fsanitize=address,undefined and run once per question, so that an overrun in the planner aborts the run.
//
//   splits    <m> <n> <k> [...]                              one number per triple
//   plan      <n_bins> <t_frames> <mlp> <layers> <max_batch>   "key value" lines, then "shadow <src_at> <n> <k> <w_at> <wt_at>" per dense weight
//   precision <value>                                        "<status> <text>"
#include <cstdio>
#include <cstdlib>
#include <string>

#include "note_trainer_plan.hpp"

using namespace pvq;

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const std::string cmd = argv[1];
    auto num = [&](int i) { return static_cast<uint32_t>(std::strtoull(argv[i], nullptr, 10)); };
    if (cmd == "splits" && argc > 2 && (argc - 2) % 3 == 0) {
        for (int at = 2; at < argc; at += 3) std::printf("%u\n", nth_splits(num(at), num(at + 1), num(at + 2)));
        return 0;
    }
    if (cmd == "plan" && argc == 7) {
        NoteModelDims d;
        d.n_bins = num(2);
        d.t_frames = num(3);
        d.mlp = num(4);
        d.layers = num(5);
        d.L = d.t_frames * d.n_bins;
        d.o_conv = (d.L - NM_KW) / 2 + 1;
        d.o_pool = d.o_conv / 2;
        d.n_features = NM_CH * d.o_pool;
        const NoteTrainerLayout lay = note_trainer_layout(d);
        const NoteTrainerHalfPlan p = note_trainer_half_plan(lay, num(6));
        std::printf("n_params %zu\nshadow_total %zu\nf_pad %u\nmlp_pad %u\nb_pad %u\n", lay.n_params, p.shadow_total, p.f_pad, p.mlp_pad, p.b_pad);
        std::printf("feat_at %zu\nfeatt_at %zu\nh_at %zu\nht_at %zu\ndz_at %zu\ndzt_at %zu\nda_at %zu\ndat_at %zu\n", p.feat_at, p.featt_at, p.h_at, p.ht_at, p.dz_at,
                    p.dzt_at, p.da_at, p.dat_at);
        std::printf("h_stride %zu\nht_stride %zu\nws_total %zu\n", p.h_stride, p.ht_stride, p.ws_total);
        for (const NthShadow& s : p.shadow) std::printf("shadow %zu %u %u %zu %zu\n", s.src_at, s.n, s.k, s.w_at, s.wt_at);
        return 0;
    }
    if (cmd == "precision" && argc == 3) {
        std::string err;
        const pvq_status st = note_trainer_check_precision(std::atoi(argv[2]), err);
        std::printf("%d %s\n", static_cast<int>(st), err.c_str());
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of note_trainer_half_plan_main.cpp\n");
    return 1;
}
