// note_test_plan_main.cpp — the host side of the note trainer's test pass (note_trainer_plan.cpp: note_trainer_test_plan,
// note_test_metrics) behind a command line, for tests/test_note_test.py: built with -fsanitize=address,undefined and run once per
// question, so that an overrun in the planner aborts the run.
//
//   plan    <n_idx> <max_batch> <batch>                       "chunk <begin> <rows>" per chunk, then "n_batches N", "rows_bytes N", "out_bytes N"
//   metrics <rows> <tp> <fp> <fn> <correct> <loss> [...]      one record per six numbers -> "mean_f1 accuracy mean_loss" (%.17g), or "refused <status> <text>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "note_trainer_plan.hpp"

using namespace pvq;

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const std::string cmd = argv[1];
    auto num = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
    if (cmd == "plan" && argc == 5) {
        const NoteTrainerTestPlan p = note_trainer_test_plan(static_cast<size_t>(num(2)), static_cast<uint32_t>(num(3)), static_cast<uint32_t>(num(4)));
        for (const NtTestChunk& c : p.chunks) std::printf("chunk %zu %u\n", c.begin, c.rows);
        std::printf("n_batches %zu\nrows_bytes %zu\nout_bytes %zu\n", p.n_batches, p.rows_bytes, p.out_bytes);
        return 0;
    }
    if (cmd == "metrics" && (argc - 2) % 6 == 0) {
        std::vector<pvq_note_test_batch> b((argc - 2) / 6);
        for (size_t k = 0; k < b.size(); ++k) {
            const int at = 2 + 6 * static_cast<int>(k);
            b[k].rows = static_cast<uint32_t>(num(at));
            b[k].tp = static_cast<uint32_t>(num(at + 1));
            b[k].fp = static_cast<uint32_t>(num(at + 2));
            b[k].fn = static_cast<uint32_t>(num(at + 3));
            b[k].correct = static_cast<uint32_t>(num(at + 4));
            b[k]._pad = 0;
            b[k].loss = std::strtod(argv[at + 5], nullptr);
        }
        double f1 = 0.0, acc = 0.0, loss = 0.0;
        std::string err;
        const pvq_status st = note_test_metrics(b.empty() ? nullptr : b.data(), b.size(), &f1, &acc, &loss, err);
        if (st != PVQ_OK) std::printf("refused %d %s\n", static_cast<int>(st), err.c_str());
        else std::printf("%.17g %.17g %.17g\n", f1, acc, loss);
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of note_test_plan_main.cpp\n");
    return 1;
}
