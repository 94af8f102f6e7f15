// note_epoch_plan_main.cpp — the host side of the note trainer's epochs (note_trainer_plan.cpp: note_trainer_epoch_plan,
// note_epoch_order over note_epoch_math.hpp, note_epoch_mean_loss) behind a command line, for tests/test_note_epoch.py: built with
// -fsanitize=address,undefined and run once per question, so that an overrun or a shift too far in the order aborts the run.
//
//   plan  <n_idx> <batch>                        "name value" per field of NoteTrainerEpochPlan
//   order <seed> <epoch> <n> <first> <count>     the order's values on one line, or "refused <status> <text>"
//   mean  <loss> [...]                           note_epoch_mean_loss of the values as floats (%.17g)
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
    if (cmd == "plan" && argc == 4) {
        const NoteTrainerEpochPlan p = note_trainer_epoch_plan(static_cast<size_t>(num(2)), static_cast<uint32_t>(num(3)));
        std::printf("n_batches %zu\nlast_rows %u\nidx_at %zu\norder_at %zu\nloss_at %zu\ndevice_bytes %zu\nh_idx_at %zu\nh_loss_at %zu\nhost_bytes %zu\n", p.n_batches,
                    p.last_rows, p.idx_at, p.order_at, p.loss_at, p.device_bytes, p.h_idx_at, p.h_loss_at, p.host_bytes);
        return 0;
    }
    if (cmd == "order" && argc == 7) {
        const uint64_t count = num(6);
        std::vector<uint32_t> out(count < (1u << 20) ? count : 0);   // exactly count values: one written beyond them is an overrun
        std::string err;
        const pvq_status st = note_epoch_order(num(2), num(3), num(4), num(5), count, out.empty() ? nullptr : out.data(), err);
        if (st != PVQ_OK) {
            std::printf("refused %d %s\n", static_cast<int>(st), err.c_str());
            return 0;
        }
        for (uint32_t v : out) std::printf("%u ", v);
        std::printf("\n");
        return 0;
    }
    if (cmd == "mean" && argc > 2) {
        std::vector<float> v;
        for (int i = 2; i < argc; ++i) v.push_back(std::strtof(argv[i], nullptr));
        std::printf("%.17g\n", note_epoch_mean_loss(v.data(), v.size()));
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of note_epoch_plan_main.cpp\n");
    return 1;
}
