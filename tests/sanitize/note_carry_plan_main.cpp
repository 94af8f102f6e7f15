// note_carry_plan_main.cpp — the host planner of the note model's carried windows (note_model_plan.cpp: note_carry_plan, and
// note_carry_row, the rule the device expands a descriptor by) behind a command line, for tests/test_note_carry.py: built with
// -fsanitize=address,undefined and run once per question, in the pattern of note_plan_main.cpp.
//
//   plan <n_bins> <t_frames> <stride> <n_streams> <n_calls> <count> ...      n_calls * n_streams counts, call by call
//        The calls in order, the counts of frames seen carried from one to the next as NoteCarry does.  Per call one line
//        "call C rows R tiles K max_rows M max_n N", one line "stream S seen B first_row A f_first F rows R head H n N" per stream
//        and one line "row I stream S f F in_stitch 0|1 at A out_row O" per model row, I its place in the call's row list.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "note_model_plan.hpp"

using namespace pvq;

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const std::string cmd = argv[1];
    auto num = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
    if (cmd == "plan" && argc >= 7) {
        NoteModelDims d;
        d.n_bins = static_cast<uint32_t>(num(2));
        d.t_frames = static_cast<uint32_t>(num(3));
        d.L = d.n_bins * d.t_frames;
        const size_t stride = num(4);
        const uint32_t n_streams = static_cast<uint32_t>(num(5));
        const size_t n_calls = num(6);
        if (static_cast<size_t>(argc) != 7 + n_calls * n_streams) return 1;
        std::vector<uint64_t> seen(n_streams, 0);
        NcPlan plan;
        for (size_t c = 0; c < n_calls; ++c) {
            std::vector<size_t> nf(n_streams);
            for (uint32_t s = 0; s < n_streams; ++s) nf[s] = num(static_cast<int>(7 + c * n_streams + s));
            std::string err;
            if (note_carry_plan(d, seen.data(), nf.data(), n_streams, stride, plan, err) != PVQ_OK) {
                std::fprintf(stderr, "%s\n", err.c_str());
                return 3;
            }
            std::printf("call %zu rows %llu tiles %llu max_rows %u max_n %u\n", c, static_cast<unsigned long long>(plan.total_rows),
                        static_cast<unsigned long long>(plan.tiles), plan.max_rows, plan.max_n);
            for (uint32_t s = 0; s < n_streams; ++s) {
                const NcStream& st = plan.streams[s];
                std::printf("stream %u seen %llu first_row %u f_first %u rows %u head %u n %u\n", s, static_cast<unsigned long long>(seen[s]), st.first_row,
                            st.f_first, st.rows, st.head, st.n);
            }
            for (uint32_t s = 0; s < n_streams; ++s) {
                const NcStream& st = plan.streams[s];
                for (uint32_t i = 0; i < st.rows; ++i) {
                    const NcRow r = note_carry_row(st, s, i, d.t_frames, d.n_bins, stride);
                    std::printf("row %u stream %u f %u in_stitch %d at %llu out_row %llu\n", st.first_row + i, s, st.f_first + i, r.in_stitch ? 1 : 0,
                                static_cast<unsigned long long>(r.at), static_cast<unsigned long long>(r.out_row));
                }
                seen[s] += st.n;
            }
        }
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of note_carry_plan_main.cpp\n");
    return 1;
}
