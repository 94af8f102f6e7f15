// Stand-alone driver for pitchvis_amd/csrc/stage_plan.cpp under ASan/UBSan (tests/test_stage_plan.py).  The arguments are a list of
// questions, answered one line each, in order:
//   image WHO WIDTH HEIGHT VIEWPORT_HEIGHT | mode WHO MODE | frames WHO N_FRAMES N_STREAMS   ->  "ok" or "refused <text>"
//   piece N_FRAMES N_STREAMS PER_ROW LIMIT                                                  ->  the piece's frames
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "stage_plan.hpp"

static unsigned long long u64(const char* s) { return std::strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
    int i = 1;
    auto left = [&](int n) { return i + n < argc; };
    while (i < argc) {
        const char* what = argv[i];
        std::string err;
        bool ok = false;
        if (!std::strcmp(what, "image") && left(4)) {
            ok = pvq::stage_image_ok(argv[i + 1], static_cast<uint32_t>(u64(argv[i + 2])), static_cast<uint32_t>(u64(argv[i + 3])),
                                     std::strtof(argv[i + 4], nullptr), err);
            i += 5;
        } else if (!std::strcmp(what, "mode") && left(2)) {
            ok = pvq::stage_mode_ok(argv[i + 1], std::atoi(argv[i + 2]), err);
            i += 3;
        } else if (!std::strcmp(what, "frames") && left(3)) {
            ok = pvq::stage_frames_ok(argv[i + 1], static_cast<size_t>(u64(argv[i + 2])), static_cast<uint32_t>(u64(argv[i + 3])), err);
            i += 4;
        } else if (!std::strcmp(what, "piece") && left(4)) {
            std::printf("%zu\n", pvq::stage_piece_frames(static_cast<size_t>(u64(argv[i + 1])), static_cast<uint32_t>(u64(argv[i + 2])),
                                                         static_cast<size_t>(u64(argv[i + 3])), static_cast<size_t>(u64(argv[i + 4]))));
            i += 5;
            continue;
        } else {
            std::fprintf(stderr, "bad question at argument %d: %s\n", i, what);
            return 2;
        }
        std::printf("%s\n", ok ? "ok" : ("refused " + err).c_str());
    }
    return 0;
}
