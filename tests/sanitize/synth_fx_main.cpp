// ASan / UBSan driver for the synth stage's effects on the host (test infrastructure; built and run by tests/test_sanitize_synth_fx.py,
// CPU only).  argv[1] is a file the test writes from tests/synth_fx_cases.py: the bank's arrays and every case's event list, sample
// rate included.  The program renders every case with effects — in one call and in three, which must give the same bits — with
// exactly sized buffers, checks that the plan carries one send per record, and drives the effects-only face with a unit impulse at
// every admitted edge rate: a read or write outside a reverb buffer, the chorus ring or the delay table aborts the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "synth_host.hpp"

using namespace pvq;

struct Case {
    std::vector<double> time;
    std::vector<int32_t> channel, command, data1, data2;
    size_t n_blocks = 0;
    uint32_t polyphony = 64;
    int32_t sample_rate = 22050;
    SynthEvents events() const { return SynthEvents{time.data(), channel.data(), command.data(), data1.data(), data2.data(), time.size()}; }
};

template <typename T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int fail(const char* what, const std::string& err) {
    std::printf("FAILED: %s: %s\n", what, err.c_str());
    return 1;
}

static pvq_status render(std::shared_ptr<const SynthBank> bank, const Case& c, const std::vector<size_t>& calls, std::vector<float>& left,
                         std::vector<float>& right, std::string& err) {
    std::unique_ptr<SynthState> st;
    if (pvq_status s = SynthState::create(bank, c.sample_rate, c.polyphony, st, err, true)) return s;
    left.assign(c.n_blocks * 64, 0.0f);
    right.assign(c.n_blocks * 64, 0.0f);
    size_t done = 0;
    for (size_t n : calls) {
        std::vector<float> l(n * 64), r(n * 64);   // exactly the call's size
        if (pvq_status s = st->render(c.events(), n, nullptr, 0, l.data(), r.data(), err)) return s;
        if (st->last_plan().sends.size() != st->last_plan().records.size()) {
            err = "the plan's sends do not match its records";
            return PVQ_ERR_INTERNAL;
        }
        std::copy(l.begin(), l.end(), left.begin() + done * 64);
        std::copy(r.begin(), r.end(), right.begin() + done * 64);
        done += n;
    }
    return PVQ_OK;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[7];
    if (fread(head, sizeof(uint64_t), 7, f) != 7) return 2;
    std::vector<int16_t> wave, igs, pgs;
    std::vector<int32_t> samples, presets;
    std::vector<uint32_t> ismp, instruments, pins;
    bool ok = read_vec(f, wave, head[0]) && read_vec(f, samples, head[1] * 7) && read_vec(f, igs, head[2] * 61) && read_vec(f, ismp, head[2]) &&
              read_vec(f, instruments, head[3] * 2) && read_vec(f, pgs, head[4] * 61) && read_vec(f, pins, head[4]) && read_vec(f, presets, head[5] * 4);
    std::vector<Case> cases(head[6]);
    for (Case& c : cases) {
        uint64_t h[4];
        ok = ok && fread(h, sizeof(uint64_t), 4, f) == 4;
        if (!ok) break;
        c.n_blocks = h[1];
        c.polyphony = static_cast<uint32_t>(h[2]);
        c.sample_rate = static_cast<int32_t>(h[3]);
        ok = read_vec(f, c.time, h[0]) && read_vec(f, c.channel, h[0]) && read_vec(f, c.command, h[0]) && read_vec(f, c.data1, h[0]) &&
             read_vec(f, c.data2, h[0]);
    }
    std::fclose(f);
    if (!ok || cases.empty()) return 2;

    std::shared_ptr<const SynthBank> bank;
    std::string err;
    if (SynthBank::create(wave.data(), wave.size(), samples.data(), static_cast<uint32_t>(samples.size() / 7), igs.data(), ismp.data(),
                          static_cast<uint32_t>(ismp.size()), instruments.data(), static_cast<uint32_t>(instruments.size() / 2), pgs.data(), pins.data(),
                          static_cast<uint32_t>(pins.size()), presets.data(), static_cast<uint32_t>(presets.size() / 4), bank, err) != PVQ_OK)
        return fail("the bank", err);
    // 1. every case with effects, in one call and in three
    size_t rendered = 0, sounding = 0;
    for (const Case& c : cases) {
        std::vector<float> l1, r1, l3, r3;
        if (render(bank, c, {c.n_blocks}, l1, r1, err) != PVQ_OK) return fail("a case", err);
        const size_t first = c.n_blocks / 3, second = 1;
        if (render(bank, c, {first, second, c.n_blocks - first - second}, l3, r3, err) != PVQ_OK) return fail("a case in three calls", err);
        if (std::memcmp(l1.data(), l3.data(), l1.size() * sizeof(float)) || std::memcmp(r1.data(), r3.data(), r1.size() * sizeof(float)))
            return fail("three calls differ from one", "");
        for (float v : l1)
            if (v != 0.0f) {
                ++sounding;
                break;
            }
        ++rendered;
    }
    // 2. the effects-only face with a unit impulse, at the edge rates and two between; a rate outside is refused
    size_t impulses = 0;
    for (int32_t sr : {16000, 22050, 44100, 48000, 192000}) {
        std::unique_ptr<SynthEffects> fx;
        if (SynthEffects::create(sr, fx, err) != PVQ_OK) return fail("effects create", err);
        const synth::FxLayout& l = fx->layout();
        const size_t n_blocks = (l.len[synth::FX_COMBS] + 63) / 64 + 2, n = n_blocks * 64;   // past the right channel's first comb
        std::vector<float> cl(n, 0.25f), cr(n, -0.25f), in(n, 0.0f), ol(n), orr(n), rl(n), rr(n);   // exactly sized
        in[0] = 1.0f;
        fx->process(1, cl.data(), cr.data(), in.data(), ol.data(), orr.data(), rl.data(), rr.data());   // in two calls
        fx->process(n_blocks - 1, cl.data() + 64, cr.data() + 64, in.data() + 64, ol.data() + 64, orr.data() + 64, rl.data() + 64, rr.data() + 64);
        for (size_t t = 0; t < l.len[0]; ++t)
            if (rl[t] != 0.0f) return fail("the impulse came back early on the left", std::to_string(sr));
        if (rl[l.len[0]] != 1.0f || rr[l.len[synth::FX_COMBS]] != 1.0f) return fail("the impulse did not come back as 1", std::to_string(sr));
        if (ol[n - 1] != 0.25f || orr[n - 1] != -0.25f) return fail("a constant chorus input did not come out unchanged", std::to_string(sr));
        ++impulses;
    }
    std::unique_ptr<SynthEffects> none;
    if (SynthEffects::create(15999, none, err) != PVQ_ERR_INVALID_ARG || SynthEffects::create(192001, none, err) != PVQ_ERR_INVALID_ARG)
        return fail("a sample rate outside 16 000 .. 192 000 was not refused", err);
    std::printf("rendered %zu cases (%zu sounding), %zu impulses\nSANITIZE_SYNTH_FX_OK\n", rendered, sounding, impulses);
    return rendered == cases.size() && sounding + 1 == rendered && impulses == 5 ? 0 : 1;
}
