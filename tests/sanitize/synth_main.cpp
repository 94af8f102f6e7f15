// ASan / UBSan driver for the synth stage's host face (test infrastructure; built and run by tests/test_sanitize_synth.py, CPU only).
// argv[1] is a file tests/test_sanitize_synth.py writes from tests/synth_cases.py: the bank's arrays and every case's event list.
// The program renders every case — in one call and in three, which must give the same bits — with exactly sized buffers, expects the
// runaway case to be refused, and then corrupts, in turn, every index field of the bank (sample points, loop points, sample rates,
// sample and instrument indices, region ranges, the address-offset generators, every generator of a region at both ends of i16) and
// feeds event lists with every channel, command, key, velocity and controller value 0 .. 255: each corruption must be either
// rejected or rendered, and a read outside wave_data, an overflowing cast or a bad shift aborts the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "synth_host.hpp"

using namespace pvq;

struct BankArrays {
    std::vector<int16_t> wave, igs, pgs;
    std::vector<int32_t> samples, presets;
    std::vector<uint32_t> ismp, instruments, pins;
};
struct Case {
    std::vector<double> time;
    std::vector<int32_t> channel, command, data1, data2;
    size_t n_blocks = 0;
    uint32_t polyphony = 64;
    SynthEvents events() const { return SynthEvents{time.data(), channel.data(), command.data(), data1.data(), data2.data(), time.size()}; }
};

template <typename T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static pvq_status make_bank(const BankArrays& a, std::shared_ptr<const SynthBank>& bank, std::string& err) {
    // exact copies: nothing behind the last element
    const BankArrays b = a;
    return SynthBank::create(b.wave.data(), b.wave.size(), b.samples.data(), static_cast<uint32_t>(b.samples.size() / 7), b.igs.data(), b.ismp.data(),
                             static_cast<uint32_t>(b.ismp.size()), b.instruments.data(), static_cast<uint32_t>(b.instruments.size() / 2), b.pgs.data(),
                             b.pins.data(), static_cast<uint32_t>(b.pins.size()), b.presets.data(), static_cast<uint32_t>(b.presets.size() / 4), bank, err);
}

// returns the status; fills left / right
static pvq_status render(std::shared_ptr<const SynthBank> bank, const Case& c, const std::vector<size_t>& calls, std::vector<float>& left,
                         std::vector<float>& right, std::string& err) {
    std::unique_ptr<SynthState> st;
    if (pvq_status s = SynthState::create(bank, 22050, c.polyphony, st, err)) return s;
    left.assign(c.n_blocks * 64, 0.0f);
    right.assign(c.n_blocks * 64, 0.0f);
    size_t done = 0;
    for (size_t n : calls) {
        const uint32_t snaps[2] = {0u, static_cast<uint32_t>(n > 1 ? n - 1 : 1)};
        std::vector<float> l(n * 64), r(n * 64);   // exactly the call's size
        if (pvq_status s = st->render(c.events(), n, snaps, 2, l.data(), r.data(), err)) return s;
        std::copy(l.begin(), l.end(), left.begin() + done * 64);
        std::copy(r.begin(), r.end(), right.begin() + done * 64);
        done += n;
    }
    return PVQ_OK;
}

static int fail(const char* what, const std::string& err) {
    std::printf("FAILED: %s: %s\n", what, err.c_str());
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[8];
    if (fread(head, sizeof(uint64_t), 8, f) != 8) return 2;
    BankArrays a;
    bool ok = read_vec(f, a.wave, head[0]) && read_vec(f, a.samples, head[1] * 7) && read_vec(f, a.igs, head[2] * 61) && read_vec(f, a.ismp, head[2]) &&
              read_vec(f, a.instruments, head[3] * 2) && read_vec(f, a.pgs, head[4] * 61) && read_vec(f, a.pins, head[4]) &&
              read_vec(f, a.presets, head[5] * 4);
    std::vector<Case> cases(head[6]);
    for (Case& c : cases) {
        uint64_t h[3];
        ok = ok && fread(h, sizeof(uint64_t), 3, f) == 3;
        if (!ok) break;
        c.n_blocks = h[1];
        c.polyphony = static_cast<uint32_t>(h[2]);
        ok = read_vec(f, c.time, h[0]) && read_vec(f, c.channel, h[0]) && read_vec(f, c.command, h[0]) && read_vec(f, c.data1, h[0]) &&
             read_vec(f, c.data2, h[0]);
    }
    std::fclose(f);
    if (!ok || cases.size() < 2) return 2;
    const size_t runaway = head[7];   // index of the case that must be refused

    std::shared_ptr<const SynthBank> bank;
    std::string err;
    if (make_bank(a, bank, err) != PVQ_OK) return fail("the bank", err);
    // 1. every case, in one call and in three
    size_t refused = 0, rendered = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        std::vector<float> l1, r1, l3, r3;
        const pvq_status s1 = render(bank, c, {c.n_blocks}, l1, r1, err);
        if (i == runaway) {
            if (s1 != PVQ_ERR_INVALID_ARG || err.find("outside wave_data") == std::string::npos) return fail("the runaway case was not refused", err);
            ++refused;
            continue;
        }
        if (s1 != PVQ_OK) return fail("a case", err);
        const size_t first = c.n_blocks / 3, second = 1;
        if (render(bank, c, {first, second, c.n_blocks - first - second}, l3, r3, err) != PVQ_OK) return fail("a case in three calls", err);
        if (std::memcmp(l1.data(), l3.data(), l1.size() * sizeof(float)) || std::memcmp(r1.data(), r3.data(), r1.size() * sizeof(float)))
            return fail("three calls differ from one", "");
        ++rendered;
    }
    // 2. the bank's index fields, corrupted in turn; every accepted bank plays every case for 48 blocks
    size_t rejected = 0, accepted = 0, refused_reads = 0;
    auto try_bank = [&](const BankArrays& b) -> int {
        std::shared_ptr<const SynthBank> bad;
        std::string e;
        const pvq_status s = make_bank(b, bad, e);
        if (s != PVQ_OK) {
            if (s != PVQ_ERR_INVALID_ARG || e.empty()) return fail("a corrupted bank: status or text", e);
            ++rejected;
            return 0;
        }
        ++accepted;
        for (const Case& c : cases) {
            Case shorter = c;
            shorter.n_blocks = std::min<size_t>(c.n_blocks, 48);
            std::vector<float> l, r;
            const pvq_status sr = render(bad, shorter, {shorter.n_blocks}, l, r, e);
            if (sr == PVQ_ERR_INVALID_ARG) ++refused_reads;
            else if (sr != PVQ_OK) return fail("a corrupted bank: render status", e);
        }
        return 0;
    };
    const int32_t nw = static_cast<int32_t>(a.wave.size());
    const int32_t points[] = {-1, 0, 1, nw - 1, nw, nw + 1, 0x7fffffff, static_cast<int32_t>(0x80000000u)};
    for (size_t s = 0; s < a.samples.size() / 7; ++s)
        for (int field = 0; field < 7; ++field)
            for (int32_t v : points) {   // sample bounds, loop points, sample rate, original pitch, pitch correction
                BankArrays b = a;
                b.samples[7 * s + field] = v;
                if (try_bank(b)) return 1;
            }
    for (size_t s = 0; s < a.samples.size() / 7; ++s) {   // loop points swapped, and an empty loop
        BankArrays b = a;
        std::swap(b.samples[7 * s + 2], b.samples[7 * s + 3]);
        if (try_bank(b)) return 1;
        b = a;
        b.samples[7 * s + 3] = b.samples[7 * s + 2];
        if (try_bank(b)) return 1;
        b = a;
        b.samples[7 * s + 1] = b.samples[7 * s + 0];   // end == start
        if (try_bank(b)) return 1;
    }
    const uint32_t indices[] = {0u, 1u, 1000u, 0x7fffffffu, 0xffffffffu};
    for (size_t i = 0; i < a.ismp.size(); ++i)
        for (uint32_t v : indices) {
            BankArrays b = a;
            b.ismp[i] = v < a.samples.size() / 7 ? v : (v == 1000u ? static_cast<uint32_t>(a.samples.size() / 7) : v);
            if (try_bank(b)) return 1;
        }
    for (size_t i = 0; i < a.pins.size(); ++i)
        for (uint32_t v : indices) {
            BankArrays b = a;
            b.pins[i] = v < a.instruments.size() / 2 ? v : (v == 1000u ? static_cast<uint32_t>(a.instruments.size() / 2) : v);
            if (try_bank(b)) return 1;
        }
    for (size_t i = 0; i < a.instruments.size(); ++i)
        for (uint32_t v : indices) {
            BankArrays b = a;
            b.instruments[i] = v;
            if (try_bank(b)) return 1;
        }
    for (size_t i = 0; i < a.presets.size(); ++i)
        for (int32_t v : points) {
            BankArrays b = a;
            b.presets[i] = v;
            if (try_bank(b)) return 1;
        }
    const int16_t ends[] = {-32768, -1, 1, 32767};
    const int offset_gens[] = {0, 1, 2, 3, 4, 12, 45, 50};
    for (size_t i = 0; i < a.ismp.size(); ++i)
        for (int g : offset_gens)
            for (int16_t v : ends) {   // the address offsets move the sample points
                BankArrays b = a;
                b.igs[61 * i + g] = v;
                if (try_bank(b)) return 1;
            }
    for (int g = 0; g < 61; ++g)
        for (int16_t v : ends) {   // every generator at both ends, in every instrument region at once and in every preset region at once
            BankArrays b = a;
            for (size_t i = 0; i < a.ismp.size(); ++i)
                if (g != 43 && g != 44) b.igs[61 * i + g] = v;
            if (try_bank(b)) return 1;
            b = a;
            for (size_t i = 0; i < a.pins.size(); ++i)
                if (g != 43 && g != 44) b.pgs[61 * i + g] = v;
            if (try_bank(b)) return 1;
        }
    // 3. event bytes 0 .. 255 on the good bank: channels, commands, keys and velocities, controllers and their values
    Case sweep;
    sweep.n_blocks = 64;
    auto push = [&](double t, int ch, int cmd, int d1, int d2) {
        sweep.time.push_back(t);
        sweep.channel.push_back(ch);
        sweep.command.push_back(cmd);
        sweep.data1.push_back(d1);
        sweep.data2.push_back(d2);
    };
    double t = 0.0;
    for (int ch = 0; ch < 256; ++ch) push(t += 1e-5, ch, 0x90, 60, 100);
    for (int cmd = 0; cmd < 256; ++cmd) push(t += 1e-5, cmd & 15, cmd, (cmd * 7) & 255, (cmd * 13) & 255);
    for (int patch = 0; patch < 256; ++patch) {
        push(t += 1e-5, patch & 15, 0xB0, 0x00, (patch * 5) & 255);
        push(t += 1e-5, patch & 15, 0xC0, patch, 0);
        push(t += 1e-5, patch & 15, 0x90, patch, 255 - patch);
    }
    for (int key = 0; key < 256; ++key)
        for (int vel : {0, 1, 127, 128, 255}) push(t += 1e-5, key & 7, 0x90, key, vel);
    for (int cc = 0; cc < 256; ++cc)
        for (int v : {0, 63, 64, 127, 128, 255}) push(t += 1e-5, cc & 15, 0xB0, cc, v);
    for (int v = 0; v < 256; ++v) push(t += 1e-5, 0, 0xE0, v, 255 - v);
    for (int key = 0; key < 256; ++key) push(t += 1e-5, key & 15, 0x80, key, 0);
    {
        std::vector<float> l, r;
        const pvq_status s = render(bank, sweep, {sweep.n_blocks}, l, r, err);
        if (s != PVQ_OK && s != PVQ_ERR_INVALID_ARG) return fail("the event sweep", err);
        Case bad = sweep;
        bad.channel[3] = 256;
        if (render(bank, bad, {1}, l, r, err) != PVQ_ERR_INVALID_ARG) return fail("a byte of 256 was taken", err);
        bad = sweep;
        bad.data2[5] = -1;
        if (render(bank, bad, {1}, l, r, err) != PVQ_ERR_INVALID_ARG) return fail("a byte of -1 was taken", err);
    }
    std::printf("cases rendered %zu refused %zu; corrupted banks rejected %zu accepted %zu (renders refused %zu)\n", rendered, refused, rejected, accepted,
                refused_reads);
    if (refused != 1 || rejected < 100 || accepted < 100) return fail("the corruption sweep did not reach both outcomes", "");
    std::printf("SANITIZE_SYNTH_OK\n");
    return 0;
}
