// ASan / UBSan driver for the text stage's host face (test infrastructure; built and run by tests/test_sanitize_text.py, CPU only).
// argv[1] is a TrueType file holding the nine glyphs of the pitch names.  The program loads it, lays out and draws the reference's
// twelve labels with exactly sized buffers on images that are no multiple of anything, and checks that every pixel with non-zero
// coverage lies in a label's pixel box, hence in a 16 x 16 tile the device stage would launch.  Then it feeds the reader every
// truncation of the file and 2 000 single-byte corruptions from a fixed seed: each must return a status — and, where the font is
// still taken, glyph queries and a drawn picture must too — without touching memory outside the buffer (the copy handed to the
// reader is exactly as long as the bytes) and without overflowing a float-to-integer cast.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "text_host.hpp"

using namespace pvq;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned next_u32() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (unsigned)((rng_state * 2685821657736338717ull) >> 32);
}

static const uint32_t CODEPOINTS[9] = {'C', 'D', 'E', 'F', 'G', 'A', 'B', 0x266F, 0x266D};

// every status is fine; what is checked is that nothing faults.  Returns how many steps succeeded.
static int exercise(const std::vector<uint8_t>& bytes, const pvq_text_label* labels) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);   // no slack behind the last byte
    if (!bytes.empty()) std::memcpy(exact.get(), bytes.data(), bytes.size());
    std::unique_ptr<TextFont> font;
    std::string err;
    if (TextFont::from_ttf(exact.get(), bytes.size(), font, err) != PVQ_OK) return err.empty() ? -1000 : 0;
    int ok = 1;
    for (uint32_t cp : CODEPOINTS) {
        const TextGlyph* g = nullptr;
        if (font->glyph(cp, g, err) == PVQ_OK && g) ++ok;
    }
    std::vector<TextLabelPlan> plans;
    if (text_plan("fuzz", *font, labels, 12, 45, 29, 15.74f, plans, err) == PVQ_OK) {
        std::vector<float> img(45 * 29 * 4, 0.25f), cov(12 * 45 * 29);
        text_frame(plans, 45, 29, img.data(), cov.data());
        ++ok;
    }
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<uint8_t> file;
    {
        FILE* fh = std::fopen(argv[1], "rb");
        if (!fh) return 2;
        uint8_t buf[4096];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, fh)) > 0) file.insert(file.end(), buf, buf + got);
        std::fclose(fh);
    }
    pvq_text_label labels[12];
    text_pitch_labels(7, nullptr, labels);
    std::unique_ptr<TextFont> font;
    std::string err;
    if (TextFont::from_ttf(file.data(), file.size(), font, err) != PVQ_OK) {
        std::printf("the font was refused: %s\n", err.c_str());
        return 1;
    }
    // 1. the twelve labels, drawn; every covered pixel lies in its label's box, and so in a tile of the device stage's list
    const uint32_t sizes[][2] = {{64, 64}, {256, 256}, {301, 173}, {17, 5}, {1, 1}, {1280, 720}};
    const float views[] = {15.74f, 40.0f, 3.0f};
    size_t covered = 0, pixels = 0;
    for (const auto& wh : sizes)
        for (float vh : views) {
            const uint32_t W = wh[0], H = wh[1];
            std::vector<TextLabelPlan> plans;
            const pvq_status st = text_plan("sanitize", *font, labels, 12, W, H, vh, plans, err);
            if (st != PVQ_OK) {
                std::printf("%u x %u at %g: %s\n", W, H, vh, err.c_str());
                return 1;
            }
            std::vector<float> img(static_cast<size_t>(W) * H * 4), cov(static_cast<size_t>(12) * W * H);
            for (float& v : img) v = (float)(next_u32() >> 8) / 16777216.0f;
            const std::vector<float> before = img;
            text_frame(plans, W, H, img.data(), cov.data());
            const uint32_t tiles_x = (W + 15) / 16;
            std::vector<uint8_t> launched(static_cast<size_t>(tiles_x) * ((H + 15) / 16), 0);
            for (const TextLabelPlan& p : plans) {
                if (!p.on_image) continue;
                if (p.x1 >= W || p.y1 >= H || p.x0 > p.x1 || p.y0 > p.y1) return 1;
                for (uint32_t ty = p.y0 / 16; ty <= p.y1 / 16; ++ty)
                    for (uint32_t tx = p.x0 / 16; tx <= p.x1 / 16; ++tx) launched[ty * tiles_x + tx] = 1;
            }
            for (uint32_t l = 0; l < 12; ++l)
                for (uint32_t j = 0; j < H; ++j)
                    for (uint32_t i = 0; i < W; ++i) {
                        const float c = cov[(static_cast<size_t>(l) * H + j) * W + i];
                        if (!(c >= 0.0f && c <= 1.0f)) return 1;
                        if (c == 0.0f) continue;
                        ++covered;
                        const TextLabelPlan& p = plans[l];
                        if (!p.on_image || i < p.x0 || i > p.x1 || j < p.y0 || j > p.y1 || !launched[(j / 16) * tiles_x + i / 16]) {
                            std::printf("label %u covers pixel (%u, %u) of %u x %u outside its box\n", l, i, j, W, H);
                            return 1;
                        }
                    }
            for (size_t k = 0; k < img.size(); k += 4) {
                bool any = false;
                for (uint32_t l = 0; l < 12; ++l) any = any || cov[static_cast<size_t>(l) * W * H + k / 4] != 0.0f;
                if (!any && std::memcmp(&img[k], &before[k], 16)) return 1;   // an uncovered pixel was touched
            }
            pixels += static_cast<size_t>(W) * H;
        }
    if (covered == 0) return 1;
    // 2. labels far off, huge and tiny, and the em limit
    {
        pvq_text_label odd[4];
        for (auto& o : odd) o = labels[3];
        odd[0].x = 3e38f, odd[0].y = -3e38f;
        odd[1].scale = 1e-30f;
        odd[2].font_px = 1e-20f;
        odd[3].x = -1e6f;
        std::vector<TextLabelPlan> plans;
        if (text_plan("sanitize", *font, odd, 4, 33, 17, 15.74f, plans, err) != PVQ_OK) return 1;
        std::vector<float> img(33 * 17 * 4, 0.5f), cov(4 * 33 * 17);
        text_frame(plans, 33, 17, img.data(), cov.data());
        odd[0] = labels[3];
        odd[0].scale = 1e30f;
        if (text_plan("sanitize", *font, odd, 1, 33, 17, 15.74f, plans, err) != PVQ_ERR_INVALID_ARG) return 1;
    }
    // 3. the reader on bad bytes
    size_t taken = 0, refused = 0;
    for (size_t n = 0; n < file.size(); ++n) {
        const int r = exercise(std::vector<uint8_t>(file.begin(), file.begin() + n), labels);
        if (r < 0) return 1;   // a refusal without a text
        r ? ++taken : ++refused;
    }
    for (int k = 0; k < 2000; ++k) {
        std::vector<uint8_t> bad = file;
        const size_t at = next_u32() % bad.size();
        uint8_t v = (uint8_t)(next_u32() >> 24);
        if (v == bad[at]) v = (uint8_t)~v;
        bad[at] = v;
        const int r = exercise(bad, labels);
        if (r < 0) return 1;
        r ? ++taken : ++refused;
    }
    if (refused == 0) return 1;
    std::printf("SANITIZE_TEXT_OK %zu pixels, %zu covered, %zu bad fonts refused, %zu taken\n", pixels, covered, refused, taken);
    return 0;
}
