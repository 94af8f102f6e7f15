// text_host.cpp — see text_host.hpp.  Built with -ffp-contract=off.
#include "text_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace pvq {

namespace {
// pitchvis_colors/src/lib.rs:19-36 and :36-38
const float DEFAULT_COLORS[12][3] = {
    {0.85f, 0.36f, 0.36f}, {0.01f, 0.52f, 0.71f}, {0.97f, 0.76f, 0.05f}, {0.45f, 0.34f, 0.63f}, {0.47f, 0.77f, 0.22f}, {0.78f, 0.32f, 0.52f},
    {0.00f, 0.64f, 0.56f}, {0.95f, 0.54f, 0.23f}, {0.30f, 0.37f, 0.64f}, {1.00f, 0.96f, 0.03f}, {0.57f, 0.30f, 0.55f}, {0.12f, 0.71f, 0.34f},
};
const char* const PITCH_NAMES[12] = {"C", "C\xE2\x99\xAF", "D", "E\xE2\x99\xAD", "E", "F", "F\xE2\x99\xAF", "G", "A\xE2\x99\xAD", "A", "B\xE2\x99\xAD", "B"};

constexpr float MAX_COORD = 65536.0f;   // font units, either sign: twice what a TrueType coordinate can reach
constexpr uint32_t MIN_UPEM = 16, MAX_UPEM = 16384;

// ---- big-endian reads of a checked range ----
struct Bytes {
    const uint8_t* p;
    size_t n;
    bool has(size_t at, size_t len) const { return at <= n && len <= n - at; }
    uint16_t u16(size_t at) const { return static_cast<uint16_t>(p[at] << 8 | p[at + 1]); }
    int16_t i16(size_t at) const { return static_cast<int16_t>(u16(at)); }
    uint32_t u32(size_t at) const { return static_cast<uint32_t>(p[at]) << 24 | static_cast<uint32_t>(p[at + 1]) << 16 | static_cast<uint32_t>(p[at + 2]) << 8 | p[at + 3]; }
};

pvq_status bad(std::string& err, const char* table, const char* what) {
    err = std::string("text font: the ") + table + " table " + what;
    return PVQ_ERR_INVALID_ARG;
}

bool glyph_ok(const TextGlyph& g, std::string& why) {
    const size_t n = g.on_curve.size();
    if (g.points.size() != 2 * n) return why = "points and flags differ in length", false;
    if (!std::isfinite(g.advance) || g.advance < 0.0f || g.advance > MAX_COORD) return why = "advance is not 0 .. 65536", false;
    uint32_t prev = 0;
    for (size_t c = 0; c < g.contour_ends.size(); ++c) {
        const uint32_t e = g.contour_ends[c];
        if (e >= n || (c > 0 && e <= prev)) return why = "contour ends must ascend and lie within the points", false;
        prev = e;
    }
    if (g.contour_ends.empty() ? n != 0 : g.contour_ends.back() + 1 != n) return why = "the last contour must end at the last point", false;
    for (float v : g.points)
        if (!(std::fabs(v) <= MAX_COORD)) return why = "a coordinate is not within +-65536 font units", false;
    return true;
}

// the next codepoint of a UTF-8 string: false at a byte sequence that is not UTF-8 (overlong forms and surrogates included)
bool next_codepoint(const unsigned char*& s, const unsigned char* end, uint32_t& cp) {
    const unsigned char b = *s;
    int extra;
    if (b < 0x80) cp = b, extra = 0;
    else if ((b & 0xE0) == 0xC0) cp = b & 0x1Fu, extra = 1;
    else if ((b & 0xF0) == 0xE0) cp = b & 0x0Fu, extra = 2;
    else if ((b & 0xF8) == 0xF0) cp = b & 0x07u, extra = 3;
    else return false;
    if (end - s <= extra) return false;
    for (int k = 1; k <= extra; ++k) {
        if ((s[k] & 0xC0) != 0x80) return false;
        cp = cp << 6 | (s[k] & 0x3Fu);
    }
    static const uint32_t least[4] = {0u, 0x80u, 0x800u, 0x10000u};
    if (cp < least[extra] || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) return false;
    s += extra + 1;
    return true;
}

std::string name_of(uint32_t cp) {
    char t[16];
    std::snprintf(t, sizeof t, "U+%04X", cp);
    return t;
}

using Pt = TextPoint;
}  // namespace

// ---- the font -------------------------------------------------------------------------------------------------------------------
pvq_status TextFont::from_outlines(uint32_t n_glyphs, const uint32_t* codepoints, const float* advances, const uint32_t* n_contours,
                                   const uint32_t* contour_ends, const uint32_t* n_points, const float* points, const uint8_t* on_curve,
                                   uint32_t units_per_em, float ascent, float descent, std::unique_ptr<TextFont>& out, std::string& err) {
    out.reset();
    if (n_glyphs == 0 || n_glyphs > 65535 || !codepoints || !advances || !n_contours || !n_points) {
        err = "text font: 1 .. 65535 glyphs, with codepoints, advances, contour counts and point counts";
        return PVQ_ERR_INVALID_ARG;
    }
    if (units_per_em < MIN_UPEM || units_per_em > MAX_UPEM || !(std::fabs(ascent) <= MAX_COORD) || !(std::fabs(descent) <= MAX_COORD)) {
        err = "text font: units_per_em is 16 .. 16384, ascent and descent within +-65536 font units";
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<TextFont> f(new TextFont());
    f->upem_ = units_per_em;
    f->ascent_ = ascent;
    f->descent_ = descent;
    size_t c_at = 0, p_at = 0;
    for (uint32_t g = 0; g < n_glyphs; ++g) {
        if (n_contours[g] > 65535 || n_points[g] > 65535 || ((n_contours[g] || n_points[g]) && (!contour_ends || !points || !on_curve))) {
            err = "text font: a glyph has at most 65535 contours and points, and its arrays are needed";
            return PVQ_ERR_INVALID_ARG;
        }
        TextGlyph gl;
        gl.advance = advances[g];
        gl.contour_ends.assign(contour_ends + c_at, contour_ends + c_at + n_contours[g]);
        gl.points.assign(points + 2 * p_at, points + 2 * (p_at + n_points[g]));
        gl.on_curve.resize(n_points[g]);
        for (uint32_t k = 0; k < n_points[g]; ++k) gl.on_curve[k] = on_curve[p_at + k] ? 1 : 0;
        c_at += n_contours[g];
        p_at += n_points[g];
        std::string why;
        if (codepoints[g] > 0x10FFFFu) why = "its codepoint is above U+10FFFF";
        if (!why.empty() || !glyph_ok(gl, why)) {
            err = "text font: glyph " + std::to_string(g) + ": " + why;
            return PVQ_ERR_INVALID_ARG;
        }
        if (!f->glyphs_.emplace(codepoints[g], std::move(gl)).second) {
            err = "text font: codepoint " + std::to_string(codepoints[g]) + " is given twice";
            return PVQ_ERR_INVALID_ARG;
        }
    }
    out = std::move(f);
    return PVQ_OK;
}

pvq_status TextFont::from_ttf(const uint8_t* bytes, size_t n_bytes, std::unique_ptr<TextFont>& out, std::string& err) {
    out.reset();
    if (!bytes || n_bytes < 12 || n_bytes > (size_t{1} << 30)) {
        err = "text font: TrueType bytes are needed (12 bytes .. 1 GiB)";
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<TextFont> f(new TextFont());
    f->bytes_.assign(bytes, bytes + n_bytes);
    f->from_bytes_ = true;
    const Bytes b{f->bytes_.data(), n_bytes};
    const uint32_t version = b.u32(0);
    if (version == 0x74746366u) {   // 'ttcf'
        err = "unsupported: a TrueType collection; pass one font";
        return PVQ_ERR_UNSUPPORTED;
    }
    if (version != 0x00010000u && version != 0x74727565u && version != 0x4F54544Fu) return bad(err, "offset", "does not begin a TrueType or OpenType font");
    const uint32_t n_tables = b.u16(4);
    if (!b.has(12, static_cast<size_t>(n_tables) * 16)) return bad(err, "offset", "lists more tables than the bytes hold");
    Table head, maxp, hhea, cmap;
    for (uint32_t t = 0; t < n_tables; ++t) {
        const size_t rec = 12 + static_cast<size_t>(t) * 16;
        const uint32_t tag = b.u32(rec);
        const Table tab{b.u32(rec + 8), b.u32(rec + 12)};
        Table* dst = tag == 0x68656164u ? &head : tag == 0x6D617870u ? &maxp : tag == 0x68686561u ? &hhea : tag == 0x686D7478u ? &f->hmtx_
                   : tag == 0x636D6170u ? &cmap : tag == 0x6C6F6361u ? &f->loca_ : tag == 0x676C7966u ? &f->glyf_ : nullptr;
        if (!dst) continue;
        if (!b.has(tab.at, tab.len)) {
            const char name[5] = {static_cast<char>(tag >> 24), static_cast<char>(tag >> 16), static_cast<char>(tag >> 8), static_cast<char>(tag), 0};
            return bad(err, name, "reaches past the end of the bytes");
        }
        *dst = tab;
    }
    if (head.len < 54) return bad(err, "head", "is missing or shorter than 54 bytes");
    if (maxp.len < 6) return bad(err, "maxp", "is missing or shorter than 6 bytes");
    if (hhea.len < 36) return bad(err, "hhea", "is missing or shorter than 36 bytes");
    f->upem_ = b.u16(head.at + 18);
    if (f->upem_ < MIN_UPEM || f->upem_ > MAX_UPEM) return bad(err, "head", "has a unitsPerEm outside 16 .. 16384");
    const int16_t loc_format = b.i16(head.at + 50);
    if (loc_format != 0 && loc_format != 1) return bad(err, "head", "has an indexToLocFormat that is neither 0 nor 1");
    f->long_loca_ = loc_format == 1;
    f->n_glyphs_ = b.u16(maxp.at + 4);
    f->ascent_ = static_cast<float>(b.i16(hhea.at + 4));
    f->descent_ = static_cast<float>(b.i16(hhea.at + 6));
    f->n_hmetrics_ = b.u16(hhea.at + 34);
    if (f->n_hmetrics_ == 0 || f->n_hmetrics_ > f->n_glyphs_) return bad(err, "hhea", "has a numberOfHMetrics that is 0 or above maxp's numGlyphs");
    if (f->hmtx_.len < static_cast<size_t>(f->n_hmetrics_) * 4) return bad(err, "hmtx", "is missing or shorter than hhea's numberOfHMetrics");
    // cmap: a Unicode subtable of format 12, else of format 4
    if (cmap.len < 4) return bad(err, "cmap", "is missing or shorter than its header");
    const uint32_t n_sub = b.u16(cmap.at + 2);
    if (cmap.len < 4 + static_cast<size_t>(n_sub) * 8) return bad(err, "cmap", "lists more subtables than it holds");
    for (uint32_t k = 0; k < n_sub; ++k) {
        const size_t rec = cmap.at + 4 + static_cast<size_t>(k) * 8;
        const uint32_t platform = b.u16(rec), encoding = b.u16(rec + 2), off = b.u32(rec + 4);
        if (!(platform == 0 || (platform == 3 && (encoding == 1 || encoding == 10)))) continue;
        if (off > cmap.len || cmap.len - off < 2) return bad(err, "cmap", "has a subtable offset past its end");
        const size_t at = cmap.at + off, room = cmap.len - off;
        const uint32_t format = b.u16(at);
        if (format == 12) {
            if (room < 16) return bad(err, "cmap", "has a format 12 subtable shorter than its header");
            const uint64_t groups = b.u32(at + 12);
            if (groups * 12 + 16 > room) return bad(err, "cmap", "has a format 12 subtable with more groups than it holds");
            f->cmap_sub_ = Table{at, static_cast<size_t>(groups * 12 + 16)};
            f->cmap_format_ = 12;
        } else if (format == 4 && f->cmap_format_ != 12) {
            if (room < 16) return bad(err, "cmap", "has a format 4 subtable shorter than its header");
            const uint32_t seg_x2 = b.u16(at + 6);
            if ((seg_x2 & 1u) || seg_x2 == 0 || 16 + static_cast<size_t>(seg_x2) * 4 > room) return bad(err, "cmap", "has a format 4 subtable with more segments than it holds");
            f->cmap_sub_ = Table{at, room};   // glyph ids may follow the segment arrays up to the table's end
            f->cmap_format_ = 4;
        }
    }
    if (f->cmap_format_ == 0) return bad(err, "cmap", "has no Unicode subtable of format 4 or 12");
    out = std::move(f);
    return PVQ_OK;
}

bool TextFont::glyph_index(uint32_t cp, uint32_t& gid) const {
    const Bytes b{bytes_.data(), bytes_.size()};
    const size_t at = cmap_sub_.at;
    gid = 0;
    if (cmap_format_ == 12) {
        const uint32_t groups = b.u32(at + 12);
        for (uint32_t g = 0; g < groups; ++g) {
            const size_t rec = at + 16 + static_cast<size_t>(g) * 12;
            const uint32_t first = b.u32(rec), last = b.u32(rec + 4);
            if (cp >= first && cp <= last) {
                const uint64_t id = static_cast<uint64_t>(b.u32(rec + 8)) + (cp - first);
                gid = id > 0xFFFFFFFFull ? 0u : static_cast<uint32_t>(id);
                break;
            }
        }
    } else {
        if (cp > 0xFFFFu) return false;
        const uint32_t seg_x2 = b.u16(at + 6);
        const size_t ends = at + 14, starts = at + 16 + seg_x2, deltas = starts + seg_x2, offsets = deltas + seg_x2;
        for (uint32_t k = 0; k < seg_x2; k += 2) {
            if (b.u16(ends + k) < cp) continue;
            const uint32_t first = b.u16(starts + k);
            if (first > cp) break;
            const uint32_t delta = b.u16(deltas + k), off = b.u16(offsets + k);
            if (off == 0) gid = (cp + delta) & 0xFFFFu;
            else {
                const size_t where = offsets + k + off + 2 * static_cast<size_t>(cp - first);
                if (where < at || where - at > cmap_sub_.len || cmap_sub_.len - (where - at) < 2) return false;   // past the subtable: no glyph
                const uint32_t id = b.u16(where);
                gid = id ? (id + delta) & 0xFFFFu : 0u;
            }
            break;
        }
    }
    return gid != 0;
}

pvq_status TextFont::read_glyph(uint32_t cp, TextGlyph& g, std::string& err) const {
    const Bytes b{bytes_.data(), bytes_.size()};
    uint32_t gid;
    if (!glyph_index(cp, gid)) {
        err = "text: the font has no glyph for " + name_of(cp);
        return PVQ_ERR_INVALID_ARG;
    }
    if (gid >= n_glyphs_) return bad(err, "cmap", "names a glyph above maxp's numGlyphs");
    if (glyf_.len == 0 && loca_.len == 0) {
        err = "unsupported: the font has no glyf outlines (CFF); the text stage reads TrueType outlines";
        return PVQ_ERR_UNSUPPORTED;
    }
    g.advance = static_cast<float>(b.u16(hmtx_.at + 4 * static_cast<size_t>(std::min(gid, n_hmetrics_ - 1u))));
    const size_t entry = long_loca_ ? 4 : 2;
    if (loca_.len < (static_cast<size_t>(gid) + 2) * entry) return bad(err, "loca", "is missing or ends before the glyph's entry");
    const size_t l = loca_.at + gid * entry;
    const size_t g0 = long_loca_ ? b.u32(l) : 2 * static_cast<size_t>(b.u16(l)), g1 = long_loca_ ? b.u32(l + 4) : 2 * static_cast<size_t>(b.u16(l + 2));
    if (g0 > g1 || g1 > glyf_.len) return bad(err, "loca", "has glyph offsets that descend or lie past glyf's end");
    if (g0 == g1) return PVQ_OK;   // no outline (a space)
    const Bytes gb{b.p + glyf_.at + g0, g1 - g0};   // the glyph's own bytes: nothing below reads outside them
    if (!gb.has(0, 10)) return bad(err, "glyf", "has a glyph shorter than its header");
    const int16_t n_contours = gb.i16(0);
    if (n_contours < 0) {
        err = "unsupported: a composite glyph (" + name_of(cp) + "); the text stage reads simple glyphs";
        return PVQ_ERR_UNSUPPORTED;
    }
    size_t at = 10;
    if (!gb.has(at, 2 * static_cast<size_t>(n_contours) + 2)) return bad(err, "glyf", "has a glyph whose contour ends reach past it");
    for (int c = 0; c < n_contours; ++c) {
        const uint32_t e = gb.u16(at + 2 * static_cast<size_t>(c));
        if (c > 0 && e <= g.contour_ends.back()) return bad(err, "glyf", "has a glyph whose contour ends do not ascend");
        g.contour_ends.push_back(e);
    }
    at += 2 * static_cast<size_t>(n_contours);
    const size_t n = n_contours ? g.contour_ends.back() + 1u : 0u;
    at += 2 + static_cast<size_t>(gb.u16(at));   // the hinting instructions are skipped, never interpreted
    std::vector<uint8_t> flags;
    flags.reserve(n);
    while (flags.size() < n) {
        if (!gb.has(at, 1)) return bad(err, "glyf", "has a glyph whose flags reach past it");
        const uint8_t fl = gb.p[at++];
        size_t times = 1;
        if (fl & 8u) {
            if (!gb.has(at, 1)) return bad(err, "glyf", "has a glyph whose flags reach past it");
            times += gb.p[at++];
        }
        if (times > n - flags.size()) return bad(err, "glyf", "has a glyph with more flags than points");
        flags.insert(flags.end(), times, fl);
    }
    g.points.assign(2 * n, 0.0f);
    g.on_curve.resize(n);
    for (int axis = 0; axis < 2; ++axis) {
        const uint8_t is_short = axis ? 4u : 2u, same = axis ? 32u : 16u;
        int64_t v = 0;
        for (size_t k = 0; k < n; ++k) {
            if (flags[k] & is_short) {
                if (!gb.has(at, 1)) return bad(err, "glyf", "has a glyph whose coordinates reach past it");
                const int64_t d = gb.p[at++];
                v += (flags[k] & same) ? d : -d;
            } else if (!(flags[k] & same)) {
                if (!gb.has(at, 2)) return bad(err, "glyf", "has a glyph whose coordinates reach past it");
                v += gb.i16(at);
                at += 2;
            }
            if (v < -65536 || v > 65536) return bad(err, "glyf", "has a glyph with a coordinate outside +-65536 font units");
            g.points[2 * k + axis] = static_cast<float>(v);
        }
    }
    for (size_t k = 0; k < n; ++k) g.on_curve[k] = flags[k] & 1u;
    return PVQ_OK;
}

pvq_status TextFont::glyph(uint32_t cp, const TextGlyph*& out, std::string& err) {
    out = nullptr;
    auto it = glyphs_.find(cp);
    if (it == glyphs_.end()) {
        if (!from_bytes_) {
            err = "text: the font has no glyph for " + name_of(cp);
            return PVQ_ERR_INVALID_ARG;
        }
        TextGlyph g;
        if (pvq_status s = read_glyph(cp, g, err)) return s;
        it = glyphs_.emplace(cp, std::move(g)).first;
    }
    out = &it->second;
    return PVQ_OK;
}

// ---- layout and flattening ------------------------------------------------------------------------------------------------------
namespace {
// one contour, already in output pixels (doubles), to chords: lines as they are, a quadratic p0 p1 p2 cut into
// n = ceil(sqrt(|p0 - 2 p1 + p2| / (4 tol))) pieces of equal parameter
// false: more chords than a label may have
bool flatten_contour(const std::vector<Pt>& pts, const std::vector<uint8_t>& on, std::vector<Pt>& poly) {
    poly.clear();
    const size_t m = pts.size();
    if (m < 2) return true;
    std::vector<Pt> p;          // with the implied on-curve points
    std::vector<uint8_t> o;
    for (size_t k = 0; k < m; ++k) {
        const size_t nx = (k + 1) % m;
        p.push_back(pts[k]);
        o.push_back(on[k]);
        if (!on[k] && !on[nx]) {
            p.push_back(Pt{0.5 * (pts[k].x + pts[nx].x), 0.5 * (pts[k].y + pts[nx].y)});
            o.push_back(1);
        }
    }
    size_t start = 0;
    while (start < p.size() && !o[start]) ++start;
    if (start == p.size()) return true;   // unreachable with m >= 2: two off-curve points imply an on-curve one
    const size_t q = p.size();
    poly.push_back(p[start]);
    for (size_t k = 1; k <= q;) {
        const Pt& a = p[(start + k) % q];
        if (o[(start + k) % q]) {
            poly.push_back(a);
            k += 1;
            continue;
        }
        const Pt p0 = poly.back(), p2 = p[(start + k + 1) % q];   // an off-curve point is followed by an on-curve one
        const double dd = std::hypot(p0.x - 2.0 * a.x + p2.x, p0.y - 2.0 * a.y + p2.y);
        const double pieces = std::ceil(std::sqrt(dd / (4.0 * text::FLATTEN_TOL)));
        const uint32_t n = pieces >= 1.0 ? static_cast<uint32_t>(std::min(pieces, 4096.0)) : 1u;
        for (uint32_t c = 1; c < n; ++c) {
            const double t = static_cast<double>(c) / n, u = 1.0 - t;
            poly.push_back(Pt{u * u * p0.x + 2.0 * u * t * a.x + t * t * p2.x, u * u * p0.y + 2.0 * u * t * a.y + t * t * p2.y});
        }
        poly.push_back(p2);
        k += 2;
        if (poly.size() > text::MAX_SEGMENTS + 1u) return false;
    }
    return true;
}
}  // namespace

bool text_contour_chords(const TextGlyph& g, uint32_t first, uint32_t last, const TextMap& map, std::vector<TextPoint>& poly) {
    std::vector<Pt> contour;
    std::vector<uint8_t> on;
    for (uint32_t q = first; q <= last; ++q) {
        contour.push_back(map(g.points[2 * q], g.points[2 * q + 1]));
        on.push_back(g.on_curve[q]);
    }
    return flatten_contour(contour, on, poly);
}

pvq_status text_plan(const char* who, TextFont& font, const pvq_text_label* labels, uint32_t n, uint32_t W, uint32_t H, float vh,
                     std::vector<TextLabelPlan>& out, std::string& err) {
    out.clear();
    if (!labels || n == 0 || n > text::MAX_LABELS) {
        err = std::string(who) + ": 1 .. 64 labels are needed";
        return PVQ_ERR_INVALID_ARG;
    }
    const double s = static_cast<double>(vh / static_cast<float>(H));   // raster::pixel_world's world units per pixel
    const double upem = font.units_per_em();
    out.resize(n);
    std::vector<Pt> poly;
    for (uint32_t l = 0; l < n; ++l) {
        const pvq_text_label& lab = labels[l];
        TextLabelPlan& plan = out[l];
        const std::string tag = std::string(who) + ": label " + std::to_string(l);
        const float numbers[] = {lab.x, lab.y, lab.font_px, lab.scale, lab.rgb[0], lab.rgb[1], lab.rgb[2]};
        for (float v : numbers)
            if (!raster::finite_f(v)) {
                err = tag + ": x, y, font_px, scale and rgb are finite";
                return PVQ_ERR_INVALID_ARG;
            }
        if (!(lab.font_px > 0.0f) || !(lab.scale > 0.0f)) {
            err = tag + ": font_px and scale are positive";
            return PVQ_ERR_INVALID_ARG;
        }
        for (int c = 0; c < 3; ++c)
            if (lab.rgb[c] < 0.0f || lab.rgb[c] > 1.0f) {
                err = tag + ": rgb is sRGB in 0 .. 1";
                return PVQ_ERR_INVALID_ARG;
            }
        const double em_px = static_cast<double>(lab.font_px) * lab.scale / s;
        if (!(em_px <= text::MAX_EM_PIXELS)) {
            err = tag + ": an em is at most 1024 output pixels";
            return PVQ_ERR_INVALID_ARG;
        }
        // the codepoints
        const unsigned char* t = reinterpret_cast<const unsigned char*>(lab.text);
        const unsigned char* end = t + sizeof(lab.text);
        const unsigned char* stop = static_cast<const unsigned char*>(std::memchr(t, 0, sizeof(lab.text)));
        uint32_t cps[text::MAX_CODEPOINTS], n_cp = 0;
        if (stop) end = stop;
        while (stop && t < end) {
            uint32_t cp;
            if (n_cp == text::MAX_CODEPOINTS || !next_codepoint(t, end, cp)) {
                n_cp = 0;
                break;
            }
            cps[n_cp++] = cp;
        }
        if (n_cp == 0) {
            err = tag + ": text is NUL-terminated UTF-8 of 1 .. 8 codepoints";
            return PVQ_ERR_INVALID_ARG;
        }
        const TextGlyph* glyphs[text::MAX_CODEPOINTS];
        double advance_units = 0.0;
        for (uint32_t k = 0; k < n_cp; ++k) {
            if (pvq_status st = font.glyph(cps[k], glyphs[k], err)) return st;
            advance_units += glyphs[k]->advance;
        }
        for (int c = 0; c < 3; ++c) plan.linear_rgb[c] = scene::srgb_to_linear(lab.rgb[c]);
        // the rule of pvq.h: font pixels (y downwards) about the label's position, then world, then output pixels
        const double k_px = static_cast<double>(lab.font_px) / upem;
        const double width = advance_units * k_px, line = static_cast<double>(text::LINE_HEIGHT) * lab.font_px;
        const double asc = font.ascent() * k_px, desc = font.descent() * k_px;
        const double left = -0.5 * width, top = -0.5 * line, baseline = top + 0.5 * (line - (asc - desc)) + asc;
        const auto to_pixel = [&](double fx, double fy_down) {
            const double wx = lab.x + fx * lab.scale, wy = lab.y - fy_down * lab.scale;
            return Pt{wx / s + 0.5 * W, 0.5 * H - wy / s};
        };
        double pen = 0.0;
        const TextMap glyph_to_pixel = [&](double gx, double gy) { return to_pixel(left + pen + gx * k_px, baseline - gy * k_px); };
        const Pt origin = to_pixel(left, baseline);
        plan.origin_x = static_cast<float>(origin.x);
        plan.baseline_y = static_cast<float>(origin.y);
        double lo_x = 1e300, lo_y = 1e300, hi_x = -1e300, hi_y = -1e300;
        std::vector<text::Segment> segs;
        for (uint32_t k = 0; k < n_cp; ++k) {
            const TextGlyph& g = *glyphs[k];
            uint32_t first = 0;
            for (uint32_t e : g.contour_ends) {
                const bool fits = text_contour_chords(g, first, e, glyph_to_pixel, poly);
                first = e + 1;
                if (!fits || segs.size() + poly.size() > text::MAX_SEGMENTS + 1u) {
                    err = tag + ": its outline takes more than 65536 line segments";
                    return PVQ_ERR_INVALID_ARG;
                }
                for (size_t q = 0; q + 1 < poly.size(); ++q) {
                    const text::Segment sg{static_cast<float>(poly[q].x), static_cast<float>(poly[q].y), static_cast<float>(poly[q + 1].x),
                                           static_cast<float>(poly[q + 1].y)};
                    lo_x = std::min({lo_x, static_cast<double>(sg.x0), static_cast<double>(sg.x1)});
                    hi_x = std::max({hi_x, static_cast<double>(sg.x0), static_cast<double>(sg.x1)});
                    lo_y = std::min({lo_y, static_cast<double>(sg.y0), static_cast<double>(sg.y1)});
                    hi_y = std::max({hi_y, static_cast<double>(sg.y0), static_cast<double>(sg.y1)});
                    if (sg.y0 == sg.y1) continue;                                             // contributes nothing
                    if (std::max(sg.y0, sg.y1) <= 0.0f || std::min(sg.y0, sg.y1) >= static_cast<float>(H)) continue;   // meets no pixel row
                    if (std::max(sg.x0, sg.x1) <= 0.0f) continue;                             // left of every pixel: 0 everywhere
                    segs.push_back(sg);
                }
            }
            pen += g.advance * k_px;
        }
        // the pixel box: every pixel square that the outline's bounding box meets with positive area
        if (!(lo_x < hi_x && lo_y < hi_y) || !(hi_x > 0.0 && hi_y > 0.0 && lo_x < W && lo_y < H) || segs.empty()) continue;
        plan.on_image = true;
        plan.x0 = static_cast<uint32_t>(std::max(std::floor(lo_x), 0.0));
        plan.y0 = static_cast<uint32_t>(std::max(std::floor(lo_y), 0.0));
        plan.x1 = static_cast<uint32_t>(std::min(std::ceil(hi_x), static_cast<double>(W)) - 1.0);
        plan.y1 = static_cast<uint32_t>(std::min(std::ceil(hi_y), static_cast<double>(H)) - 1.0);
        plan.segments = std::move(segs);
    }
    return PVQ_OK;
}

void text_frame(const std::vector<TextLabelPlan>& plans, uint32_t W, uint32_t H, float* image, float* coverage) {
    if (coverage) std::fill_n(coverage, plans.size() * W * H, 0.0f);
    for (size_t l = 0; l < plans.size(); ++l) {
        const TextLabelPlan& p = plans[l];
        if (!p.on_image) continue;
        for (uint32_t j = p.y0; j <= p.y1; ++j)
            for (uint32_t i = p.x0; i <= p.x1; ++i) {
                const float c = text_coverage_at(p, i, j);
                if (c == 0.0f) continue;
                const size_t at = static_cast<size_t>(j) * W + i;
                if (coverage) coverage[l * W * H + at] = c;
                if (image) text::blend_label(p.linear_rgb, c, image + 4 * at);
            }
    }
}

void text_pitch_labels(uint32_t octaves, const float* colors, pvq_text_label* out12) {
    const float(*pal)[3] = colors ? reinterpret_cast<const float(*)[3]>(colors) : DEFAULT_COLORS;
    for (uint32_t idx = 0; idx < 12; ++idx) {
        float x, y;
        scene::bin_to_spiral(12, static_cast<float>(12u * octaves - 12u + idx), x, y);   // util.rs:3-7, the last twelve
        const float f = 0.85f + 0.025f * std::fabs(x);                                    // setup.rs:405
        const uint32_t pitch = (idx + 12 - 3) % 12;                                        // setup.rs:402
        pvq_text_label& o = out12[idx];
        std::memset(&o, 0, sizeof(o));
        std::strcpy(o.text, PITCH_NAMES[pitch]);
        o.x = x * f;
        o.y = y * f;
        o.font_px = 40.0f;   // setup.rs:394
        o.scale = 0.02f;     // setup.rs:412
        for (int c = 0; c < 3; ++c) o.rgb[c] = pal[pitch][c];
    }
}

}  // namespace pvq
