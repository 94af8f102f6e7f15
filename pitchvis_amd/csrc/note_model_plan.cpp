// note_model_plan.cpp — see note_model_plan.hpp
#include "note_model_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pvq {

pvq_status note_model_check(const pvq_note_model_params* p, const pvq_note_model_weights* w, NoteModelDims& d, std::string& err) {
    if (!p || !w) {
        err = "note model: null params or weights";
        return PVQ_ERR_INVALID_ARG;
    }
    if (p->n_bins == 0 || p->t_frames == 0 || p->mlp_size == 0) {
        err = "note model: n_bins, t_frames and mlp_size must be positive";
        return PVQ_ERR_INVALID_ARG;
    }
    if (p->mlp_size % 16 != 0) {
        err = "note model: mlp_size must be a multiple of 16";
        return PVQ_ERR_INVALID_ARG;
    }
    if (p->n_bins < 3 || p->n_bins > 1024) {
        err = "unsupported: the note model takes 3 .. 1024 bins";
        return PVQ_ERR_UNSUPPORTED;
    }
    if (p->t_frames > 8 || p->t_frames * p->n_bins < 8) {
        err = "unsupported: the note model takes windows of 1 .. 8 frames and at least 8 values";
        return PVQ_ERR_UNSUPPORTED;
    }
    if (p->mlp_size > 4096) {
        err = "unsupported: the note model takes an mlp_size of 16 .. 4096";
        return PVQ_ERR_UNSUPPORTED;
    }
    if (p->mlp_layers > 8) {
        err = "unsupported: the note model takes 0 .. 8 hidden layers";
        return PVQ_ERR_UNSUPPORTED;
    }
    bool null_w = !w->conv_weight || !w->conv_bias || !w->fc1_weight || !w->fc1_bias || !w->output_weight || !w->output_bias;
    if (p->mlp_layers && (!w->layer_weight || !w->layer_bias)) null_w = true;
    for (uint32_t i = 0; !null_w && i < p->mlp_layers; ++i) null_w = !w->layer_weight[i] || !w->layer_bias[i];
    if (null_w) {
        err = "note model: a weight pointer is null";
        return PVQ_ERR_INVALID_ARG;
    }
    d.n_bins = p->n_bins;
    d.t_frames = p->t_frames;
    d.mlp = p->mlp_size;
    d.layers = p->mlp_layers;
    d.L = p->t_frames * p->n_bins;
    d.o_conv = (d.L - NM_KW) / 2 + 1;
    d.o_pool = d.o_conv / 2;
    d.n_features = NM_CH * d.o_pool;
    return PVQ_OK;
}

std::vector<float> note_model_pack_b(const float* W, uint32_t n, uint32_t k, bool conv_order, uint32_t o_pool) {
    const uint32_t n_ct = (n + NM_BN - 1) / NM_BN;
    const uint32_t chunks = k / NM_KC;   // k is a multiple of 16 in both orders
    const uint32_t chunks_padded = note_model_stages(chunks) * NM_PC;
    std::vector<float> out(static_cast<size_t>(n_ct) * chunks_padded * NM_BN * NM_KC, 0.0f);
    for (uint32_t ct = 0; ct < n_ct; ++ct)
        for (uint32_t kc = 0; kc < chunks; ++kc) {
            float* dst = out.data() + (static_cast<size_t>(ct) * chunks_padded + kc) * NM_BN * NM_KC;
            for (uint32_t s = 0; s < 4; ++s)
                for (uint32_t l = 0; l < 64; ++l) {
                    const uint32_t col = NM_BN * ct + 16 * s + (l & 15);
                    if (col >= n) continue;
                    for (uint32_t i = 0; i < 4; ++i) {
                        const uint32_t kk = 4 * (l >> 4) + i;   // position in the chunk; in conv order the channel
                        const size_t src = conv_order ? static_cast<size_t>(kk) * o_pool + kc : static_cast<size_t>(NM_KC) * kc + kk;
                        dst[(s * 64 + l) * 4 + i] = W[static_cast<size_t>(col) * k + src];
                    }
                }
        }
    return out;
}

std::vector<NmTile> note_model_tiles(const NoteModelDims& d, const size_t* n_frames, uint32_t n_streams, size_t stride_frames) {
    std::vector<NmTile> tiles;
    for (uint32_t s = 0; s < n_streams; ++s) {
        const size_t nf = n_frames ? n_frames[s] : stride_frames;
        for (size_t f0 = d.t_frames - 1; f0 < nf; f0 += NM_BM)
            tiles.push_back(NmTile{s, static_cast<uint32_t>(f0), static_cast<uint32_t>(std::min<size_t>(NM_BM, nf - f0)), 0u});
    }
    return tiles;
}

pvq_status note_carry_plan(const NoteModelDims& d, const uint64_t* seen, const size_t* n_frames, uint32_t n_streams, size_t stride_frames,
                           NcPlan& out, std::string& err) {
    out.streams.resize(n_streams);
    out.total_rows = out.tiles = 0;
    out.max_rows = out.max_n = 0;
    const uint64_t lead = d.t_frames - 1u;   // frames a stream needs before its first model row
    for (uint32_t s = 0; s < n_streams; ++s) {
        const uint64_t n = n_frames ? n_frames[s] : stride_frames;
        const uint64_t missing = seen[s] < lead ? lead - seen[s] : 0u;
        const uint64_t f_first = std::min(missing, n);
        NcStream& st = out.streams[s];
        st.first_row = static_cast<uint32_t>(out.total_rows);
        st.f_first = static_cast<uint32_t>(f_first);
        st.rows = static_cast<uint32_t>(n - f_first);
        st.head = static_cast<uint32_t>(std::min(n, lead) - std::min(f_first, lead));
        st.n = static_cast<uint32_t>(n);
        st.pad[0] = st.pad[1] = st.pad[2] = 0u;
        out.total_rows += st.rows;
        out.max_rows = std::max(out.max_rows, st.rows);
        out.max_n = std::max(out.max_n, st.n);
        if (out.total_rows > 0x7fffffffull) {
            err = "note carry: too many model rows in one call";
            return PVQ_ERR_INVALID_ARG;
        }
    }
    out.tiles = (out.total_rows + NM_BM - 1) / NM_BM;
    return PVQ_OK;
}

namespace {
uint32_t f32_bits(float x) {
    uint32_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}
float bits_f32(uint32_t u) {
    float x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}
}  // namespace

float note_round(pvq_note_precision prec, float x) {
    if (prec == PVQ_NOTE_F32 || x != x) return x;
    const uint32_t u = f32_bits(x);
    if (prec == PVQ_NOTE_BF16) return bits_f32((u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u);   // (a carry out of the largest finite value is infinity)
    const uint32_t sign = u & 0x80000000u;
    uint32_t a = u & 0x7fffffffu;
    if (a >= 0x477ff000u) return bits_f32(sign | 0x7f800000u);   // 65520 = 65504 + half a step, and above (infinity included)
    if (a < 0x38800000u) {   // below 2^-14: a multiple of 2^-24, the step of the f32 values in [0.5, 1)
        volatile float t = bits_f32(a) + 0.5f;   // (the addition rounds to nearest even; volatile: it is not folded away)
        return bits_f32(sign | f32_bits(t - 0.5f));
    }
    a = (a + 0xfffu + ((a >> 13) & 1u)) & ~0x1fffu;
    return bits_f32(sign | a);
}

uint16_t note_bits16(pvq_note_precision prec, float rounded) {
    const uint32_t u = f32_bits(rounded);
    if (prec != PVQ_NOTE_F16) return static_cast<uint16_t>(u >> 16);
    const uint16_t sign = static_cast<uint16_t>((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;
    if (a >= 0x47800000u) return sign | 0x7c00u;
    if (a < 0x38800000u) return sign | static_cast<uint16_t>(bits_f32(a) * 16777216.0f);   // the multiple of 2^-24 is the mantissa
    return sign | static_cast<uint16_t>((a - 0x38000000u) >> 13);
}

pvq_status note_model_check_range(const NoteModelDims& d, const pvq_note_model_weights& w, pvq_note_precision prec, std::string& err) {
    if (prec != PVQ_NOTE_F16) return PVQ_OK;
    auto beyond = [](const float* p, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (std::fabs(p[i]) > 65504.0f) return true;   // (NaN compares false: it stays NaN)
        return false;
    };
    std::string layer;
    if (beyond(w.fc1_weight, static_cast<size_t>(d.mlp) * d.n_features)) layer = "fc1.weight";
    for (uint32_t i = 0; layer.empty() && i < d.layers; ++i)
        if (beyond(w.layer_weight[i], static_cast<size_t>(d.mlp) * d.mlp)) layer = "layers." + std::to_string(i) + ".weight";
    if (layer.empty() && beyond(w.output_weight, static_cast<size_t>(NM_OUT) * d.mlp)) layer = "output.weight";
    if (layer.empty()) return PVQ_OK;
    err = "note model: " + layer + " holds a value beyond the f16 range (+-65504)";
    return PVQ_ERR_INVALID_ARG;
}

std::vector<uint16_t> note_model_pack_b16(const float* W, uint32_t n, uint32_t k, bool conv_order, uint32_t o_pool, pvq_note_precision prec) {
    const uint32_t n_ct = (n + NM_BN - 1) / NM_BN;
    const uint32_t chunks = note_model_pad32(k) / NM_KC16;
    const uint32_t chunks_padded = note_model_stages16(k) * NM_PC;
    std::vector<uint16_t> out(static_cast<size_t>(n_ct) * chunks_padded * NM_BN * NM_KC16, 0);
    for (uint32_t ct = 0; ct < n_ct; ++ct)
        for (uint32_t kc = 0; kc < chunks; ++kc) {
            uint16_t* dst = out.data() + (static_cast<size_t>(ct) * chunks_padded + kc) * NM_BN * NM_KC16;
            for (uint32_t s = 0; s < 4; ++s)
                for (uint32_t l = 0; l < 64; ++l) {
                    const uint32_t col = NM_BN * ct + 16 * ((l & 15) >> 2) + 4 * s + (l & 3);
                    if (col >= n) continue;
                    for (uint32_t j = 0; j < 8; ++j) {
                        const uint32_t kk = NM_KC16 * kc + 8 * (l >> 4) + j;   // k'; in conv order 16 p + c
                        if (kk >= k) continue;                                  // the padded half chunk
                        const size_t src = conv_order ? static_cast<size_t>(kk % NM_CH) * o_pool + kk / NM_CH : kk;
                        dst[(s * 64 + l) * 8 + j] = note_bits16(prec, note_round(prec, W[static_cast<size_t>(col) * k + src]));
                    }
                }
        }
    return out;
}

NmWorkspace note_model_workspace(const NoteModelDims& d, pvq_note_precision precision, size_t n_tiles, uint64_t limit) {
    NmWorkspace w;
    const bool half = precision != PVQ_NOTE_F32;
    if (half) {
        w.kf_pad = note_model_pad32(d.n_features);
        w.mlp_pad = note_model_pad32(d.mlp);
    }
    const size_t row_bytes = half ? 2 * static_cast<size_t>(w.mlp_pad) : sizeof(float) * static_cast<size_t>(d.mlp);   // of a hidden buffer
    const size_t feat_bytes = 2 * static_cast<size_t>(w.kf_pad);                                                       // of the features: 16-bit only
    w.tab_bytes = (n_tiles * sizeof(NmTile) + 255) & ~static_cast<size_t>(255);
    w.tile_bytes = static_cast<size_t>(NM_BM) * (feat_bytes + 2 * row_bytes);
    // a launch's grid: the features kernel has a block per row and 64 pooled positions, a dense kernel one per tile and column tile
    const size_t per_tile = std::max<size_t>({static_cast<size_t>(NM_BM) * ((w.kf_pad / NM_CH + 63) / 64), (d.mlp + NM_BN - 1) / NM_BN, NM_OUT / NM_BN});
    const size_t fit = limit > w.tab_bytes ? static_cast<size_t>((limit - w.tab_bytes) / w.tile_bytes) : 0;
    w.chunk_tiles = std::max<size_t>(1, std::min<size_t>({fit, n_tiles, 0x7fffffffull / per_tile}));
    if (half) w.feat_at = w.tab_bytes;
    w.h_at[0] = w.tab_bytes + w.chunk_tiles * NM_BM * feat_bytes;
    w.h_at[1] = w.h_at[0] + w.chunk_tiles * NM_BM * row_bytes;
    w.total = w.tab_bytes + w.chunk_tiles * w.tile_bytes;
    return w;
}

void NoteModelHost::assign(const NoteModelDims& dims, const pvq_note_model_weights& w, pvq_note_precision prec) {
    d = dims;
    precision = prec;
    conv_w.assign(w.conv_weight, w.conv_weight + NM_CH * NM_KW);
    conv_b.assign(w.conv_bias, w.conv_bias + NM_CH);
    fc1_w.assign(w.fc1_weight, w.fc1_weight + static_cast<size_t>(d.mlp) * d.n_features);
    fc1_b.assign(w.fc1_bias, w.fc1_bias + d.mlp);
    layer_w.resize(d.layers);
    layer_b.resize(d.layers);
    for (uint32_t i = 0; i < d.layers; ++i) {
        layer_w[i].assign(w.layer_weight[i], w.layer_weight[i] + static_cast<size_t>(d.mlp) * d.mlp);
        layer_b[i].assign(w.layer_bias[i], w.layer_bias[i] + d.mlp);
    }
    out_w.assign(w.output_weight, w.output_weight + static_cast<size_t>(NM_OUT) * d.mlp);
    out_b.assign(w.output_bias, w.output_bias + NM_OUT);
    if (precision != PVQ_NOTE_F32) {   // every dense weight is rounded once, here
        for (float& v : fc1_w) v = note_round(precision, v);
        for (std::vector<float>& lw : layer_w)
            for (float& v : lw) v = note_round(precision, v);
        for (float& v : out_w) v = note_round(precision, v);
    }
}

namespace {
void linear(const float* W, const float* b, const float* x, uint32_t n, uint32_t k, bool relu, float* y) {
    for (uint32_t j = 0; j < n; ++j) {
        const float* row = W + static_cast<size_t>(j) * k;
        float acc = 0.0f;
        for (uint32_t i = 0; i < k; ++i) acc += row[i] * x[i];
        acc += b[j];
        y[j] = relu ? std::max(acc, 0.0f) : acc;
    }
}
}  // namespace

void NoteModelHost::infer(const float* window, float* out_prob) const {
    std::vector<float> feat(d.n_features), h(d.mlp), h2(d.mlp);
    if (precision != PVQ_NOTE_F32) {
        for (int c = 0; c < NM_CH; ++c)
            for (uint32_t p = 0; p < d.o_pool; ++p) {
                float e = conv_b[c], o = conv_b[c];   // the kernels' chain: from the bias, one fmaf per tap
                for (int i = 0; i < NM_KW; ++i) {
                    e = std::fmaf(conv_w[c * NM_KW + i], window[4 * p + i], e);
                    o = std::fmaf(conv_w[c * NM_KW + i], window[4 * p + 2 + i], o);
                }
                feat[static_cast<size_t>(c) * d.o_pool + p] = note_round(precision, std::max(std::max(e, o), 0.0f));
            }
        linear(fc1_w.data(), fc1_b.data(), feat.data(), d.mlp, d.n_features, true, h.data());
        for (uint32_t i = 0; i <= d.layers; ++i) {
            for (float& v : h) v = note_round(precision, v);   // a hidden activation as it is stored
            if (i == d.layers) break;
            linear(layer_w[i].data(), layer_b[i].data(), h.data(), d.mlp, d.mlp, true, h2.data());
            h.swap(h2);
        }
        float logit[NM_OUT];
        linear(out_w.data(), out_b.data(), h.data(), NM_OUT, d.mlp, false, logit);
        for (int j = 0; j < NM_OUT; ++j) out_prob[j] = 1.0f / (1.0f + std::exp(-logit[j]));
        return;
    }
    for (int c = 0; c < NM_CH; ++c)
        for (uint32_t p = 0; p < d.o_pool; ++p) {
            float best = 0.0f;   // ReLU, then the pool's maximum over conv positions 2p and 2p + 1 (train.py:89-90)
            for (uint32_t j = 2 * p; j < 2 * p + 2; ++j) {
                float acc = 0.0f;
                for (int i = 0; i < NM_KW; ++i) acc += conv_w[c * NM_KW + i] * window[2 * j + i];
                best = std::max(best, acc + conv_b[c]);
            }
            feat[static_cast<size_t>(c) * d.o_pool + p] = best;
        }
    linear(fc1_w.data(), fc1_b.data(), feat.data(), d.mlp, d.n_features, true, h.data());
    for (uint32_t i = 0; i < d.layers; ++i) {
        linear(layer_w[i].data(), layer_b[i].data(), h.data(), d.mlp, d.mlp, true, h2.data());
        h.swap(h2);
    }
    float logit[NM_OUT];
    linear(out_w.data(), out_b.data(), h.data(), NM_OUT, d.mlp, false, logit);
    for (int j = 0; j < NM_OUT; ++j) out_prob[j] = 1.0f / (1.0f + std::exp(-logit[j]));
}

}  // namespace pvq
