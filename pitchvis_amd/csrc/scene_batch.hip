// scene_batch.hip — the pitch-ball scene for many streams (scene_batch.hpp), split by what recurs.
//
// scene_peaks (frame-parallel, a wavefront per (stream, frame) row, a lane per peak): util::arg_max of the row's sizes, then
// scene::peak_record for every entry of the list — colour, spiral position, alpha, z, scale, the three params, key bin, hide range
// (update.rs:199-302, :310-315) — and, once per row, the bloom and the bass spiral's (lit count, colour) (update.rs:336-425).  None
// of it reads the scene's state, and all the libm of a frame sits here.  The records go to a workspace of the handle.  With a
// probability buffer (the note model's d_prob, its own frame stride) a record's alpha follows the `ml` branch (update.rs:247-255).
//
// scene_frames<NK> (a wavefront per stream, frames in order; lane l owns bins l, l + 64, ...; NK: the bin count's 64-chunk): what
// recurs.  Per bin the fade (update.rs:151-177: two multiplies, a max, a subtract, two compares), then the frame's records are
// applied.  The reference's HashMap ("the later entry of a key wins", update.rs:208-212) and the OR of the hide ranges of the map's
// entries (update.rs:307-330) are resolved per bin through LDS: every peak enters 1 + its list index into its key bin with an LDS
// max — peaks go through in chunks of 64 in list order, any max_peaks works — then the entries that survived hand their record to
// their ball and mark their hide range, and the lane that owns a bin shows or hides it.
// A stream's whole state sits in LDS for the call (60 bytes a bin with the tables: 15 KiB at the benchmark's 252 bins, 60 KiB at
// 1024), not in registers: the peaks address balls by key, which registers cannot be, and sixteen chunks of eleven fields in
// registers left the 1024-bin instantiation spilling.  The fade's LDS traffic (7 dwords a bin and frame) is small beside the 11
// dwords a bin and frame that go out to memory.
//
// fade_pitch_balls' powf depends on (bin, frame time) alone: the host builds dropoff per bin and the z step with its own libm
// (scene_fade_table) once per distinct frame time of a call, so the fade carries the host's bits.  FMA contraction is off and `/`
// is the correctly rounded division, as in render_batch.hip.
#include "scene_batch.hpp"

#include <algorithm>
#include <cstring>
#include <string>

#include "stage_device.hpp"
#include "stage_plan.hpp"
#include "vqt_engine.hpp"

namespace pvq {

namespace {
constexpr uint32_t MAX_BINS = 1024;
constexpr int STATE_FIELDS = 12;   // x y z scale r g b a calmness accuracy deviation visible(u32)
enum { SX, SY, SZ, SSCALE, SR, SG, SB, SA, SPC, SPA, SPD, SVIS };
constexpr size_t WORKSPACE_LIMIT = 256ull << 20;   // records of one piece of a call

struct RowHeader {   // what a frame with peaks makes of bloom and bass spiral
    uint32_t bass_lit;
    float bass_rgba[4];
    float bloom;
    uint32_t pad[2];
};
static_assert(sizeof(scene::PeakRecord) == 64 && sizeof(RowHeader) == 32, "workspace layout");

struct SceneArgs {
    const float* center;
    const float* size;
    const uint32_t* peak_count;
    const float* calmness;
    const float* accuracy;
    const float* deviation;
    const float* scene_calmness;
    const float* ml_prob;             // [n_streams][ml_stride][128] or null: no `ml` branch
    size_t ml_stride;
    uint32_t max_peaks, n_streams;
    uint32_t n_frames, f0, pf;        // the call's frames; this piece is frames f0 .. f0 + pf
    int n_bins;
    const scene::Settings* settings;
    scene::PeakRecord* rec;           // [n_streams * pf][max_peaks]
    RowHeader* hdr;                   // [n_streams * pf]
    const float* fade;                // [rows][n_bins + 1]
    const uint32_t* fade_row;         // [n_frames] or null: row 0
    float* state;                     // [n_streams][STATE_FIELDS][n_bins]
    float* scalars;                   // [n_streams][8]
    float* out_xyzs;
    float* out_rgba;
    float* out_params;
    uint32_t* out_visible;
    uint32_t* out_bass_lit;
    float* out_bass_rgba;
    float* out_bloom;
};

__global__ __launch_bounds__(64) __attribute__((flatten)) void scene_peaks(SceneArgs a) {   // (flatten: the colour routines' small arrays stay in registers)
#pragma clang fp contract(off)
    __shared__ scene::Settings s_set;
    const int lane = threadIdx.x;
    for (int i = lane; i < static_cast<int>(sizeof(scene::Settings) / 4); i += 64)
        reinterpret_cast<uint32_t*>(&s_set)[i] = reinterpret_cast<const uint32_t*>(a.settings)[i];
    __syncthreads();
    const uint32_t rows = a.n_streams * a.pf;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const size_t g = stage::piece_row(r, a.pf, a.n_frames, a.f0);
        const uint32_t cnt = min(a.peak_count[g], a.max_peaks);
        if (cnt == 0u) continue;   // update.rs:85-87: scene_frames never reads this row's records or header
        const float* c_row = a.center + g * a.max_peaks;
        const float* z_row = a.size + g * a.max_peaks;
        // util::arg_max (util.rs:48-57): the FIRST maximum.  Its value is all that is used, but with both signs of zero in the list
        // the first one's sign is the value: every lane carries (value, list index) and ends with the same pair
        float best = scene::F32_MIN;
        uint32_t best_at = 0xFFFFFFFFu;
        for (uint32_t p = lane; p < cnt; p += 64) {
            const float v = z_row[p];
            if (v > best) {
                best = v;
                best_at = p;
            }
        }
        for (int o = 32; o; o >>= 1) {
            const float other = __shfl_xor(best, o);
            const uint32_t other_at = __shfl_xor(best_at, o);
            if (other > best || (!(other < best) && other_at < best_at)) {   // (a NaN never gets into `best`)
                best = other;
                best_at = other_at;
            }
        }
        const float max_size = best > scene::F32_MIN ? best : z_row[0];
        const size_t bins = g * static_cast<size_t>(a.n_bins);
        // the row's probabilities: stream r / pf, frame f0 + r % pf of a buffer with its own frame stride (so not row g)
        const float* ml = a.ml_prob ? a.ml_prob + (static_cast<size_t>(r / a.pf) * a.ml_stride + a.f0 + r % a.pf) * scene::MIDI_PITCHES : nullptr;
        for (uint32_t p = lane; p < cnt; p += 64) {
            scene::PeakRecord q;
            scene::peak_record(s_set, c_row[p], z_row[p], max_size, a.calmness + bins, a.accuracy + bins, a.deviation + bins, q, ml);
            uint4* dst = reinterpret_cast<uint4*>(a.rec + static_cast<size_t>(r) * a.max_peaks + p);
            dst[0] = make_uint4(__float_as_uint(q.x), __float_as_uint(q.y), __float_as_uint(q.z), __float_as_uint(q.scale));
            dst[1] = make_uint4(__float_as_uint(q.r), __float_as_uint(q.g), __float_as_uint(q.b), __float_as_uint(q.a));
            dst[2] = make_uint4(__float_as_uint(q.calmness), __float_as_uint(q.accuracy), __float_as_uint(q.deviation), q.key);
            dst[3] = make_uint4(q.lo, q.hi, q.shows, 0u);
        }
        if (lane == 0) {
            float rgba[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const uint32_t lit = scene::bass_of(s_set, c_row[0], z_row[0], max_size, rgba);
            uint4* dst = reinterpret_cast<uint4*>(a.hdr + r);
            dst[0] = make_uint4(lit, __float_as_uint(rgba[0]), __float_as_uint(rgba[1]), __float_as_uint(rgba[2]));
            dst[1] = make_uint4(__float_as_uint(rgba[3]), __float_as_uint(scene::bloom_of(s_set, a.scene_calmness[g])), 0u, 0u);
        }
    }
}

template <int NK>   // 64 (NK - 1) < n_bins <= 64 NK (the host's promise): an instantiation's LDS is its chunk count's
__global__ __launch_bounds__(64) void scene_frames(SceneArgs a) {
#pragma clang fp contract(off)
    constexpr int NB = 64 * NK;
    __builtin_assume(a.n_bins > 64 * (NK - 1) && a.n_bins <= NB);
    __shared__ float s_f[SVIS][NB];     // the eleven float fields of every ball, in the state's order
    __shared__ uint32_t s_vis[NB];
    __shared__ float s_drop[NB];        // the fade table's row
    __shared__ uint32_t s_own[NB];      // 1 + the list index of the last entry keyed to the bin, 0: none
    __shared__ uint32_t s_hide[NB];     // bit 0: the bin lies in the hide range of an entry that survived; bit 1: its own entry shows

    const int lane = threadIdx.x;
    const int n = a.n_bins;
    const uint32_t s = blockIdx.x;
    float* st = a.state + static_cast<size_t>(s) * STATE_FIELDS * n;
#pragma unroll 1
    for (int fld = 0; fld < SVIS; ++fld)
        for (int bin = lane; bin < n; bin += 64) s_f[fld][bin] = st[fld * n + bin];
    for (int bin = lane; bin < n; bin += 64) s_vis[bin] = __float_as_uint(st[SVIS * n + bin]);
    float* sc = a.scalars + static_cast<size_t>(s) * 8;
    uint32_t bass_lit = __float_as_uint(sc[0]);
    float bass_r = sc[1], bass_g = sc[2], bass_b = sc[3], bass_a = sc[4], bloom = sc[5];
    uint32_t cur_row = 0xFFFFFFFFu;
    float z_step = 0.0f;
    const uint32_t words = (static_cast<uint32_t>(n) + 31u) / 32u;
    __syncthreads();

    for (uint32_t fi = 0; fi < a.pf; ++fi) {
        const uint32_t f = a.f0 + fi;
        const size_t g = static_cast<size_t>(s) * a.n_frames + f;
        const size_t r = static_cast<size_t>(s) * a.pf + fi;
        const uint32_t row = a.fade_row ? a.fade_row[f] : 0u;
        if (row != cur_row) {   // (a lane reads back only what it wrote: bins lane, lane + 64, ...)
            const float* t = a.fade + static_cast<size_t>(row) * (n + 1);
            for (int bin = lane; bin < n; bin += 64) s_drop[bin] = t[bin];
            z_step = t[n];
            cur_row = row;
        }
#pragma unroll 2
        for (int bin = lane; bin < n; bin += 64) {   // update.rs:80: fade_pitch_balls
            float scale = s_f[SSCALE][bin], alpha = s_f[SA][bin], z = s_f[SZ][bin];
            bool v = s_vis[bin] != 0u;
            scene::fade_ball(scale, alpha, z, v, s_drop[bin], z_step);
            s_f[SSCALE][bin] = scale;
            s_f[SA][bin] = alpha;
            s_f[SZ][bin] = z;
            s_vis[bin] = v ? 1u : 0u;
        }
        const uint32_t cnt = min(a.peak_count[g], a.max_peaks);
        if (cnt) {   // update.rs:85-87
            for (int bin = lane; bin < NB; bin += 64) {
                s_own[bin] = 0u;
                s_hide[bin] = 0u;
            }
            __syncthreads();
            const scene::PeakRecord* rec = a.rec + r * a.max_peaks;
            for (uint32_t p = lane; p < cnt; p += 64) {   // update.rs:208-212: HashMap::insert, the later entry of a key stays
                const uint32_t key = rec[p].key;
                if (key < static_cast<uint32_t>(n)) atomicMax(&s_own[key], p + 1u);
            }
            __syncthreads();
            for (uint32_t p = lane; p < cnt; p += 64) {   // the map's entries: a lane per surviving peak hands its record to the ball
                const uint4* q = reinterpret_cast<const uint4*>(rec + p);
                const uint4 q2 = q[2];
                const uint32_t key = q2.w;
                if (key < static_cast<uint32_t>(n) && s_own[key] == p + 1u) {
                    const uint4 q0 = q[0], q1 = q[1], q3 = q[3];
                    s_f[SX][key] = __uint_as_float(q0.x);     // update.rs:216-302
                    s_f[SY][key] = __uint_as_float(q0.y);
                    s_f[SZ][key] = __uint_as_float(q0.z);
                    s_f[SSCALE][key] = __uint_as_float(q0.w);
                    s_f[SR][key] = __uint_as_float(q1.x);
                    s_f[SG][key] = __uint_as_float(q1.y);
                    s_f[SB][key] = __uint_as_float(q1.z);
                    s_f[SA][key] = __uint_as_float(q1.w);
                    s_f[SPC][key] = __uint_as_float(q2.x);
                    s_f[SPA][key] = __uint_as_float(q2.y);
                    s_f[SPD][key] = __uint_as_float(q2.z);
                    if (q3.z) atomicOr(&s_hide[key], 2u);     // update.rs:300-302
                    const uint32_t hi = min(q3.y, static_cast<uint32_t>(n) - 1u);
                    for (uint32_t i = q3.x; i <= hi; ++i) atomicOr(&s_hide[i], 1u);   // update.rs:308-319
                }
            }
            __syncthreads();
            for (int bin = lane; bin < n; bin += 64) {
                const uint32_t h = s_hide[bin];
                if (s_own[bin]) {
                    if (h & 2u) s_vis[bin] = 1u;
                } else if (h & 1u) {
                    s_vis[bin] = 0u;                       // update.rs:320-330
                }
            }
            const uint4* h = reinterpret_cast<const uint4*>(a.hdr + r);
            const uint4 h0 = h[0], h1 = h[1];
            bloom = __uint_as_float(h1.y);                 // update.rs:98
            bass_lit = h0.x;                               // update.rs:369-373, :390-397
            if (bass_lit) {                                // update.rs:418-420: only lit segments take the colour
                bass_r = __uint_as_float(h0.y);
                bass_g = __uint_as_float(h0.z);
                bass_b = __uint_as_float(h0.w);
                bass_a = __uint_as_float(h1.x);
            }
            __syncthreads();   // s_own / s_hide are the next frame's
        }
        if (a.out_xyzs) {
            float4* o = reinterpret_cast<float4*>(a.out_xyzs) + g * n;
            for (int bin = lane; bin < n; bin += 64) o[bin] = make_float4(s_f[SX][bin], s_f[SY][bin], s_f[SZ][bin], s_f[SSCALE][bin]);
        }
        if (a.out_rgba) {
            float4* o = reinterpret_cast<float4*>(a.out_rgba) + g * n;
            for (int bin = lane; bin < n; bin += 64) o[bin] = make_float4(s_f[SR][bin], s_f[SG][bin], s_f[SB][bin], s_f[SA][bin]);
        }
        if (a.out_params) {   // a row is 3 n consecutive floats: lane l writes floats l, l + 64, ... of it
            float* o = a.out_params + g * n * 3;
            for (int i = lane; i < 3 * n; i += 64) {
                const int bin = i / 3;
                o[i] = s_f[SPC + (i - 3 * bin)][bin];
            }
        }
        if (a.out_visible) {
            uint32_t* o = a.out_visible + g * words;
            for (int k = 0; k < NK; ++k) {   // (uniform: every lane takes part in the ballot)
                const int bin = lane + 64 * k;
                const unsigned long long m = __ballot(bin < n && s_vis[bin < n ? bin : 0] != 0u);
                if (lane == 0) {
                    o[2 * k] = static_cast<uint32_t>(m);
                    if (2u * k + 1u < words) o[2 * k + 1] = static_cast<uint32_t>(m >> 32);
                }
            }
        }
        if (lane == 0) {
            if (a.out_bass_lit) a.out_bass_lit[g] = bass_lit;
            if (a.out_bass_rgba) reinterpret_cast<float4*>(a.out_bass_rgba)[g] = make_float4(bass_r, bass_g, bass_b, bass_a);
            if (a.out_bloom) a.out_bloom[g] = bloom;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int fld = 0; fld < SVIS; ++fld)
        for (int bin = lane; bin < n; bin += 64) st[fld * n + bin] = s_f[fld][bin];
    for (int bin = lane; bin < n; bin += 64) st[SVIS * n + bin] = __uint_as_float(s_vis[bin]);
    if (lane == 0) {
        sc[0] = __uint_as_float(bass_lit);
        sc[1] = bass_r;
        sc[2] = bass_g;
        sc[3] = bass_b;
        sc[4] = bass_a;
        sc[5] = bloom;
    }
}

template <int NK>
void launch_nk(int nk, const SceneArgs& a, dim3 grid, hipStream_t stream) {
    if constexpr (NK > 16) {
        return;
    } else {
        if (nk == NK)
            hipLaunchKernelGGL(scene_frames<NK>, grid, dim3(64), 0, stream, a);
        else
            launch_nk<NK + 1>(nk, a, grid, stream);
    }
}
}  // namespace

pvq_status SceneBatch::create(int device_id, uint32_t octaves, uint32_t buckets_per_octave, const pvq_scene_settings* settings,
                              uint32_t n_streams, std::unique_ptr<SceneBatch>& out) {
    out.reset();
    if (octaves == 0 || buckets_per_octave == 0 || n_streams == 0) {
        set_last_error("scene batch: octaves, buckets_per_octave and n_streams must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    const uint64_t n = static_cast<uint64_t>(octaves) * buckets_per_octave;
    if (n < 3 || n > MAX_BINS) {
        set_last_error("unsupported: the batched scene takes 3 .. 1024 bins");
        return PVQ_ERR_UNSUPPORTED;
    }
    std::unique_ptr<SceneBatch> b(new SceneBatch());
    const pvq_scene_settings def{PVQ_VISUALS_FULL, 1, nullptr, 60.0f, 1.3f};
    const pvq_scene_settings& cfg = settings ? *settings : def;
    if (!scene_settings(octaves, buckets_per_octave, cfg.visuals_mode, cfg.enable_bloom, cfg.colors, cfg.gray_level, cfg.easing_pow, b->s_)) {
        set_last_error("scene: unknown visuals mode");
        return PVQ_ERR_INVALID_ARG;
    }
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_streams_ = n_streams;
    if (device_id >= 0) {
        SceneBalls init;
        float bass[4];
        scene_initial(b->s_, init, bass);
        const size_t per = static_cast<size_t>(STATE_FIELDS) * n;
        std::vector<float> one(per);
        const std::vector<float>* src[] = {&init.x, &init.y, &init.z, &init.scale, &init.r, &init.g, &init.b, &init.a,
                                           &init.calmness, &init.accuracy, &init.deviation};
        for (int fld = 0; fld < 11; ++fld) std::copy(src[fld]->begin(), src[fld]->end(), one.begin() + fld * n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t v = init.visible[i];
            std::memcpy(&one[SVIS * n + i], &v, 4);
        }
        std::vector<float> all(per * n_streams), scal(static_cast<size_t>(8) * n_streams, 0.0f);
        for (uint32_t s = 0; s < n_streams; ++s) {
            std::copy(one.begin(), one.end(), all.begin() + s * per);
            for (int i = 0; i < 4; ++i) scal[static_cast<size_t>(8) * s + 1 + i] = bass[i];
        }
        PVQ_HIP(hipSetDevice(device_id));
        if (pvq_status s = b->settings_.upload(&b->s_, sizeof(scene::Settings))) return s;
        if (pvq_status s = b->state_.upload(all.data(), all.size() * sizeof(float))) return s;
        if (pvq_status s = b->scalars_.upload(scal.data(), scal.size() * sizeof(float))) return s;
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status SceneBatch::frames_device(size_t n_frames, const pvq_scene_inputs& in, uint64_t frame_time_ns, const uint64_t* frame_times_ns,
                                     const pvq_scene_outputs& outs, hipStream_t stream, const float* d_ml_prob, size_t ml_stride_frames) {
    if (!in.center || !in.size || !in.peak_count || in.max_peaks == 0) {
        set_last_error("scene batch: center, size and peak_count are needed, with max_peaks > 0");
        return PVQ_ERR_INVALID_ARG;
    }
    if (!in.calmness || !in.pitch_accuracy || !in.pitch_deviation || !in.scene_calmness) {
        set_last_error("scene batch: calmness, pitch_accuracy, pitch_deviation and scene_calmness are needed");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(outs.ball_xyzs) | reinterpret_cast<uintptr_t>(outs.ball_rgba) |
         reinterpret_cast<uintptr_t>(outs.bass_rgba)) & 15) {
        set_last_error("scene batch: ball_xyzs, ball_rgba and bass_rgba must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("scene batch", n_frames, n_streams_, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (d_ml_prob && (ml_stride_frames < n_frames || ml_stride_frames > (~0ull >> 12) / n_streams_)) {
        set_last_error("scene batch: ml_stride_frames must be at least n_frames");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched scene runs on a GPU; this handle has none (pvq_scene_state_* is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_frames == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    const uint32_t n = s_.n_bins;

    // the fade table: one row per distinct frame time of the call, from the host's libm
    std::vector<uint64_t> distinct;
    std::vector<uint32_t> rows;
    if (frame_times_ns) {
        rows.resize(n_frames);
        for (size_t f = 0; f < n_frames; ++f) {
            const auto it = std::find(distinct.begin(), distinct.end(), frame_times_ns[f]);
            rows[f] = static_cast<uint32_t>(it - distinct.begin());
            if (it == distinct.end()) distinct.push_back(frame_times_ns[f]);
        }
    } else {
        distinct.push_back(frame_time_ns);
    }
    if (distinct != fade_times_ || frame_times_ns) PVQ_HIP(hipStreamSynchronize(stream));   // the buffers below may still be read
    if (distinct != fade_times_) {
        std::vector<float> tab(distinct.size() * (n + 1));
        for (size_t r = 0; r < distinct.size(); ++r) scene_fade_table(n, distinct[r], &tab[r * (n + 1)], tab[r * (n + 1) + n]);
        fade_times_.clear();   // until the new table is whole on the device
        if (pvq_status s = fade_.upload(tab.data(), tab.size() * sizeof(float))) return s;
        fade_times_ = distinct;
    }
    if (frame_times_ns)
        if (pvq_status s = fade_row_.upload(rows.data(), n_frames * sizeof(uint32_t))) return s;

    // the records of a piece of the call's frames fit the workspace
    const size_t per_row = static_cast<size_t>(in.max_peaks) * sizeof(scene::PeakRecord) + sizeof(RowHeader);
    const size_t pf = stage_piece_frames(n_frames, n_streams_, per_row, WORKSPACE_LIMIT);
    if (pvq_status s = rec_.reserve(per_row * n_streams_ * pf)) return s;
    SceneArgs a{};
    a.center = in.center;
    a.size = in.size;
    a.peak_count = in.peak_count;
    a.calmness = in.calmness;
    a.accuracy = in.pitch_accuracy;
    a.deviation = in.pitch_deviation;
    a.scene_calmness = in.scene_calmness;
    a.ml_prob = d_ml_prob;
    a.ml_stride = ml_stride_frames;
    a.max_peaks = in.max_peaks;
    a.n_streams = n_streams_;
    a.n_frames = static_cast<uint32_t>(n_frames);
    a.n_bins = static_cast<int>(n);
    a.settings = settings_.as<scene::Settings>();
    a.fade = fade_.as<float>();
    a.fade_row = frame_times_ns ? fade_row_.as<uint32_t>() : nullptr;
    a.state = state_.as<float>();
    a.scalars = scalars_.as<float>();
    a.out_xyzs = outs.ball_xyzs;
    a.out_rgba = outs.ball_rgba;
    a.out_params = outs.ball_params;
    a.out_visible = outs.ball_visible;
    a.out_bass_lit = outs.bass_lit;
    a.out_bass_rgba = outs.bass_rgba;
    a.out_bloom = outs.bloom;
    for (size_t f0 = 0; f0 < n_frames; f0 += pf) {
        a.f0 = static_cast<uint32_t>(f0);
        a.pf = static_cast<uint32_t>(std::min(pf, n_frames - f0));
        const size_t rows_here = static_cast<size_t>(n_streams_) * a.pf;
        a.rec = rec_.as<scene::PeakRecord>();
        // the headers follow the records of the largest piece
        a.hdr = reinterpret_cast<RowHeader*>(rec_.as<char>() + static_cast<size_t>(in.max_peaks) * sizeof(scene::PeakRecord) * n_streams_ * pf);
        hipLaunchKernelGGL(scene_peaks, dim3(static_cast<unsigned>(std::min<size_t>(rows_here, 256 * 32))), dim3(64), 0, stream, a);
        launch_nk<1>(static_cast<int>((n + 63) / 64), a, dim3(n_streams_), stream);
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

pvq_status SceneBatch::get_state(uint32_t stream_index, float* ball_xyzs, float* ball_rgba, float* ball_params, uint32_t* ball_visible,
                                 uint32_t* bass_lit, float* bass_rgba, float* bloom) {
    if (stream_index >= n_streams_) {
        set_last_error("scene batch: stream index out of range");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched scene runs on a GPU; this handle has none");
        return PVQ_ERR_NO_DEVICE;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipDeviceSynchronize());
    const uint32_t n = s_.n_bins;
    std::vector<float> st(static_cast<size_t>(STATE_FIELDS) * n);
    float sc[8];
    PVQ_HIP(hipMemcpy(st.data(), state_.as<float>() + static_cast<size_t>(stream_index) * st.size(), st.size() * sizeof(float), hipMemcpyDeviceToHost));
    PVQ_HIP(hipMemcpy(sc, scalars_.as<float>() + static_cast<size_t>(stream_index) * 8, sizeof(sc), hipMemcpyDeviceToHost));
    const uint32_t words = (n + 31) / 32;
    if (ball_visible) std::fill(ball_visible, ball_visible + words, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        if (ball_xyzs) {
            ball_xyzs[4 * i] = st[SX * n + i];
            ball_xyzs[4 * i + 1] = st[SY * n + i];
            ball_xyzs[4 * i + 2] = st[SZ * n + i];
            ball_xyzs[4 * i + 3] = st[SSCALE * n + i];
        }
        if (ball_rgba) {
            ball_rgba[4 * i] = st[SR * n + i];
            ball_rgba[4 * i + 1] = st[SG * n + i];
            ball_rgba[4 * i + 2] = st[SB * n + i];
            ball_rgba[4 * i + 3] = st[SA * n + i];
        }
        if (ball_params) {
            ball_params[3 * i] = st[SPC * n + i];
            ball_params[3 * i + 1] = st[SPA * n + i];
            ball_params[3 * i + 2] = st[SPD * n + i];
        }
        uint32_t v;
        std::memcpy(&v, &st[SVIS * n + i], 4);
        if (ball_visible && v) ball_visible[i / 32] |= 1u << (i % 32);
    }
    if (bass_lit) std::memcpy(bass_lit, &sc[0], 4);
    if (bass_rgba)
        for (int i = 0; i < 4; ++i) bass_rgba[i] = sc[1 + i];
    if (bloom) *bloom = sc[5];
    return PVQ_OK;
}

}  // namespace pvq
