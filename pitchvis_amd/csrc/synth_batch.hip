// synth_batch.hip — the replay of the synthesizer's plan for many streams (synth_batch.hpp).
//
// synth_replay: a workgroup of one wavefront per stream, a lane per voice object.  Per 64-sample block:
//   1. the block's records (64 bytes each) come into LDS as 16-byte pieces, consecutive lanes on consecutive pieces;
//   2. record k names its voice object, and lane `voice` takes record k: the lane walks the 64 samples with synth::walk_block — the
//      16-bit reads of eight samples are issued before the first of them enters the filter chain, position and x1 x2 y1 y2 stay in
//      registers from block to block — and writes both products a_left * x and a_right * x, a stepped by the reference's repeated
//      addition, to row k of two [64][65] LDS tiles (row stride 65 dwords: the 64 lanes of a column write, and later the 64 lanes of a
//      row read, 64 distinct banks);
//   3. lanes turn from "voice" to "sample index": lane t adds column t of rows 0 .. n - 1 in record order, skipping the channels
//      write_block skips (synthesizer.rs:485), which is the host replay's sum; one coalesced 256-byte store per row and channel.
// No lane walks a global row: rows are only ever written 64 consecutive dwords at a time.  FMA contraction is off (synth_math.hpp),
// f32 subnormals are kept, the i64 -> f32 conversion is the correctly rounded one on both sides.
//
// With effects the plan and its sends are replayed by synth_replay_fx, a unit of its own (synth_fx_batch.hip): this unit keeps its
// one kernel, its code path and its resources.
#include "synth_batch.hpp"

#include "synth_device.hpp"

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>

namespace pvq {

namespace {
__global__ __launch_bounds__(64) void synth_replay(SynthArgs a) {
#pragma clang fp contract(off)
    __shared__ uint4 s_rec[64 * 4];
    __shared__ float s_left[64 * LDT];
    __shared__ float s_right[64 * LDT];
    __shared__ uint32_t s_slot[64];
    const uint32_t lane = threadIdx.x;
    const SynthStream st = a.tab[blockIdx.x];
    uint4* state = a.lanes + static_cast<size_t>(blockIdx.x) * 128;
    const uint4 p0 = state[lane], p1 = state[64 + lane];
    synth::Lane s;
    s.position_fp = static_cast<int64_t>((static_cast<uint64_t>(p0.y) << 32) | p0.x);
    s.x1 = __uint_as_float(p1.x);
    s.x2 = __uint_as_float(p1.y);
    s.y1 = __uint_as_float(p1.z);
    s.y2 = __uint_as_float(p1.w);
    uint32_t desc_index = p0.z;
    synth::SampleDesc desc = a.descs[desc_index];
    const uint32_t* ptr = a.block_ptr + st.ptr_base;
    const synth::Record* recs = reinterpret_cast<const synth::Record*>(s_rec);
    for (uint32_t b = 0; b < st.n_blocks; ++b) {
        const uint32_t r0 = ptr[b], n = ptr[b + 1] - r0;   // n <= 64: the host checked
        s_slot[lane] = 0xffffffffu;
        for (uint32_t p = lane; p < 4 * n; p += 64) s_rec[p] = a.records[static_cast<size_t>(r0) * 4 + p];
        __syncthreads();
        if (lane < n) s_slot[recs[lane].voice] = lane;
        __syncthreads();
        const uint32_t slot = s_slot[lane];
        if (slot != 0xffffffffu) {
            const synth::Record rec = recs[slot];
            if (rec.flags & synth::F_START) {
                desc_index = rec.desc;
                desc = a.descs[desc_index];
            }
            const synth::MixGain gl = synth::mix_gain(rec.gain[0], rec.gain[1]), gr = synth::mix_gain(rec.gain[2], rec.gain[3]);
            float* tl = s_left + slot * LDT;
            float* tr = s_right + slot * LDT;
            synth::walk_block(rec, desc, a.wave, s, gl, gr, [&](int t, float pl, float pr) {
                tl[t] = pl;
                tr[t] = pr;
            });
        }
        __syncthreads();
        float acc_l = 0.0f, acc_r = 0.0f;   // synthesizer.rs:367-391, lane = sample index
        for (uint32_t k = 0; k < n; ++k) {
            const synth::MixGain gl = synth::mix_gain(recs[k].gain[0], recs[k].gain[1]), gr = synth::mix_gain(recs[k].gain[2], recs[k].gain[3]);
            if (gl.mode != synth::MIX_SKIP) acc_l += s_left[k * LDT + lane];
            if (gr.mode != synth::MIX_SKIP) acc_r += s_right[k * LDT + lane];
        }
        st.left[static_cast<size_t>(b) * synth::BLOCK + lane] = acc_l;
        st.right[static_cast<size_t>(b) * synth::BLOCK + lane] = acc_r;
        __syncthreads();   // the records and tiles are free for the next block
    }
    state[lane] = make_uint4(static_cast<uint32_t>(static_cast<uint64_t>(s.position_fp)), static_cast<uint32_t>(static_cast<uint64_t>(s.position_fp) >> 32),
                             desc_index, 0u);
    state[64 + lane] = make_uint4(__float_as_uint(s.x1), __float_as_uint(s.x2), __float_as_uint(s.y1), __float_as_uint(s.y2));
}
}  // namespace

SynthBatch::~SynthBatch() {
    if (uploaded_) {
        (void)hipEventSynchronize(uploaded_);
        (void)hipEventDestroy(uploaded_);
    }
    if (began_) (void)hipEventDestroy(began_);
    if (ended_) (void)hipEventDestroy(ended_);
}

pvq_status SynthBatch::create(int device_id, std::shared_ptr<const SynthBank> bank, uint32_t n_streams, int32_t sample_rate, uint32_t maximum_polyphony,
                              std::unique_ptr<SynthBatch>& out, bool effects) {
    out.reset();
    if (n_streams == 0) {
        set_last_error("synth batch: zero streams");
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<SynthBatch> b(new SynthBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->n_streams_ = n_streams;
    b->bank_ = bank;
    b->effects_ = effects;
    b->states_.resize(n_streams);
    b->plans_.resize(n_streams);
    std::string err;
    for (uint32_t s = 0; s < n_streams; ++s) {
        if (pvq_status st = SynthState::create(bank, sample_rate, maximum_polyphony, b->states_[s], err, effects, true)) {
            set_last_error(err);
            return st;
        }
        b->plans_[s].clear();
    }
    std::unique_ptr<SynthEffects> fx;   // the layout and the table, and the check of the table's bounds: before any device is touched
    if (effects) {
        if (pvq_status st = SynthEffects::create(sample_rate, fx, err)) {
            set_last_error(err);
            return st;
        }
        b->master_volume_ = b->states_[0]->master_volume();
    }
    if (device_id >= 0) {
        PVQ_HIP(hipSetDevice(device_id));
        std::vector<int16_t> wave(bank->wave);
        wave.resize((wave.size() + 7) / 8 * 8, 0);
        if (pvq_status st = b->wave_.upload(wave.data(), wave.size() * sizeof(int16_t))) return st;
        if (pvq_status st = b->descs_.upload(bank->descs.data(), bank->descs.size() * sizeof(synth::SampleDesc))) return st;
        const size_t lane_bytes = static_cast<size_t>(n_streams) * 128 * sizeof(uint4);
        if (pvq_status st = b->lanes_.reserve(lane_bytes)) return st;
        PVQ_HIP(hipMemset(b->lanes_.as<void>(), 0, lane_bytes));
        if (pvq_status st = b->tab_.reserve(n_streams * sizeof(SynthStream))) return st;
        if (effects) {
            const synth::FxLayout& l = fx->layout();
            if (pvq_status st = b->fx_layout_.upload(&l, sizeof l)) return st;
            if (pvq_status st = b->fx_table_.upload(fx->table().data(), fx->table().size() * sizeof(float))) return st;
            const size_t sizes[4] = {static_cast<size_t>(n_streams) * l.total * sizeof(float), static_cast<size_t>(n_streams) * 2 * synth::FX_COMBS * sizeof(float),
                                     static_cast<size_t>(n_streams) * 2 * l.ring * sizeof(float), static_cast<size_t>(n_streams) * sizeof(unsigned long long)};
            DeviceBuffer* const bufs[4] = {&b->fx_reverb_, &b->fx_store_, &b->fx_ring_, &b->fx_count_};
            for (int k = 0; k < 4; ++k) {
                if (pvq_status st = bufs[k]->reserve(sizes[k])) return st;
                PVQ_HIP(hipMemset(bufs[k]->as<void>(), 0, sizes[k]));
            }
        }
        PVQ_HIP(hipDeviceSynchronize());
    }
    out = std::move(b);
    return PVQ_OK;
}

pvq_status SynthBatch::render_device(const SynthEvents* events, const size_t* n_blocks, float* const* d_left, float* const* d_right,
                                     const uint32_t* snapshot_blocks, size_t n_snapshots, hipStream_t stream) {
    if (!events || !n_blocks || !d_left || !d_right) {
        set_last_error("synth batch: the events, n_blocks, left and right tables must be non-null");
        return PVQ_ERR_INVALID_ARG;
    }
    if (n_snapshots && !snapshot_blocks) {
        set_last_error("synth batch: snapshot_blocks is null");
        return PVQ_ERR_INVALID_ARG;
    }
    size_t total_blocks = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) {
        if (n_blocks[s] > 0x7fffffffull / synth::BLOCK) {
            set_last_error("synth batch: stream " + std::to_string(s) + " is too long");
            return PVQ_ERR_INVALID_ARG;
        }
        if (n_blocks[s] && (!d_left[s] || !d_right[s])) {
            set_last_error("synth batch: stream " + std::to_string(s) + " has a null left or right pointer");
            return PVQ_ERR_INVALID_ARG;
        }
        if ((reinterpret_cast<uintptr_t>(d_left[s]) | reinterpret_cast<uintptr_t>(d_right[s])) & 3) {
            set_last_error("synth batch: stream " + std::to_string(s) + " has a row that is not 4-byte aligned");
            return PVQ_ERR_INVALID_ARG;
        }
        total_blocks += n_blocks[s];
    }
    if (total_blocks + n_streams_ > 0xffffffffull) {
        set_last_error("synth batch: more than 2^32 blocks in one call");
        return PVQ_ERR_INVALID_ARG;
    }
    if (broken_) {
        set_last_error("synth batch: an earlier call failed while planning; the handle cannot go on");
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched synthesizer runs on a GPU; this handle has none (pvq_synth_state_render is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<SynthState*> states(n_streams_);
    for (uint32_t s = 0; s < n_streams_; ++s) states[s] = states_[s].get();
    std::string err;
    if (pvq_status st = synth_plan_streams(states.data(), events, n_blocks, n_streams_, snapshot_blocks, n_snapshots, plans_.data(), err)) {
        broken_ = true;
        set_last_error(err);
        return st;
    }
    const auto t1 = std::chrono::steady_clock::now();
    plan_ms_ = std::chrono::duration<float, std::milli>(t1 - t0).count();
    stage_ms_ = 0.0f;
    timed_ = false;
    if (total_blocks == 0) return PVQ_OK;
    size_t total_records = 0;
    for (uint32_t s = 0; s < n_streams_; ++s) total_records += plans_[s].records.size();
    if (total_records > 0xffffffffull) {
        set_last_error("synth batch: more than 2^32 voice-blocks in one call");
        return PVQ_ERR_INVALID_ARG;
    }
    PVQ_HIP(hipSetDevice(device_id_));
    // the staging vectors live in the handle: the copies of the call before may still read them
    if (uploaded_) PVQ_HIP(hipEventSynchronize(uploaded_));
    else {
        PVQ_HIP(hipEventCreate(&uploaded_));
        PVQ_HIP(hipEventCreate(&began_));
        PVQ_HIP(hipEventCreate(&ended_));
    }
    std::vector<SynthStream> tab(n_streams_);
    std::vector<uint32_t>& block_ptr = h_block_ptr_;
    block_ptr.clear();
    block_ptr.reserve(total_blocks + n_streams_);
    std::vector<synth::Record>& records = h_records_;
    records.clear();
    records.reserve(std::max<size_t>(total_records, 1));
    std::vector<synth::Sends>& sends = h_sends_;
    sends.clear();
    if (effects_) sends.reserve(std::max<size_t>(total_records, 1));
    for (uint32_t s = 0; s < n_streams_; ++s) {
        const SynthPlan& p = plans_[s];
        tab[s] = SynthStream{d_left[s], d_right[s], static_cast<uint32_t>(n_blocks[s]), static_cast<uint32_t>(block_ptr.size())};
        const uint32_t base = static_cast<uint32_t>(records.size());
        for (size_t b = 0; b <= n_blocks[s]; ++b) {
            if (b > 0 && p.block_ptr[b] - p.block_ptr[b - 1] > SYNTH_MAX_POLYPHONY) {
                set_last_error("synth batch: a block with more records than voice objects");
                return PVQ_ERR_INTERNAL;
            }
            block_ptr.push_back(base + p.block_ptr[b]);
        }
        records.insert(records.end(), p.records.begin(), p.records.end());
        if (effects_) {
            if (p.sends.size() != p.records.size()) {
                set_last_error("synth batch: a plan whose sends do not match its records");
                return PVQ_ERR_INTERNAL;
            }
            sends.insert(sends.end(), p.sends.begin(), p.sends.end());
        }
    }
    if (records.empty()) records.push_back(synth::Record{});
    if (effects_ && sends.empty()) sends.push_back(synth::Sends{});
    if (effects_)
        if (pvq_status st = sends_.reserve(sends.size() * sizeof(synth::Sends))) return st;
    if (pvq_status st = block_ptr_.reserve(block_ptr.size() * sizeof(uint32_t))) return st;
    if (pvq_status st = records_.reserve(records.size() * sizeof(synth::Record))) return st;
    stage_ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
    PVQ_HIP(hipEventRecord(began_, stream));
    h_tab_.assign(reinterpret_cast<const unsigned char*>(tab.data()), reinterpret_cast<const unsigned char*>(tab.data() + tab.size()));
    PVQ_HIP(hipMemcpyAsync(tab_.as<void>(), h_tab_.data(), h_tab_.size(), hipMemcpyHostToDevice, stream));
    PVQ_HIP(hipMemcpyAsync(block_ptr_.as<void>(), block_ptr.data(), block_ptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    PVQ_HIP(hipMemcpyAsync(records_.as<void>(), records.data(), records.size() * sizeof(synth::Record), hipMemcpyHostToDevice, stream));
    SynthArgs a{};
    a.tab = tab_.as<SynthStream>();
    a.block_ptr = block_ptr_.as<uint32_t>();
    a.records = records_.as<uint4>();
    a.wave = wave_.as<int16_t>();
    a.descs = descs_.as<synth::SampleDesc>();
    a.lanes = lanes_.as<uint4>();
    if (effects_) PVQ_HIP(hipMemcpyAsync(sends_.as<void>(), sends.data(), sends.size() * sizeof(synth::Sends), hipMemcpyHostToDevice, stream));
    PVQ_HIP(hipEventRecord(uploaded_, stream));
    if (effects_) {
        SynthFxArgs fa{};
        fa.dry = a;
        fa.sends = sends_.as<uint4>();
        fa.layout = fx_layout_.as<uint32_t>();
        fa.table = fx_table_.as<float>();
        fa.reverb = fx_reverb_.as<float>();
        fa.store = fx_store_.as<float>();
        fa.ring = fx_ring_.as<float>();
        fa.count = fx_count_.as<unsigned long long>();
        fa.master_volume = master_volume_;
        launch_synth_replay_fx(fa, n_streams_, stream);
    } else {
        hipLaunchKernelGGL(synth_replay, dim3(n_streams_), dim3(64), 0, stream, a);
    }
    PVQ_HIP(hipGetLastError());
    PVQ_HIP(hipEventRecord(ended_, stream));
    timed_ = true;
    last_records_ = total_records;
    return PVQ_OK;
}

pvq_status SynthBatch::last_times(float* out4, uint64_t* out_records) {
    if (!out4) {
        set_last_error("synth batch: out4 is needed");
        return PVQ_ERR_INVALID_ARG;
    }
    out4[0] = plan_ms_;
    out4[1] = stage_ms_;
    out4[2] = out4[3] = 0.0f;
    if (out_records) *out_records = timed_ ? last_records_ : 0;
    if (!timed_) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));
    PVQ_HIP(hipEventSynchronize(ended_));
    PVQ_HIP(hipEventElapsedTime(&out4[2], began_, uploaded_));
    PVQ_HIP(hipEventElapsedTime(&out4[3], uploaded_, ended_));
    return PVQ_OK;
}

}  // namespace pvq
