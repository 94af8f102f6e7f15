// synth_fx_batch.hip — the replay of the synthesizer's plan WITH its effects for many streams (synth_batch.hpp, PVQ_SYNTH_EFFECTS).
//
// synth_replay_fx: the same plan with its sends (enable_reverb_and_chorus; synth_fx_math.hpp), again one wavefront per stream.  Per block:
//   1. records and sends come into LDS; the voice lanes walk a QUARTER of a block at a time (walk_span over 16 samples) and write
//      five products — dry left / right, chorus left / right, reverb — to [64][17] tiles (22 KB; five whole-block tiles would be
//      83 KB and one workgroup a CU, half-block tiles 42 KB and two: with quarters the kernel's LDS is below the dry kernel's and
//      four workgroups share a CU); position, filter memory and the five stepped gains stay in registers across the quarters;
//   2. per quarter, 16 lanes a channel sum sample t of dry left, dry right, chorus left, chorus right (the first 16 then the reverb
//      input too), in record order with each channel's own skip bit, into five [64] sums;
//   3. lane = sample: the chorus reads its two ring slots — a slot this block has already overwritten (input s < t) from the sums in
//      LDS, any other from the ring in global memory — then the block's 64 inputs go to the ring, one coalesced store a channel;
//   4. lane = sample: 16 comb and 8 all-pass values are read, 64 consecutive dwords a buffer (two runs where the ring wraps); the
//      comb outputs are flushed and summed in comb order, and the 16 x 64 comb values are staged in LDS;
//   5. lane = comb (16 lanes, 64 steps): the filter_store recurrence over the staged values, in place; then lane = sample writes
//      the 16 buffers back, coalesced;
//   6. lane = sample: the four all-passes in series, the wet mix, the final sum and the two row stores.
// No lane walks a global row.  Ordering: a buffer or ring position stored in one block is loaded by ANOTHER lane in a later block —
// the very next one for the 82-sample all-pass and the 64-slot ring at 16 kHz.  The __syncthreads() that ends each block stands
// between them, and that suffices here because the workgroup is ONE wavefront on one CU: a wave's vector memory instructions are
// issued in program order to that CU's L1, which is the only L1 between this wave and its state (the state of a stream is touched
// by no other workgroup in a launch, and launches of a handle are ordered by their stream), so a later load cannot pass an earlier
// store to the same address; the barrier is the workgroup-scope release / acquire that keeps the compiler from moving one across
// the other.  (Programming guide, "Execution model": every CU has its own vector L1 and workgroup scope stays inside a CU;
// Guideline 16: only data handed between workgroups needs agent-scope release / acquire.  Nothing here is handed between workgroups.)
#include "synth_device.hpp"

namespace pvq {

namespace {
constexpr int SPAN = synth::BLOCK / 4, LDS_ROW = SPAN + 1;   // samples of a walk span, dwords of a product tile's row
constexpr int TILE = 64 * LDS_ROW + SPAN;                    // dwords from one channel's tile to the next: the four channels summed side by side start 16 banks apart
constexpr int NFX = synth::FX_CHANNELS;
constexpr int LAYOUT_WORDS = sizeof(synth::FxLayout) / sizeof(uint32_t);
static_assert(LAYOUT_WORDS <= 64, "one lane a word");

__global__ __launch_bounds__(64) void synth_replay_fx(SynthFxArgs fa) {
#pragma clang fp contract(off)
    __shared__ uint4 s_rec[64 * 4];
    __shared__ uint4 s_snd[64 * 2];
    __shared__ float s_prod[NFX * TILE];
    __shared__ float s_sum[NFX][64];
    __shared__ float s_comb[2 * synth::FX_COMBS * LDT];
    __shared__ uint32_t s_slot[64];
    __shared__ uint32_t s_mask[64];
    __shared__ uint32_t s_lay[LAYOUT_WORDS];
    __shared__ uint32_t s_pos[synth::FX_BUFFERS];
    const SynthArgs& a = fa.dry;
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
    if (lane < LAYOUT_WORDS) s_lay[lane] = fa.layout[lane];
    __syncthreads();
    const synth::FxLayout& lay = *reinterpret_cast<const synth::FxLayout*>(s_lay);
    const uint32_t ring = lay.ring, table = lay.table;
    const unsigned long long count = fa.count[blockIdx.x];
    if (lane < synth::FX_BUFFERS) s_pos[lane] = static_cast<uint32_t>(count % lay.len[lane]);
    uint32_t ring_index = static_cast<uint32_t>(count % ring);
    uint32_t table_index[2] = {static_cast<uint32_t>(count % table), static_cast<uint32_t>((count + table / 4) % table)};   // chorus.rs:34-35
    float* const rv = fa.reverb + static_cast<size_t>(blockIdx.x) * lay.total;
    float* const rg = fa.ring + static_cast<size_t>(blockIdx.x) * 2 * ring;
    float filter_store = lane < 2 * synth::FX_COMBS ? fa.store[static_cast<size_t>(blockIdx.x) * 2 * synth::FX_COMBS + lane] : 0.0f;
    const synth::ReverbConstants kc = synth::reverb_constants();
    const uint32_t* ptr = a.block_ptr + st.ptr_base;
    const synth::Record* recs = reinterpret_cast<const synth::Record*>(s_rec);
    const synth::Sends* snds = reinterpret_cast<const synth::Sends*>(s_snd);
    const uint32_t part = lane / SPAN, tt = lane % SPAN;   // in the sums: the channel and the sample of the span
    __syncthreads();
    for (uint32_t b = 0; b < st.n_blocks; ++b) {
        const uint32_t r0 = ptr[b], n = ptr[b + 1] - r0;   // n <= 64: the host checked
        s_slot[lane] = 0xffffffffu;
        for (uint32_t p = lane; p < 4 * n; p += 64) s_rec[p] = a.records[static_cast<size_t>(r0) * 4 + p];
        for (uint32_t p = lane; p < 2 * n; p += 64) s_snd[p] = fa.sends[static_cast<size_t>(r0) * 2 + p];
        __syncthreads();
        if (lane < n) s_slot[recs[lane].voice] = lane;
        __syncthreads();
        const uint32_t slot = s_slot[lane];
        const bool sounds = slot != 0xffffffffu;
        synth::Record rec{};
        synth::MixGain g[NFX] = {};
        synth::Walk w{0, 0.0f, 0.0f};
        if (sounds) {
            rec = recs[slot];
            if (rec.flags & synth::F_START) {
                desc_index = rec.desc;
                desc = a.descs[desc_index];
            }
            synth::fx_gains(rec, snds[slot], g);
            uint32_t mask = 0;
            for (int c = 0; c < NFX; ++c) mask |= (g[c].mode != synth::MIX_SKIP ? 1u : 0u) << c;
            s_mask[slot] = mask;
            w = synth::walk_begin(rec, desc, s);
        }
        for (int h = 0; h < synth::BLOCK / SPAN; ++h) {
            if (sounds) {
                float* tile = s_prod + slot * LDS_ROW - h * SPAN;
                synth::walk_span<NFX>(rec, desc, a.wave, s, w, g, h * SPAN, (h + 1) * SPAN, [&](int t, const float(&p)[NFX]) {
                    for (int c = 0; c < NFX; ++c) tile[c * TILE + t] = p[c];
                });
            }
            __syncthreads();
            float acc0 = 0.0f, acc1 = 0.0f;   // synthesizer.rs:372-391, 403-423, 448-462: channel `part`, and with part 0 the reverb input
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t mask = s_mask[k];
                if ((mask >> part) & 1u) acc0 += s_prod[part * TILE + k * LDS_ROW + tt];
                if (part == 0 && ((mask >> 4) & 1u)) acc1 += s_prod[4 * TILE + k * LDS_ROW + tt];
            }
            s_sum[part][h * SPAN + tt] = acc0;
            if (part == 0) s_sum[4][h * SPAN + tt] = acc1;
            __syncthreads();
        }
        if (sounds) synth::walk_end(rec, s, w);
        // chorus (chorus.rs:59-117), lane = sample
        float cho[2];
        for (int c = 0; c < 2; ++c) {
            const float* ring_c = rg + c * ring;
            uint32_t ri = ring_index + lane, ti = table_index[c] + lane;
            if (ri >= ring) ri -= ring;
            if (ti >= table) ti -= table;
            const synth::ChorusTap tap = synth::chorus_tap(ri, fa.table[ti], ring);
            float x[2];
            const uint32_t idx[2] = {tap.index1, tap.index2};
            for (int q = 0; q < 2; ++q) {
                const uint32_t j = idx[q];
                const uint32_t written = j >= ring_index ? j - ring_index : j + ring - ring_index;   // the sample of this block that writes slot j, if < 64
                const float old_value = ring_c[j], new_value = s_sum[2 + c][written & 63];
                x[q] = written < lane ? new_value : old_value;
            }
            cho[c] = synth::chorus_mix(tap, x[0], x[1]);
        }
        // reverb reads (reverb.rs:297, 371), lane = sample: every value is older than the block
        float rev[2], ap[2 * synth::FX_ALLPASSES];
        uint32_t ap_at[2 * synth::FX_ALLPASSES];
        for (int c = 0; c < 2; ++c) {
            float v[synth::FX_COMBS];
            for (int i = 0; i < synth::FX_COMBS; ++i) {
                const int bi = c * synth::FX_COMBS + i;
                uint32_t p = s_pos[bi] + lane;
                if (p >= lay.len[bi]) p -= lay.len[bi];
                v[i] = rv[lay.off[bi] + p];
                s_comb[bi * LDT + lane] = v[i];
            }
            rev[c] = synth::comb_output_sum([&](int i) { return v[i]; });
        }
        for (int q = 0; q < 2 * synth::FX_ALLPASSES; ++q) {
            const int bi = synth::FX_FIRST_ALLPASS + q;
            uint32_t p = s_pos[bi] + lane;
            if (p >= lay.len[bi]) p -= lay.len[bi];
            ap_at[q] = lay.off[bi] + p;
            ap[q] = rv[ap_at[q]];
        }
        __syncthreads();   // the ring's loads above, its stores below
        for (int c = 0; c < 2; ++c) {
            uint32_t ri = ring_index + lane;
            if (ri >= ring) ri -= ring;
            rg[c * ring + ri] = s_sum[2 + c][lane];   // chorus.rs:77
        }
        if (lane < 2 * synth::FX_COMBS) {   // the comb recurrence (reverb.rs:302-307), lane = comb
            float* row = s_comb + lane * LDT;
            for (int t0 = 0; t0 < synth::BLOCK; t0 += 8) {
                float v[8], in[8];
                PVQ_SYNTH_UNROLL
                for (int k = 0; k < 8; ++k) {
                    v[k] = row[t0 + k];
                    in[k] = s_sum[4][t0 + k];
                }
                PVQ_SYNTH_UNROLL
                for (int k = 0; k < 8; ++k) row[t0 + k] = synth::comb_step(v[k], in[k], filter_store, kc);
            }
        }
        __syncthreads();
        for (int bi = 0; bi < 2 * synth::FX_COMBS; ++bi) {
            uint32_t p = s_pos[bi] + lane;
            if (p >= lay.len[bi]) p -= lay.len[bi];
            rv[lay.off[bi] + p] = s_comb[bi * LDT + lane];
        }
        for (int c = 0; c < 2; ++c) {   // reverb.rs:172-182, 369-377
            float x = rev[c];
            for (int k = 0; k < synth::FX_ALLPASSES; ++k) {
                const int q = c * synth::FX_ALLPASSES + k;
                x = synth::allpass_step(ap[q], x);
                rv[ap_at[q]] = ap[q];
            }
            rev[c] = x;
        }
        synth::reverb_wet_mix(rev[0], rev[1], kc);
        st.left[static_cast<size_t>(b) * synth::BLOCK + lane] = synth::fx_final(s_sum[0][lane], cho[0], rev[0], fa.master_volume);
        st.right[static_cast<size_t>(b) * synth::BLOCK + lane] = synth::fx_final(s_sum[1][lane], cho[1], rev[1], fa.master_volume);
        __syncthreads();   // every read of s_pos and the sums is done
        if (lane < synth::FX_BUFFERS) {
            uint32_t p = s_pos[lane] + synth::BLOCK;   // every buffer is longer than a block
            if (p >= lay.len[lane]) p -= lay.len[lane];
            s_pos[lane] = p;
        }
        ring_index += synth::BLOCK;   // the ring is at least a block long
        if (ring_index >= ring) ring_index -= ring;
        for (int c = 0; c < 2; ++c) {
            table_index[c] += synth::BLOCK;
            if (table_index[c] >= table) table_index[c] -= table;
        }
        __syncthreads();   // the block's stores stand before the next block's loads; records, tiles and sums are free
    }
    state[lane] = make_uint4(static_cast<uint32_t>(static_cast<uint64_t>(s.position_fp)), static_cast<uint32_t>(static_cast<uint64_t>(s.position_fp) >> 32),
                             desc_index, 0u);
    state[64 + lane] = make_uint4(__float_as_uint(s.x1), __float_as_uint(s.x2), __float_as_uint(s.y1), __float_as_uint(s.y2));
    if (lane < 2 * synth::FX_COMBS) fa.store[static_cast<size_t>(blockIdx.x) * 2 * synth::FX_COMBS + lane] = filter_store;
    if (lane == 0) fa.count[blockIdx.x] = count + static_cast<unsigned long long>(st.n_blocks) * synth::BLOCK;
}
}  // namespace

void launch_synth_replay_fx(const SynthFxArgs& args, uint32_t n_streams, hipStream_t stream) {
    hipLaunchKernelGGL(synth_replay_fx, dim3(n_streams), dim3(64), 0, stream, args);
}

}  // namespace pvq
