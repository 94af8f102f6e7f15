// vqt_blockdft.hip — hop-block DFT path of the batched VQT (fp32 MFMA GEMM + phase-combine tree).
//
// What it replaces: the per-frame real FFTs of Vqt::calculate_vqt_instant_in_db (reference
// pitchvis_analysis/src/vqt.rs:876-887) when many frames are analysed at a small hop.  The
// reference (one call per frame) cannot share work between frames; a batch can.  With hop h
// dividing every analysis window W_g, frame f's window of group g is the union of the Nb_g = W_g/h
// hop blocks j = f .. f+Nb_g-1 (blocks of group g start at s_g + j*h), and the low spectrum
// columns c the sparse kernel reads (vqt.rs:725-735: c <= W_g/(2M)) are
//
//     X_f[c] = sum_{b<Nb} e^{-2 pi i c b / Nb} * P_g[f+b][c],   P_g[j][c] = sum_{m<h} x[s_g+jh+m] e^{-2 pi i c m / W_g}
//
// P is a dense real GEMM  [blocks x h] . [h x 2*n_cols]  shared by all Nb frames that see the
// block (exact-f32 MFMA v_mfma_f32_32x32x2_f32, the matrix is 100 % dense), the sum over b is a
// log2(Nb)-level tree  A_{l+1}[j] = A_l[j] + phi^(2^l) A_l[j+2^l]  evaluated in LDS, then the
// banded complex row dots (vqt.rs:889-910) and power_to_db (vqt.rs:922-954) as in the FFT path.
//
// Three units and one private header (blockdft_device.hpp: BlockDftTables, BlockLaunch, the workspace helper, the shared constants):
//   vqt_blockdft.hip    this file, the path's host side: tables to the device, workspaces, a call's walk over its launches
//   blockdft_gemm.hip   blockdft_gemm_tree[_bf16x3], blockdft_gemm_gen, blockdft_tree_finish, blockdft_gemm_rows + blockdft_combine,
//                       their launchers and the tile-list cache
//   blockdft_dots.hip   blockdft_banddots4c_db / blockdft_banddots_db[_bf16x3] (kernel product as a banded MFMA GEMM + power_to_db)
//                       and their launcher
// Host planning (tables, run packing, tile lists) is blockdft_plan.cpp; this file uploads what it builds and walks the launches.
#include <algorithm>
#include <cmath>

#include "blockdft_device.hpp"

namespace pvq {

// Frames per sub-batch: the X (+ Y) workspace is sized for one.  As many as the handle's workspace limit holds (default 1 GiB:
// 131 072 frames at 48 kHz / 252 bins = 0.74 GB; wide geometries — 840 bins: 15 KB per frame — take fewer), a multiple of 64,
// at most 147 456 (BASELINE configs[2]'s 131 072 per rank is one sub-batch; against two of 65 536 the step is 4 % shorter: one ramp and
// one tail per kernel instead of two); sub-batches small enough for the Infinity Cache were measured no faster (32 768: 9 % slower).
static size_t chunk_frames(size_t limit_bytes, size_t bytes_per_frame) {
    const long knob = dev_knob("PVQ_CHUNK_FRAMES", 0);   // (developer build; read per call)
    if (knob >= 64) return (size_t)knob;
    size_t f = limit_bytes / std::max<size_t>(bytes_per_frame, 1) / 64 * 64;
    return std::min<size_t>(std::max<size_t>(f, 64), 147456);   // (131 072 + an eighth: 64 staged streams of 2 048 frames with their gaps are 135 168 frames — one launch, not one and a 4 000-frame tail)
}

void free_blockdft_tables(BlockDftTables* t) {
    if (!t) return;
    for (void* p : {(void*)t->d_E, (void*)t->d_Et, (void*)t->d_tile_group, (void*)t->d_tile_s, (void*)t->d_groups, (void*)t->d_comb_tw, (void*)t->d_band, (void*)t->d_band_B,
                    (void*)t->d_band8, (void*)t->d_band_B4, (void*)t->d_band_list8, (void*)t->d_band_stages8, (void*)t->d_band_B3, (void*)t->d_band_list, (void*)t->d_P, (void*)t->d_X, (void*)t->d_Y,
                    (void*)t->d_clk, (void*)t->d_E16, (void*)t->d_E16R, (void*)t->d_gen_tw})
        if (p) (void)hipFree(p);
    for (auto& tl : t->tile_lists)
        if (tl.d) (void)hipFree(tl.d);
    delete t;
}

// median over the sampled workgroups of the last profiled fused-GEMM launch: shader clock (MHz) held inside the K loop
float Vqt::last_sclk_mhz() {
    if (!dev_ || !dev_->block || !dev_->block->d_clk || dev_->block->clk_n <= 0) return 0.0f;
    BlockDftTables* t = dev_->block;
    const int per = 4;
    std::vector<unsigned long long> h((size_t)t->clk_n * per);
    if (hipSetDevice(device_id_) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0.0f;
    if (hipMemcpy(h.data(), t->d_clk, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0.0f;
    std::vector<double> r;
    for (int i = 0; i < t->clk_n; ++i)
        if (h[per * i + 3] > h[per * i + 1]) r.push_back(100.0 * (double)(h[per * i + 2] - h[per * i]) / (double)(h[per * i + 3] - h[per * i + 1]));
    if (r.empty()) return 0.0f;
    std::sort(r.begin(), r.end());
    return (float)r[r.size() / 2];
}

uint32_t Vqt::blockdft_columns() const { return (dev_ && dev_->block) ? (uint32_t)(dev_->block->n_tiles * CB_C) : 0u; }

// whether the block-DFT path can take several streams in one launch (the fused GEMM + tree kernels; the unfused fallback stages —
// more than 8 window groups — run one stream per call).  A pure predicate on the plan: it builds no tables and evicts none (a query
// such as pvq_vqt_resolve_algo must not move the handle's tables of the hop in use, let alone allocate on whatever device is current).
bool Vqt::blockdft_takes_streams(size_t hop) const {
    if (!blockdft_applicable(hop)) return false;
    const auto& groups = plan_.kernel.window_groups;
    bool divides = (hop & (hop - 1)) == 0;
    size_t nb_max = 0;
    for (const WindowGroup& g : groups) {
        divides = divides && g.window_size() % hop == 0;
        nb_max = std::max(nb_max, g.window_size() / hop);
    }
    if (!divides) return true;   // a general hop: blockdft_gemm_gen (blockdft_applicable has checked its conditions)
    const bool use_bf = gemm_split_bf16_ && hop % FB_BK == 0;
    return !dev_knob("PVQ_NO_FUSE", 0) && nb_max <= (size_t)CB_MAX_NB && groups.size() <= 8 && hop % (use_bf ? FB_BK : 64) == 0;
}

bool Vqt::blockdft_applicable(size_t hop) const { return has_device() && blockdft_plan_applicable(plan_, hop); }

// a host table to the device; D is the HIP type the kernels read, H the planner's plain struct of the same layout
template <typename D, typename H>
static bool up(D** dst, const std::vector<H>& src) {
    static_assert(sizeof(D) == sizeof(H) && alignof(D) == alignof(H), "device and host element types differ");
    if (hipMalloc(reinterpret_cast<void**>(dst), sizeof(H) * std::max<size_t>(src.size(), 1)) != hipSuccess) return false;
    if (!src.empty() && hipMemcpy(*dst, src.data(), sizeof(H) * src.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
    return true;
}

pvq_status Vqt::prepare_blockdft(size_t hop) {
    if (dev_->block && dev_->block->hop == hop) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));   // the tables live on the handle's device, whatever device the calling thread has current
    if (dev_->block) {
        free_blockdft_tables(dev_->block);
        dev_->block = nullptr;
    }
    BlockDftHostTables h;
    std::string err;
    if (!build_blockdft_tables(plan_, hop, twiddle_fp16_, h, &err)) {
        set_last_error(err);
        return PVQ_ERR_UNSUPPORTED;
    }
    auto* t = new BlockDftTables();
    t->hop = hop;
    t->n_groups = (int)h.groups.size();
    t->n_tiles = h.n_tiles;
    t->nb_max = h.nb_max;
    t->n_bins_pad = h.n_bins_pad;
    t->general = h.general;
    t->band_per_wave = h.band_per_wave;
    t->band_waves = h.band_waves;
    t->band_per_wave8 = h.band_per_wave8;
    t->band_stage_stride8 = h.band_stage_stride8;
    std::copy(h.band_stage_count8, h.band_stage_count8 + 8, t->band_stage_count8);
    h.E16.insert(h.E16.end(), h.E16M.begin(), h.E16M.end());   // the mixed tiles' merged slices: column tiles n_tiles ... of the device's E16
    t->mixed = h.mixed;
    const bool ok = up(&t->d_E16R, h.E16R) && up(&t->d_gen_tw, h.gen_tw) && up(&t->d_E, h.E) && up(&t->d_tile_group, h.tile_group) && up(&t->d_tile_s, h.tile_s) &&
                    up(&t->d_groups, h.groups) && up(&t->d_comb_tw, h.comb_tw) && up(&t->d_band, h.band) && up(&t->d_band_B, h.band_B) && up(&t->d_band_list, h.band_list) &&
                    up(&t->d_band8, h.band8) && up(&t->d_band_B4, h.band_B4) && up(&t->d_band_list8, h.band_list8) && up(&t->d_band_stages8, h.band_stages8) && up(&t->d_band_B3, h.band_B3) && up(&t->d_E16, h.E16);
    if (!ok) {
        free_blockdft_tables(t);
        set_last_error("hipMalloc/hipMemcpy failed while building block-DFT tables");
        return PVQ_ERR_DEVICE;
    }
    t->groups = std::move(h.groups);
    t->h_E = std::move(h.E);  // kept for the lazily built bf16 planes
    dev_->block = t;
    return PVQ_OK;
}

// Every kernel of a sub-batch runs on the caller's stream; peaks once over the whole batch.  (A two-stream
// variant that overlapped the GEMM of sub-batch c+1 with the memory-bound stages of c was measured slower:
// the streams contend for the same CUs.)
pvq_status Vqt::launch_blockdft_path(const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames, float* d_out_db,
                                     float* d_out_cplx, const PeakParamsDev* pk, hipStream_t stream) {
    const StreamRun one{d_pcm, n_lead + hop, n_lead + n_frames * hop, n_frames, 0, 1};
    return launch_blockdft_streams(&one, 1, hop, d_out_db, d_out_cplx, n_frames, pk, stream);
}

// the X (+ Y, P) workspaces for the largest of the call's launches, and the split-bf16 GEMM's E^T planes on first use
pvq_status Vqt::grow_blockdft_workspaces(const std::vector<LaunchShape>& shapes, size_t rows_cap, bool fused, bool use_bf, hipStream_t stream) {
    BlockDftTables* t = dev_->block;
    const int ntot = t->n_tiles * GM_BN, xcp = t->n_tiles * CB_C + X_PAD_COLS;
    size_t x_tiles = 1, y_tiles = 1;
    for (const LaunchShape& s : shapes) {
        x_tiles = std::max(x_tiles, s.x_tiles);
        y_tiles = std::max(y_tiles, s.y_tiles);
    }
    const size_t x_bytes = x_tiles * (size_t)xcp * 64 * sizeof(float2);
    bool grown = false;
    pvq_status s = grow(&t->d_X, &t->x_cap, x_bytes, &grown);
    if (s != PVQ_OK) return s;
    if (grown) PVQ_HIP(hipMemsetAsync(t->d_X, 0, x_bytes, stream));   // (the pad columns stay zero: no kernel writes them)
    if (fused && (t->nb_max > 64 || t->general))   // (general hops: the remainder GEMM's results, laid out like X)
        if ((s = grow(&t->d_Y, &t->y_cap, y_tiles * (size_t)xcp * 64 * sizeof(float2))) != PVQ_OK) return s;
    if (!fused)
        if ((s = grow(&t->d_P, &t->p_cap, rows_cap * ntot * sizeof(float))) != PVQ_OK) return s;
    if (use_bf && fused && !t->d_Et) {
        const std::vector<uint16_t> Et = build_Et_bf16x3(t->h_E, ntot, t->hop);
        PVQ_HIP(hipMalloc(reinterpret_cast<void**>(&t->d_Et), Et.size() * 2));
        PVQ_HIP(hipMemcpy(t->d_Et, Et.data(), Et.size() * 2, hipMemcpyHostToDevice));
    }
    return PVQ_OK;
}

// The same path over MANY streams (pvq_vqt_*_streams).  Every stream is cut into runs of at most one sub-batch; runs are packed
// into launches up to the sub-batch size (the workspace limit), so 64 streams of 2 048 frames are ONE launch per stage where a
// loop over single-stream calls pays 64 ramps and tails per stage; a long stream still runs sub-batch by sub-batch, alone in
// its launches, exactly as through the single-stream entry point.  Stream s writes its rows to out rows st[s].out_row0 ...
pvq_status Vqt::launch_blockdft_streams(const StreamRun* st, size_t n_st, size_t hop, float* d_out_db, float* d_out_cplx, size_t rows_total,
                                        const PeakParamsDev* pk, hipStream_t stream) {
    pvq_status pst = prepare_blockdft(hop);
    if (pst != PVQ_OK) return pst;
    BlockDftTables* t = dev_->block;
    const int ntot = t->n_tiles * GM_BN, xcp = t->n_tiles * CB_C + X_PAD_COLS;
    // the launches' base pointer: the lowest stream pointer (segment offsets are counted from it, in samples)
    const float* pcm_min = nullptr;
    const std::vector<BdStream> streams = rebase_runs(st, n_st, &pcm_min);
    size_t longest = 0, total_frames = 0;
    for (const BdStream& S : streams) {
        longest = std::max(longest, S.n_frames);
        total_frames += S.n_frames;
    }
    const size_t chunk = std::min(n_st == 1 ? longest : std::max<size_t>((total_frames + 63) / 64 * 64, 64),
                                  chunk_frames(workspace_limit_, (size_t)xcp * sizeof(float2) * (t->nb_max > 64 ? 2 : 1)));
    const bool use_bf = gemm_split_bf16_ && hop % FB_BK == 0 && !t->general;   // (a general hop runs the fp32 GEMM whatever the setting; the kernel product follows the setting)
    static const bool fuse_env = !dev_knob("PVQ_NO_FUSE", 0);
    const bool fused = t->general || (fuse_env && t->nb_max <= CB_MAX_NB && t->n_groups <= 8 && hop % (use_bf ? FB_BK : 64) == 0);
    if (!fused && n_st > 1) {
        set_last_error("internal: the unfused block-DFT stages take one stream per call");
        return PVQ_ERR_INTERNAL;
    }
    const std::vector<std::vector<BdRun>> launches = pack_runs(streams.data(), n_st, chunk);
    std::vector<LaunchShape> shapes;
    for (const auto& runs : launches) shapes.push_back(launch_shape(streams.data(), runs, hop, plan_.params.n_fft, t->nb_max));
    const size_t rows_cap = chunk + t->nb_max - 1;
    if ((pst = grow_blockdft_workspaces(shapes, rows_cap, fused, use_bf, stream)) != PVQ_OK) return pst;
    for (size_t i = 0; i < launches.size(); ++i) {
        const LaunchShape& sh = shapes[i];
        const bool multi = launches[i].size() > 1 || sh.strided;
        BlockLaunch L{&sh, &launches[i], streams.data(), use_bf, multi, multi ? pcm_min : pcm_min + sh.segs[0].pcm_off,
                      multi ? sh.x_tiles * 64 : (size_t)sh.segs[0].nf, rows_cap, ntot, xcp, nullptr};
        if (fused) {
            if ((pst = launch_blockdft_gemm_fused(L, stream)) != PVQ_OK) return pst;
            if (t->nb_max > 64) launch_blockdft_tree_finish(L, stream);
        } else
            launch_blockdft_gemm_unfused(L, stream);
        if ((pst = launch_blockdft_dots(L, d_out_db, d_out_cplx, stream)) != PVQ_OK) return pst;
        last_frames_per_launch_ = (uint32_t)sh.n_frames;
    }
    if (pk) {
        pvq_status ps = peaks_stage(d_out_db, rows_total, *pk, stream);
        if (ps != PVQ_OK) return ps;
    }
    PVQ_HIP(hipGetLastError());
    last_algo_ = PVQ_ALGO_BLOCKDFT;
    if (n_st == 1) last_frames_per_launch_ = (uint32_t)chunk;
    return PVQ_OK;
}

}  // namespace pvq
