// fft_path.hip — the FFT path of the batched VQT for MI355X (gfx950 / CDNA4): kernels and launchers.
//
// Hot path being replaced: Vqt::calculate_vqt_instant_in_db (reference
// pitchvis_analysis/src/vqt.rs:866-916) and power_to_db (:922-954), batched over hops.
//
// Kernel inventory (wave64, LDS-staged, no compatibility layers):
//   vqt_fft_frames<BLOCK, E, T>  the walk: a workgroup per BLOCK / T frames.  Per window group: gather the window from the
//                           hop stream, an in-place register-staged Stockham FFT (radix 16/8/4/2)
//                           of the packed real window in padded LDS, real-split of only the
//                           columns the sparse kernel reads, banded complex row dots reduced with
//                           16-lane shuffles; then the frame-relative dB epilogue.  Few frames: a workgroup per window
//                           group (FftArgs::xv_split), the frames finished by db_rows.
//   vqt_fft_group<N, BLOCK>      batches: one instantiation per window size, a launch per window group, rows of x_vqt out
//   db_rows<T>                   x_vqt rows of a group-split launch -> frame-relative dB
//   db_rows_batch<T>             the same behind vqt_fft_group, output rows by stream
// Launchers: Vqt::launch_fft_path, launch_fft_streams (which form), launch_fft_groups, launch_fft_walk.  FftStream, FftArgs: fft_path.hpp.
#include "vqt_engine.hpp"

#include <algorithm>
#include <string>
#include <type_traits>

#include "fft_path.hpp"

// Every floating-point operation of this file rounds where it is written: no implicit FMA contraction.  The FFT path exists in several forms —
// the walk (vqt_fft_frames, any window at run time, for four thread counts), its group-split launch for few frames, and one kernel per window
// size for batches (vqt_fft_group) — and a frame must have the same bits whichever form computed it (a stream's values do not depend on the size
// of the batch it is analysed in).  Left to contract on its own, the compiler fuses a product into a neighbouring addition or not depending on the
// code around it: the same source, inlined into two kernels, rounded differently in 94 % of the coefficients (1.4e-7 of the frame peak;
// profiles/r05_fft_path.txt).  Where a fused multiply-add is wanted it is written (fmaf): the same instructions in every form, by construction.
#pragma clang fp contract(off)

namespace pvq {

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {   // two products, two fused multiply-adds
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// LDS padding: one float2 of padding after every 16, so that radix-16 strided writes
// (stride 16 elements = 128 B) land on distinct banks within each 16-lane ds_write_b64 group.
__device__ __forceinline__ int lpad(int i) { return i + (i >> 4); }

// cos/sin(2*pi*k/16), k = 0..7
__device__ constexpr float kC16[8] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f,
                                      0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f};
__device__ constexpr float kS16[8] = {0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f,
                                      1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f};

// In-register forward DFT of R points (natural order in and out), decimation in time.
template <int R>
struct RegFft;

template <int R, int K>
struct RegBfly {
    static __device__ __forceinline__ void run(float2* u, const float2* e, const float2* o) {
        constexpr int idx = K * (16 / R);  // twiddle exp(-2*pi*i*idx/16)
        float2 t;
        if constexpr (idx == 0) {
            t = o[K];
        } else if constexpr (idx == 4) {
            t = make_float2(o[K].y, -o[K].x);  // * (-i)
        } else {
            t = cmul(o[K], make_float2(kC16[idx], -kS16[idx]));
        }
        u[K] = cadd(e[K], t);
        u[K + R / 2] = csub(e[K], t);
        if constexpr (K + 1 < R / 2) RegBfly<R, K + 1>::run(u, e, o);
    }
};

template <>
struct RegFft<1> {
    static __device__ __forceinline__ void run(float2*) {}
};
template <>
struct RegFft<2> {
    static __device__ __forceinline__ void run(float2* u) {
        float2 a = u[0], b = u[1];
        u[0] = cadd(a, b);
        u[1] = csub(a, b);
    }
};
template <int R>
struct RegFft {
    static __device__ __forceinline__ void run(float2* u) {
        float2 e[R / 2], o[R / 2];
#pragma unroll
        for (int k = 0; k < R / 2; ++k) {
            e[k] = u[2 * k];
            o[k] = u[2 * k + 1];
        }
        RegFft<R / 2>::run(e);
        RegFft<R / 2>::run(o);
        RegBfly<R, 0>::run(u, e, o);
    }
};

// One in-place Stockham autosort pass of radix R over N points living in padded LDS.
//   item i in [0, N/R): k = i mod p, u[r] = Z[i + r*N/R] * w_{pR}^{k r}, DFT_R, Z[(i-k)R + k + r p] = u[r]
// Every thread first pulls all of its inputs into registers, the workgroup synchronises, then the
// outputs go back into the same buffer: one LDS buffer serves any N <= E*BLOCK.
template <int R, int BLOCK, int E>
__device__ __forceinline__ void stockham_pass(float2* __restrict__ Z, int N, int p, const float2* __restrict__ tw,
                                              int tw_stride, int tid) {
    constexpr int NB = E / R;  // butterflies a thread may own
    const int T = N / R;
    float2 u[NB][R];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tid + b * BLOCK;
        if (i < T) {
#pragma unroll
            for (int r = 0; r < R; ++r) u[b][r] = Z[lpad(i + r * T)];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tid + b * BLOCK;
        if (i < T) {
            if (p > 1) {
                const int k = i & (p - 1);
                const int base = k * tw_stride;
#pragma unroll
                for (int r = 1; r < R; ++r) u[b][r] = cmul(u[b][r], tw[base * r]);
            }
            RegFft<R>::run(u[b]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tid + b * BLOCK;
        if (i < T) {
            const int k = i & (p - 1);
            const int j = (i - k) * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) Z[lpad(j + r * p)] = u[b][r];
        }
    }
    __syncthreads();
}

// Output-pruned pass.  The kernel reads only the spectrum columns 0 .. M of a window group (vqt.rs:725-735 bounds them by the
// decimated Nyquist), i.e. FFT bins 0 .. M and N - M .. N - 1 (the real split pairs c with N - c).  An output o of the pass with
// stride p lands in residue k + r p of o mod p R (k = i mod p), and a later pass only moves it within that residue class of ITS
// p' = p R — so the bins the kernel needs descend from the outputs with k + r p <= M or k + r p >= p R - M.  Once M < p that leaves
// r = 0 (for k <= M) and r = R - 1 (for k >= p - M) of an item, and nothing at all of the items in between: two of R outputs
// computed and written (out[0] = sum u_r, out[R-1] = sum u_r e^{+2 pi i r / R}), the other items not even loaded.  At 48 kHz /
// 252 bins that is the last two of the 16 384-sample window's four passes (an LDS pass moves all N points whatever its radix).
template <int R, int BLOCK, int E>
__device__ __forceinline__ void stockham_pass_ends(float2* __restrict__ Z, int N, int p, const float2* __restrict__ tw, int tw_stride, int tid, int M) {
    constexpr int NB = E / R;
    const int T = N / R;
    float2 lo[NB], hi[NB];
    bool nl[NB], nh[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tid + b * BLOCK;
        const int k = i & (p - 1);
        nl[b] = i < T && k <= M;
        nh[b] = i < T && k >= p - M;
        lo[b] = make_float2(0.0f, 0.0f);
        hi[b] = lo[b];
        if (nl[b] || nh[b]) {
            float2 u[R];
#pragma unroll
            for (int r = 0; r < R; ++r) u[r] = Z[lpad(i + r * T)];
            const int base = k * tw_stride;   // (p > M >= 0: never the first pass, the twiddles apply)
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[base * r]);
            float2 s0 = u[0], s1 = u[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                constexpr int step = 16 / R;
                const int idx = r * step;   // e^{+2 pi i idx / 16}
                const float c = idx < 8 ? kC16[idx] : -kC16[idx - 8], sn = idx < 8 ? kS16[idx] : -kS16[idx - 8];
                s0 = cadd(s0, u[r]);
                s1 = cadd(s1, cmul(u[r], make_float2(c, sn)));
            }
            lo[b] = s0;
            hi[b] = s1;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tid + b * BLOCK;
        const int k = i & (p - 1);
        const int j = (i - k) * R + k;
        if (nl[b]) Z[lpad(j)] = lo[b];
        if (nh[b]) Z[lpad(j + (R - 1) * p)] = hi[b];
    }
    __syncthreads();
}

// Forward FFT of N = 2^logN complex points in padded LDS (natural order in and out); only the bins 0 .. M and N - M .. N - 1 are
// guaranteed on return (M >= N / 2: all of them).
template <int BLOCK, int E>
__device__ __forceinline__ void lds_fft(float2* Z, int N, const float2* tw, int n_tw, int tid, int M) {
    int p = 1;
    int rem = N;
    while (rem >= 16) {
        if (M < p) stockham_pass_ends<16, BLOCK, E>(Z, N, p, tw, n_tw / (p * 16), tid, M);
        else stockham_pass<16, BLOCK, E>(Z, N, p, tw, n_tw / (p * 16), tid);
        p *= 16;
        rem >>= 4;
    }
    if (rem == 8) {
        if (M < p) stockham_pass_ends<8, BLOCK, E>(Z, N, p, tw, n_tw / (p * 8), tid, M);
        else stockham_pass<8, BLOCK, E>(Z, N, p, tw, n_tw / (p * 8), tid);
    } else if (rem == 4) {
        if (M < p) stockham_pass_ends<4, BLOCK, E>(Z, N, p, tw, n_tw / (p * 4), tid, M);
        else stockham_pass<4, BLOCK, E>(Z, N, p, tw, n_tw / (p * 4), tid);
    } else if (rem == 2) {
        if (M < p) stockham_pass_ends<2, BLOCK, E>(Z, N, p, tw, n_tw / (p * 2), tid, M);
        else stockham_pass<2, BLOCK, E>(Z, N, p, tw, n_tw / (p * 2), tid);
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// vqt.rs:922-954 constants
#define PVQ_REF_POWER (0.3f * 0.3f)
#define PVQ_A_MIN (1e-6f * 1e-6f)
#define PVQ_TOP_DB 60.0f

// Frame-relative dB epilogue shared by both algorithm paths.  xv: n_bins complex coefficients in
// LDS; red: 2*(BLOCK/64) floats of LDS scratch.  Writes n_bins floats to out (global).
// status: the handle's sticky flag word; bit 0 is raised when a coefficient of the frame is not finite (a NaN / Inf sample
// in the frame's windows: the reference's callers drop such input, audio_desktop.rs:102-105, and peak_detection.rs:145
// would panic on it).  T threads (T / 64 waves) share one frame; `red` holds that frame's 2 * T / 64 partial results; the
// barrier is the workgroup's (every frame of a workgroup runs the epilogue at the same time); live = false: a padding
// frame, nothing is stored.
template <int T>
__device__ __forceinline__ void db_epilogue(const float2* xv, float* red, int n_bins, float* __restrict__ out,
                                            float* lds_out, int tid, unsigned* status, bool live = true) {
    const float ref_db = 10.0f * log10f(PVQ_REF_POWER);
    constexpr int NW = T / 64;
    constexpr int PER = 1024 / T < 4 ? 4 : 1024 / T;  // supports n_bins <= max(1024, 4 T): fft_db_threads() picks T
    float d[PER];
    float mx = -3.40282347e+38f, mn = 3.40282347e+38f;
    bool bad = false;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int k = tid + t * T;
        d[t] = 0.0f;
        if (k < n_bins) {
            const float2 z = xv[k];
            const float ns = fmaf(z.x, z.x, z.y * z.y);
            bad |= !(ns <= 3.40282347e+38f);
            d[t] = 10.0f * log10f(fmaxf(ns, PVQ_A_MIN)) - ref_db;
            mx = fmaxf(mx, d[t]);
            mn = fminf(mn, d[t]);
        }
    }
    mx = wave_max(mx);
    mn = wave_min(mn);
    if (status && live && __builtin_amdgcn_ballot_w64(bad) != 0 && (tid & 63) == 0) atomicOr(status, 1u);
    if ((tid & 63) == 0) {
        red[tid >> 6] = mx;
        red[NW + (tid >> 6)] = mn;
    }
    __syncthreads();
    mx = red[0];
    mn = red[NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        mx = fmaxf(mx, red[w]);
        mn = fminf(mn, red[NW + w]);
    }
    const float floor_db = mx - PVQ_TOP_DB;
    mn = fmaxf(mn, floor_db);
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int k = tid + t * T;
        if (k < n_bins && live) {
            const float c = fmaxf(d[t], floor_db);
            const float r = (mn > 0.0f) ? (c - mn) : fmaxf(c, 0.0f);
            out[k] = r;
            if (lds_out) lds_out[k] = r;
        }
    }
}

// threads per frame the dB epilogue needs for n_bins (PER * T >= n_bins): the forms up to 1024 bins keep their own T; beyond, 512
// threads cover 2 048 bins and 1 024 threads 4 096 (FFT_MAX_BINS, the most any form covers).  Same bits for every T: a bin's dB is
// computed alone, the frame's max / min are exact.
constexpr int FFT_MAX_BINS = 4096;
constexpr size_t FFT_MAX_LDS = 160 * 1024;   // a workgroup's LDS on gfx950
__host__ __device__ constexpr int fft_db_threads(int T, int n_bins) {
    return n_bins <= (1024 / T < 4 ? 4 * T : 1024) ? T : n_bins <= 2048 ? (T > 512 ? T : 512) : 1024;
}

// ------------------------------------------------------------------------------------------------
// The walk: gather, FFT, real split, row dots and dB fused, a workgroup per BLOCK / T frames (FftStream, FftArgs: fft_path.hpp)
// ------------------------------------------------------------------------------------------------
// T threads per frame, F = BLOCK / T frames per workgroup side by side: a 4096-sample window is a 2048-point complex FFT =
// 128 radix-16 butterflies per pass, so a whole 512-thread workgroup on one frame leaves three quarters of its threads idle
// through every pass (the trainer's geometry, pitchvis_train/src/train.rs:30-43: 13 M frames/s that way).  All frames of a
// workgroup walk the same window groups in step, so the barriers inside the FFT passes stay the workgroup's.  The real split
// writes the spectrum columns the kernel reads in place of the FFT output (column c and N - c come from the same pair of
// FFT bins, so one thread computes both and nothing else touches that pair): no separate spectrum buffer, 19 KB of LDS per
// frame at that geometry instead of 27, eight frames in flight per CU.
template <int BLOCK, int E, int T>
__global__ __launch_bounds__(BLOCK, 4) void vqt_fft_frames(FftArgs a) {   // four waves per SIMD: two 512-thread workgroups per CU
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int F = BLOCK / T;
    const int tid = threadIdx.x, tl = tid % T, fl = tid / T;
    const int zlen = lpad(a.n_tw) + 1;          // FFT buffer of the largest window, + the slot of its Nyquist column
    const int per_frame = zlen + a.n_bins;      // complex slots per frame
    float2* Z = reinterpret_cast<float2*>(smem) + (size_t)fl * per_frame;
    float2* xv = Z + zlen;
    float* red = reinterpret_cast<float*>(reinterpret_cast<float2*>(smem) + (size_t)F * per_frame) + fl * 2 * (T / 64);

    // (split: every frame's largest window first, then the next — workgroups start in index order, the long ones must not come last)
    const int fg_step = a.xv_split ? (int)(gridDim.x / a.n_groups) : (int)gridDim.x;
    const int g_only = a.xv_split ? (int)(blockIdx.x / fg_step) : -1;
    const int fg0 = a.xv_split ? (int)(blockIdx.x % fg_step) : (int)blockIdx.x;
    for (int fg = fg0; fg * F < a.n_frames; fg += fg_step) {
        const bool live = fg * F + fl < a.n_frames;
        const int gframe = live ? fg * F + fl : a.n_frames - 1;   // a padding frame repeats the last one and stores nothing
        // the frame's stream (wave-uniform: T >= 64 threads share a frame)
        const float* pcm = a.pcm;
        long long n_lead = a.n_lead, n_samples = a.n_samples, frame = gframe, out_row = gframe;
        if (a.streams) {
            int lo = 0, n = a.n_streams;   // the last stream whose first frame is at or before gframe
            while (n > 1) {
                const int h = n >> 1;
                if (a.streams[lo + h].frame0 <= gframe) { lo += h; n -= h; } else n = h;
            }
            const FftStream st = a.streams[lo];
            pcm = st.pcm;
            n_lead = st.n_lead;
            n_samples = st.n_samples;
            frame = gframe - st.frame0;
            out_row = st.row0 + frame;
        }
        // x[j] of the reference's n_fft buffer is pcm[buf0 + j]; zeros before the stream start
        const long long buf0 = n_lead + (frame + 1) * a.hop - a.n_fft;

        for (int g = 0; g < a.n_groups; ++g) {
            if (g_only >= 0 && g != g_only) continue;   // (uniform)
            const GroupDev G = a.groups[g];
            const int N = G.n_cplx;
            // gather the window: Z[n] = (x[w0 + 2n], x[w0 + 2n + 1]): one 8-byte load (the stream's samples are 4-byte aligned, whatever the
            // hop) and one 8-byte LDS store per complex point, eight loads in flight per thread; zeros before the stream start
            {
                struct __attribute__((packed, aligned(4))) F2U { float x, y; };
                const long long s0 = buf0 + G.w0;
                for (int n0 = tl; n0 < N; n0 += 8 * T) {
                    float2 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int n = n0 + u * T;
                        const long long sx = s0 + 2 * n;
                        v[u] = make_float2(0.0f, 0.0f);
                        if (n < N) {
                            if (sx >= 0 && sx + 1 < n_samples) {
                                const F2U t = *reinterpret_cast<const F2U*>(pcm + sx);
                                v[u] = make_float2(t.x, t.y);
                            } else {
                                if (sx >= 0 && sx < n_samples) v[u].x = pcm[sx];
                                if (sx + 1 >= 0 && sx + 1 < n_samples) v[u].y = pcm[sx + 1];
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int n = n0 + u * T;
                        if (n < N) Z[lpad(n)] = v[u];
                    }
                }
            }
            __syncthreads();
            if (!(a.dev_skip & 2)) lds_fft<T, E>(Z, N, a.tw, a.n_tw, tl, (a.dev_skip & 4) ? N : G.n_cols - 1);   // (PVQ_FFT_SKIP=4: unpruned, for A/B)
            // real split, in place, only for the columns the kernel reads (c <= n_cols - 1 <= N): columns c and d = N - c
            // are both made of FFT bins c and N - c
            for (int c = tl; c <= N / 2; c += T) {
                const int d = N - c;
                const bool need_c = c < G.n_cols, need_d = d < G.n_cols && d != c;
                if (!need_c && !need_d) continue;
                const float2 zc = Z[lpad(c & (N - 1))], zd = Z[lpad(d & (N - 1))];
                auto column = [&](float2 za, float2 zb, int col) {   // za = Z[col], zb = conj(Z[N - col])
                    zb.y = -zb.y;
                    const float2 w = a.split_tw[G.split_off + col];
                    const float2 ev = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y + zb.y));
                    const float2 dv = make_float2(0.5f * (za.x - zb.x), 0.5f * (za.y - zb.y));
                    const float2 t = cmul(w, dv);
                    return make_float2(ev.x + t.y, ev.y - t.x);
                };
                float2 sc = make_float2(0.0f, 0.0f), sd = sc;
                if (need_c) sc = column(zc, zd, c);
                if (need_d) sd = column(zd, zc, d);
                if (need_c) Z[lpad(c)] = sc;
                if (need_d) Z[lpad(d)] = sd;   // d = N (the Nyquist column, from FFT bin 0) lands in the slot behind the buffer
            }
            __syncthreads();
            // banded complex row dots (vqt.rs:889-910), the whole workgroup over all its frames: a team of G.tpr lanes
            // walks one kernel row, every entry is fetched once (one 16-byte load) and applied to the F frames' spectra
            {
                const int tpr = G.tpr;
                const int team = tid / tpr, tm = tid & (tpr - 1), n_teams = BLOCK / tpr;
                const uint32_t* rp = a.row_ptr + G.row_ptr_off;
                const float2* Z0 = reinterpret_cast<const float2*>(smem);
                float2* xv0 = reinterpret_cast<float2*>(smem) + zlen;
                for (int row = team; row < G.n_rows && !(a.dev_skip & 1); row += n_teams) {
                    const int s = G.ent_off + rp[row], e = G.ent_off + rp[row + 1];
                    float2 acc[F];
#pragma unroll
                    for (int f = 0; f < F; ++f) acc[f] = make_float2(0.0f, 0.0f);
                    for (int i = s + tm; i < e; i += tpr) {
                        const float4 en = a.ent[i];
                        const uint32_t c = __builtin_bit_cast(uint32_t, en.z);
                        const int idx = lpad(c & 0x7fffu);
                        const float sg = (c & 0x8000u) ? -1.0f : 1.0f;
#pragma unroll
                        for (int f = 0; f < F; ++f) {
                            float2 x = Z0[(size_t)f * per_frame + idx];
                            x.y *= sg;
                            acc[f].x = fmaf(-en.y, x.y, fmaf(en.x, x.x, acc[f].x));
                            acc[f].y = fmaf(en.y, x.x, fmaf(en.x, x.y, acc[f].y));
                        }
                    }
                    for (int o = tpr >> 1; o > 0; o >>= 1) {
#pragma unroll
                        for (int f = 0; f < F; ++f) {
                            acc[f].x += __shfl_xor(acc[f].x, o);
                            acc[f].y += __shfl_xor(acc[f].y, o);
                        }
                    }
                    if (tm == 0) {
#pragma unroll
                        for (int f = 0; f < F; ++f) xv0[(size_t)f * per_frame + G.first_bin + row] = acc[f];
                    }
                }
            }
            __syncthreads();   // the next group's gather overwrites the spectrum columns
        }
        if (g_only >= 0) {   // this group's rows of x_vqt; db_rows takes the frame from there
            const GroupDev G = a.groups[g_only];
            if (live)
                for (int k = tl; k < G.n_rows; k += T) a.xv_split[(size_t)out_row * a.n_bins + G.first_bin + k] = xv[G.first_bin + k];
            __syncthreads();
            continue;
        }
        if (a.out_cplx && live) {
            for (int k = tl; k < a.n_bins; k += T) a.out_cplx[(size_t)out_row * a.n_bins + k] = xv[k];
        }
        db_epilogue<T>(xv, red, a.n_bins, a.out_db + (size_t)out_row * a.n_bins, nullptr, tl, a.status, live);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// The FFT path for BATCHES (round 5): one kernel instantiation per window size.  vqt_fft_frames above takes any window at run time:
// every LDS address of its Stockham passes is computed from N, p and the thread's item (lpad, masks, multiplies), and of the ~330
// vector instructions it spends per radix-16 item and pass two thirds are that index arithmetic.  Here N, the pass stride P and the
// threads per frame T = N / 16 are template parameters: an item's 16 reads and 16 writes are ONE base address plus immediates, the
// pass chain is unrolled, and a workgroup serves one window group (the launch is per group, as the few-frames form of the kernel
// above already is: rows of x_vqt through `xv_split`, db_rows finishes the frames).  The arithmetic is the walk's — the same twiddle
// table entries, the same cmul and RegFft<R>, the same pass radices and pruning, the same real split and row dots with the same
// lanes-per-row — so a frame's bits are what vqt_fft_frames gives (tests/test_configs_gpu.py::test_fft_batch_kernels_equal_the_walk_in_subprocesses).
// ------------------------------------------------------------------------------------------------
template <int R, int N, int P, int T>
__device__ __forceinline__ void stockham_pass_ct(float2* __restrict__ Z, const float2* __restrict__ tw, int n_tw, int tl) {
    constexpr int NB = 16 / R;            // items per thread: NB * T = N / R exactly
    constexpr int TI = N / R;             // items of the pass
    static_assert(TI % 16 == 0 && NB * T == TI, "pass geometry");
    constexpr int LTI = TI + TI / 16;     // lpad(i + r TI) = lpad(i) + r LTI
    float2 u[NB][R];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float2* zi = Z + lpad(tl + b * T);
#pragma unroll
        for (int r = 0; r < R; ++r) u[b][r] = zi[r * LTI];
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (P > 1) {
            const int k = (tl + b * T) & (P - 1);
            const int base = k * (n_tw / (P * R));
#pragma unroll
            for (int r = 1; r < R; ++r) u[b][r] = cmul(u[b][r], tw[base * r]);
        }
        RegFft<R>::run(u[b]);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tl + b * T;
        const int k = i & (P - 1);
        const int j = (i - k) * R + k;
        if (P >= 16) {   // lpad(j + r P) = lpad(j) + r (P + P / 16)
            float2* zj = Z + lpad(j);
#pragma unroll
            for (int r = 0; r < R; ++r) zj[r * (P + P / 16)] = u[b][r];
        } else {         // the first pass (P = 1, R = 16): j = 16 i, lpad(j + r) = 17 i + r
            static_assert(P >= 16 || (P == 1 && R == 16), "first pass");
            float2* zj = Z + 17 * i;
#pragma unroll
            for (int r = 0; r < R; ++r) zj[r] = u[b][r];
        }
    }
    __syncthreads();
}
template <int R, int N, int P, int T>
__device__ __forceinline__ void stockham_pass_ends_ct(float2* __restrict__ Z, const float2* __restrict__ tw, int n_tw, int tl, int M) {
    constexpr int NB = 16 / R;
    constexpr int TI = N / R;
    constexpr int LTI = TI + TI / 16;
    static_assert(P >= 16, "a pruned pass is never the first");
    float2 lo[NB], hi[NB];
    bool nl[NB], nh[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tl + b * T;
        const int k = i & (P - 1);
        nl[b] = k <= M;
        nh[b] = k >= P - M;
        lo[b] = make_float2(0.0f, 0.0f);
        hi[b] = lo[b];
        if (nl[b] || nh[b]) {
            float2 u[R];
            const float2* zi = Z + lpad(i);
#pragma unroll
            for (int r = 0; r < R; ++r) u[r] = zi[r * LTI];
            const int base = k * (n_tw / (P * R));
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[base * r]);
            float2 s0 = u[0], s1 = u[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                constexpr int step = 16 / R;
                const int idx = r * step;   // e^{+2 pi i idx / 16}
                const float c = idx < 8 ? kC16[idx] : -kC16[idx - 8], sn = idx < 8 ? kS16[idx] : -kS16[idx - 8];
                s0 = cadd(s0, u[r]);
                s1 = cadd(s1, cmul(u[r], make_float2(c, sn)));
            }
            lo[b] = s0;
            hi[b] = s1;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = tl + b * T;
        const int k = i & (P - 1);
        float2* zj = Z + lpad((i - k) * R + k);
        if (nl[b]) zj[0] = lo[b];
        if (nh[b]) zj[(R - 1) * (P + P / 16)] = hi[b];
    }
    __syncthreads();
}
// the pass chain of lds_fft for a compile-time N: radix 16 while 16 or more points remain, then one pass of radix 8, 4 or 2
template <int N, int P, int T>
__device__ __forceinline__ void lds_fft_ct(float2* Z, const float2* tw, int n_tw, int tl, int M) {
    constexpr int REM = N / P;
    if constexpr (REM >= 16) {
        if (M < P) {
            if constexpr (P >= 16) stockham_pass_ends_ct<16, N, P, T>(Z, tw, n_tw, tl, M);
        } else {
            stockham_pass_ct<16, N, P, T>(Z, tw, n_tw, tl);
        }
        lds_fft_ct<N, P * 16, T>(Z, tw, n_tw, tl, M);
    } else if constexpr (REM > 1) {
        if (M < P) stockham_pass_ends_ct<REM, N, P, T>(Z, tw, n_tw, tl, M);
        else stockham_pass_ct<REM, N, P, T>(Z, tw, n_tw, tl);
    }
}

template <int N, int BLOCK>   // N complex points (a window of 2 N samples), T = N / 16 threads per frame, F = BLOCK / T frames per workgroup side by side
__global__ __launch_bounds__(BLOCK, 4) void vqt_fft_group(FftArgs a, int g, int frame0, int n_frames_here) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = N / 16, F = BLOCK / T;
    constexpr int ZLEN = N + N / 16 + 1;   // lpad(N) + the slot of the Nyquist column
    const int tid = threadIdx.x, tl = tid % T, fl = tid / T;
    float2* Z = reinterpret_cast<float2*>(smem) + (size_t)fl * ZLEN;
    const GroupDev G = a.groups[g];
    {   // one group of F frames per workgroup, no loop over groups: a loop's hoisted invariants (addresses of every pass) cost registers and scratch
        const int fg = blockIdx.x;
        const bool live = fg * F + fl < n_frames_here;
        const int gframe = frame0 + (live ? fg * F + fl : n_frames_here - 1);   // a padding frame repeats the last one and stores nothing
        const float* pcm = a.pcm;
        long long n_lead = a.n_lead, n_samples = a.n_samples, frame = gframe, out_row = gframe;
        if (a.streams) {
            int lo = 0, n = a.n_streams;   // the last stream whose first frame is at or before gframe
            while (n > 1) {
                const int h = n >> 1;
                if (a.streams[lo + h].frame0 <= gframe) { lo += h; n -= h; } else n = h;
            }
            const FftStream st = a.streams[lo];
            pcm = st.pcm;
            n_lead = st.n_lead;
            n_samples = st.n_samples;
            frame = gframe - st.frame0;
            out_row = st.row0 + frame;
        }
        const long long s0 = n_lead + (frame + 1) * a.hop - a.n_fft + G.w0;
        // gather the window: Z[n] = (x[w0 + 2n], x[w0 + 2n + 1]), 16 points per thread, all loads in flight before the first LDS store
        {
            struct __attribute__((packed, aligned(4))) F2U { float x, y; };
            float2 v[16];
            if (s0 >= 0 && s0 + 2 * N <= n_samples) {   // the window lies inside the stream (all but a stream's first frames)
                const F2U* src = reinterpret_cast<const F2U*>(pcm + s0);
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const F2U t = src[tl + u * T];
                    v[u] = make_float2(t.x, t.y);
                }
            } else {
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const long long sx = s0 + 2 * (tl + u * T);
                    v[u] = make_float2(0.0f, 0.0f);
                    if (sx >= 0 && sx < n_samples) v[u].x = pcm[sx];
                    if (sx + 1 >= 0 && sx + 1 < n_samples) v[u].y = pcm[sx + 1];
                }
            }
            // (the thread's index goes through an empty asm once per frame: left to itself the compiler hoists the 15 twiddle ADDRESSES of every
            // pass — loop-invariant 64-bit values — out of the frame loop and spills them: 380 bytes of scratch per lane, reloaded in every pass)
            int tl_ = tl;
            asm volatile("" : "+v"(tl_));
            // The first pass (stride 1, radix 16, no twiddles) takes item i = tl's inputs Z[tl + r N / 16] — exactly the 16 points this thread
            // has just gathered (T = N / 16): they go through the butterfly in registers and only its outputs reach LDS.  The walk writes the
            // gathered window to LDS, meets at a barrier and reads it back: same values, 16 LDS writes, a barrier and 16 LDS reads more.
            // (n_cols > 1, checked by the host: with a single column the walk prunes even this pass)
            RegFft<16>::run(v);
            float2* zj = Z + 17 * tl_;   // lpad(16 i + r) = 17 i + r
#pragma unroll
            for (int r = 0; r < 16; ++r) zj[r] = v[r];
            __syncthreads();
            lds_fft_ct<N, 16, T>(Z, a.tw, a.n_tw, tl_, G.n_cols - 1);
        }
        // real split, in place, only for the columns the kernel reads (as in vqt_fft_frames)
        for (int c = tl; c <= N / 2; c += T) {
            const int d = N - c;
            const bool need_c = c < G.n_cols, need_d = d < G.n_cols && d != c;
            if (!need_c && !need_d) continue;
            const float2 zc = Z[lpad(c & (N - 1))], zd = Z[lpad(d & (N - 1))];
            auto column = [&](float2 za, float2 zb, int col) {   // za = Z[col], zb = conj(Z[N - col])
                zb.y = -zb.y;
                const float2 w = a.split_tw[G.split_off + col];
                const float2 ev = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y + zb.y));
                const float2 dv = make_float2(0.5f * (za.x - zb.x), 0.5f * (za.y - zb.y));
                const float2 t = cmul(w, dv);
                return make_float2(ev.x + t.y, ev.y - t.x);
            };
            float2 sc = make_float2(0.0f, 0.0f), sd = sc;
            if (need_c) sc = column(zc, zd, c);
            if (need_d) sd = column(zd, zc, d);
            if (need_c) Z[lpad(c)] = sc;
            if (need_d) Z[lpad(d)] = sd;
        }
        __syncthreads();
        // banded complex row dots: a team of G.tpr lanes walks one kernel row, every entry fetched once and applied to the F frames' spectra;
        // the sums go straight to the frames' rows of x_vqt (xv_split)
        {
            const int tpr = G.tpr;
            const int team = tid / tpr, tm = tid & (tpr - 1), n_teams = BLOCK / tpr;
            const uint32_t* rp = a.row_ptr + G.row_ptr_off;
            const float2* Z0 = reinterpret_cast<const float2*>(smem);
            for (int row = team; row < G.n_rows; row += n_teams) {
                const int s = G.ent_off + rp[row], e = G.ent_off + rp[row + 1];
                float2 acc[F];
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = make_float2(0.0f, 0.0f);
                for (int i = s + tm; i < e; i += tpr) {
                    const float4 en = a.ent[i];
                    const uint32_t c = __builtin_bit_cast(uint32_t, en.z);
                    const int idx = lpad(c & 0x7fffu);
                    const float sg = (c & 0x8000u) ? -1.0f : 1.0f;
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        float2 x = Z0[(size_t)f * ZLEN + idx];
                        x.y *= sg;
                        acc[f].x = fmaf(-en.y, x.y, fmaf(en.x, x.x, acc[f].x));
                        acc[f].y = fmaf(en.y, x.x, fmaf(en.x, x.y, acc[f].y));
                    }
                }
                for (int o = tpr >> 1; o > 0; o >>= 1) {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        acc[f].x += __shfl_xor(acc[f].x, o);
                        acc[f].y += __shfl_xor(acc[f].y, o);
                    }
                }
                if (tm == 0) {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const int fr = fg * F + f;
                        if (fr < n_frames_here) a.xv_split[(size_t)fr * a.n_bins + G.first_bin + row] = acc[f];   // (rows of the launch's frames, from frame0 on)
                    }
                }
            }
        }
    }
}

// the frames of a group-split launch: x_vqt rows -> (optional complex output), frame-relative dB; T threads per row as in the walk
template <int T>
__global__ __launch_bounds__(T) void db_rows(const float2* __restrict__ xv_rows, int n_rows, int n_bins, float* __restrict__ out_db, float2* __restrict__ out_cplx,
                                             unsigned* status) {
    __shared__ float red[2 * (T / 64)];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= n_rows) return;
    const float2* xv = xv_rows + (size_t)row * n_bins;
    if (out_cplx)
        for (int k = tid; k < n_bins; k += T) out_cplx[(size_t)row * n_bins + k] = xv[k];
    db_epilogue<T>(xv, red, n_bins, out_db + (size_t)row * n_bins, nullptr, tid, status, true);
}

// ... and of a vqt_fft_group launch: row r holds frame frame0 + r of the call, whose output row is the frame's own (one stream) or its stream's
template <int T>
__global__ __launch_bounds__(T) void db_rows_batch(const float2* __restrict__ xv_rows, int n_rows, int frame0, int n_bins, const FftStream* __restrict__ streams, int n_streams,
                                                   float* __restrict__ out_db, float2* __restrict__ out_cplx, unsigned* status) {
    __shared__ float red[2 * (T / 64)];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= n_rows) return;
    long long out_row = frame0 + r;
    if (streams) {
        const int gframe = frame0 + r;
        int lo = 0, n = n_streams;
        while (n > 1) {
            const int h = n >> 1;
            if (streams[lo + h].frame0 <= gframe) { lo += h; n -= h; } else n = h;
        }
        out_row = streams[lo].row0 + (gframe - streams[lo].frame0);
    }
    const float2* xv = xv_rows + (size_t)r * n_bins;
    if (out_cplx)
        for (int k = tid; k < n_bins; k += T) out_cplx[(size_t)out_row * n_bins + k] = xv[k];
    db_epilogue<T>(xv, red, n_bins, out_db + (size_t)out_row * n_bins, nullptr, tid, status, true);
}

pvq_status Vqt::launch_fft_path(const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames, float* d_out_db,
                                float* d_out_cplx, const PeakParamsDev* pk, hipStream_t stream) {
    return launch_fft_streams(nullptr, 0, d_pcm, n_lead, hop, n_frames, n_frames, d_out_db, d_out_cplx, pk, stream);
}

// st != nullptr: n_st streams in ONE launch (their frames numbered through; rows_total output rows for the peak stage)
pvq_status Vqt::launch_fft_streams(const void* st_table, size_t n_st, const float* d_pcm, size_t n_lead, size_t hop, size_t n_frames, size_t rows_total,
                                   float* d_out_db, float* d_out_cplx, const PeakParamsDev* pk, hipStream_t stream) {
    FftArgs a;
    a.streams = nullptr;
    a.n_streams = 0;
    if (st_table) {
        pvq_status es = ws_stage_tab_.reserve(n_st * sizeof(FftStream));
        if (es != PVQ_OK) return es;
        PVQ_HIP(hipMemcpyAsync(ws_stage_tab_.as<void>(), st_table, n_st * sizeof(FftStream), hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns)
        a.streams = ws_stage_tab_.as<FftStream>();
        a.n_streams = (int)n_st;
    }
    a.pcm = d_pcm;
    a.n_lead = (long long)n_lead;
    a.hop = (long long)hop;
    a.n_samples = (long long)(n_lead + n_frames * hop);
    a.n_fft = (int)plan_.params.n_fft;
    a.n_frames = (int)n_frames;
    a.n_groups = (int)plan_.kernel.window_groups.size();
    a.n_bins = (int)n_bins();
    a.n_tw = dev_->n_tw;
    a.max_cols = dev_->max_cols;
    a.groups = dev_->d_groups;
    a.tw = dev_->d_tw;
    a.split_tw = dev_->d_split_tw;
    a.row_ptr = dev_->d_row_ptr;
    a.ent = dev_->d_ent;
    a.out_db = d_out_db;
    a.out_cplx = reinterpret_cast<float2*>(d_out_cplx);
    a.status = dev_->d_status;
    static const int skip_env = dev_knob("PVQ_FFT_SKIP", 0);   // (developer build only: timing probes that skip stages)
    a.dev_skip = skip_env;

    // threads per frame: one radix-16 butterfly per thread and pass for the largest window; 512-thread workgroups hold
    // 512 / T frames side by side (a single frame, e.g. the streaming front end's, keeps the whole workgroup)
    const int n_tw = dev_->n_tw;
    // (more than 1 024 bins: at least as many threads as the dB epilogue needs for them, fft_db_threads)
    const int T = fft_db_threads(n_frames < 4 ? (n_tw <= 8192 ? 512 : 1024) : n_tw <= 2048 ? 128 : n_tw <= 4096 ? 256 : n_tw <= 8192 ? 512 : 1024,
                                 a.n_bins);
    const int F = (T == 1024 ? 1024 : 512) / T;
    const size_t lds = (size_t)F * (sizeof(float2) * ((size_t)(n_tw + (n_tw >> 4)) + 1 + a.n_bins) + sizeof(float) * 2 * (T / 64));
    if (a.n_bins > FFT_MAX_BINS || lds > FFT_MAX_LDS) {   // (up to 1 024 bins every form fits: 147 KB at most, 16 384-point FFTs)
        set_last_error("unsupported: the FFT path takes up to 4096 bins, and a frame's largest FFT and its bins must fit 160 KB of LDS (" +
                       std::to_string(a.n_bins) + " bins, " + std::to_string(lds) + " bytes)");
        return PVQ_ERR_UNSUPPORTED;
    }
    const int grid = (int)std::min<size_t>((n_frames + F - 1) / F, 1u << 20);
    // few frames of one stream: a workgroup per window group (FftArgs::xv_split).  Measured against the walk (profiles/r04_fft_split.txt):
    // 1 frame 47 -> 19 us at 48 kHz / 252 bins (77 -> 27 at 96 kHz / 360), ahead up to ~400 frames there (~200 at 96 kHz, ~750 at
    // 22 050 Hz / 588 bins): up to ~1 500 workgroups, beyond which the chip is full either way and the walk's one pass over LDS wins
    static const int split_env = dev_knob("PVQ_FFT_SPLIT", 1);   // (developer build: 0 = every workgroup walks its frames' groups)
    static const int split_max_env = dev_knob("PVQ_FFT_SPLIT_MAX", 1500);
    const bool split = !st_table && split_env && a.n_groups > 1 && (size_t)grid * (size_t)a.n_groups <= (size_t)split_max_env;
    a.xv_split = nullptr;
    // batches: one kernel instantiation per window size (vqt_fft_group), a launch per window group and 16 384-frame part, db_rows_batch
    // behind them.  Same bits as the walk.  (developer build: PVQ_FFT_CT=0 keeps the walk)
    static const int ct_env = dev_knob("PVQ_FFT_CT", 1);
    bool ct = ct_env && !split && !skip_env && a.n_groups >= 1 && n_frames >= 64;
    for (int g = 0; g < a.n_groups && ct; ++g) {
        const int N = dev_->h_groups[g].n_cplx;
        ct = N >= 256 && N <= 16384 && (N & (N - 1)) == 0 && dev_->h_groups[g].n_cols > 1;
    }
    const pvq_status fs = ct ? launch_fft_groups(a, n_frames, stream) : launch_fft_walk(a, T, grid, lds, split, n_frames, stream);
    if (fs != PVQ_OK) return fs;
    if (pk) {  // peak / note detection as its own launch (one wavefront per frame)
        pvq_status ps = peaks_stage(d_out_db, rows_total, *pk, stream);
        if (ps != PVQ_OK) return ps;
    }
    PVQ_HIP(hipGetLastError());
    last_algo_ = PVQ_ALGO_FFT;
    last_frames_per_launch_ = (uint32_t)n_frames;
    last_gemm_flop_ = 0.0;
    return PVQ_OK;
}

// the per-window kernels: a launch per window group and 16 384-frame part, the parts' dB rows behind them
pvq_status Vqt::launch_fft_groups(FftArgs& a, size_t n_frames, hipStream_t stream) {
    constexpr size_t PART = 16384;
    pvq_status es = ws_split_.reserve(std::min(PART, n_frames) * (size_t)a.n_bins * sizeof(float2));
    if (es != PVQ_OK) return es;
    a.xv_split = ws_split_.as<float2>();
    slot_begin(SLOT_FFT_FRAMES, stream);
    auto launch_group = [&](auto n_c, auto block_c, int g, int f0, int nf) -> pvq_status {
        constexpr int N = decltype(n_c)::value, BLK = decltype(block_c)::value;
        constexpr int Tg = N / 16, Fg = BLK / Tg;
        const size_t lds_g = (size_t)Fg * (N + N / 16 + 1) * sizeof(float2);
        auto kern = vqt_fft_group<N, BLK>;
        PVQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g));
        const int grid_g = (int)(((size_t)nf + Fg - 1) / Fg);   // a workgroup per Fg frames (the kernel makes one pass)
        hipLaunchKernelGGL(kern, dim3(grid_g), dim3(BLK), lds_g, stream, a, g, f0, nf);
        return PVQ_OK;
    };
    using std::integral_constant;
    for (size_t f0 = 0; f0 < n_frames; f0 += PART) {
        const int nf = (int)std::min(PART, n_frames - f0);
        for (int g = 0; g < a.n_groups; ++g) {
            pvq_status ls = PVQ_OK;
            switch (dev_->h_groups[g].n_cplx) {
                case 16384: ls = launch_group(integral_constant<int, 16384>{}, integral_constant<int, 1024>{}, g, (int)f0, nf); break;
                case 8192: ls = launch_group(integral_constant<int, 8192>{}, integral_constant<int, 512>{}, g, (int)f0, nf); break;
                case 4096: ls = launch_group(integral_constant<int, 4096>{}, integral_constant<int, 512>{}, g, (int)f0, nf); break;
                case 2048: ls = launch_group(integral_constant<int, 2048>{}, integral_constant<int, 512>{}, g, (int)f0, nf); break;
                case 1024: ls = launch_group(integral_constant<int, 1024>{}, integral_constant<int, 512>{}, g, (int)f0, nf); break;
                case 512: ls = launch_group(integral_constant<int, 512>{}, integral_constant<int, 256>{}, g, (int)f0, nf); break;
                default: ls = launch_group(integral_constant<int, 256>{}, integral_constant<int, 128>{}, g, (int)f0, nf); break;
            }
            if (ls != PVQ_OK) return ls;
        }
        if (fft_db_threads(256, a.n_bins) == 256)
            hipLaunchKernelGGL(db_rows_batch<256>, dim3((unsigned)nf), dim3(256), 0, stream, ws_split_.as<float2>(), nf, (int)f0, a.n_bins, a.streams,
                               a.n_streams, a.out_db, a.out_cplx, a.status);
        else   // more than 1 024 bins
            hipLaunchKernelGGL(db_rows_batch<1024>, dim3((unsigned)nf), dim3(1024), 0, stream, ws_split_.as<float2>(), nf, (int)f0, a.n_bins, a.streams,
                               a.n_streams, a.out_db, a.out_cplx, a.status);
    }
    slot_end(SLOT_FFT_FRAMES, stream);
    return PVQ_OK;
}

// the walk (every workgroup its frames' window groups in turn), or its group-split launch with db_rows behind it
pvq_status Vqt::launch_fft_walk(FftArgs& a, int T, int grid, size_t lds, bool split, size_t n_frames, hipStream_t stream) {
    if (split) {
        pvq_status es = ws_split_.reserve(n_frames * (size_t)a.n_bins * sizeof(float2));
        if (es != PVQ_OK) return es;
        a.xv_split = ws_split_.as<float2>();
        grid *= a.n_groups;
    }
    slot_begin(SLOT_FFT_FRAMES, stream);
    auto launch = [&](auto kern, unsigned blocks, int threads, size_t dyn, auto... args) -> pvq_status {
        if (dyn) PVQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), dyn, stream, args...);
        return PVQ_OK;
    };
    const int BLOCK = T == 1024 ? 1024 : 512;
    pvq_status lst = T == 128 ? launch(vqt_fft_frames<512, 16, 128>, grid, BLOCK, lds, a) : T == 256 ? launch(vqt_fft_frames<512, 16, 256>, grid, BLOCK, lds, a)
                     : T == 512 ? launch(vqt_fft_frames<512, 16, 512>, grid, BLOCK, lds, a) : launch(vqt_fft_frames<1024, 16, 1024>, grid, BLOCK, lds, a);
    if (lst != PVQ_OK) return lst;
    if (split) {
        const float2* rows = ws_split_.as<float2>();
        const unsigned nr = (unsigned)n_frames;
        lst = T == 128 ? launch(db_rows<128>, nr, 128, 0, rows, (int)n_frames, a.n_bins, a.out_db, a.out_cplx, a.status)
              : T == 256 ? launch(db_rows<256>, nr, 256, 0, rows, (int)n_frames, a.n_bins, a.out_db, a.out_cplx, a.status)
              : T == 512 ? launch(db_rows<512>, nr, 512, 0, rows, (int)n_frames, a.n_bins, a.out_db, a.out_cplx, a.status)
                         : launch(db_rows<1024>, nr, 1024, 0, rows, (int)n_frames, a.n_bins, a.out_db, a.out_cplx, a.status);
    }
    slot_end(SLOT_FFT_FRAMES, stream);
    return lst;
}

}  // namespace pvq
