// present_batch.hip — bloom, display transform and sRGB bytes for many pictures (present_batch.hpp).
//
// A call's rows are cut into pieces whose mip chains fit the workspace; a piece runs one launch per pyramid level over all of its
// rows: present_down<true> (picture -> mip 0), present_down<false> (mip k - 1 -> mip k), present_up<false> (mip k into mip k - 1,
// k = n - 1 .. 1) and present_up<true> (mip 0 into the picture, display transform, encode).  Every kernel has the tile kernels'
// shape — a workgroup per 16 x 16 target texels, a wave per 8 x 8 block, a lane per texel, rows along gridDim.y — and every lane
// writes its own texel only: a row's result depends neither on its place in the call nor on the cut.  A row whose intensity does
// not bloom is skipped by a workgroup-uniform test in every launch but the last, which still transforms and encodes it.
//
// The 13 (9) bilinear taps of neighbouring targets overlap almost completely, so a workgroup first stages its tile's source
// footprint in LDS (16-byte texels, 16-byte loads) and samples there.  Between two mips a footprint always fits; the picture's
// size is the caller's, so its two passes have a STAGED = false form that samples device memory: the first pass where mip 0 is
// far smaller than the picture, the last where it is far larger.  The host decides with the very function the kernel sizes its
// footprint with (present::footprint).  The last pass reads a picture pixel only in the lane that writes it, so d_hdr may be
// d_image.
//
// FMA contraction is off and `/` is the correctly rounded one, as in raster_batch.hip.
#include "present_batch.hpp"

#include <algorithm>
#include <string>

#include "stage_device.hpp"
#include "stage_plan.hpp"

namespace pvq {

namespace {
constexpr uint32_t FOOT = 44 * 44;   // texels of a staged footprint: a 16 x 16 tile at twice the target's size, taps and slack

struct GlobalTex {
    const float4* p;
    uint32_t w;
    __device__ __forceinline__ void operator()(uint32_t x, uint32_t y, float rgb[3]) const {
        const float4 t = p[static_cast<size_t>(y) * w + x];
        rgb[0] = t.x;
        rgb[1] = t.y;
        rgb[2] = t.z;
    }
};
// the footprint lx .. lx + fw, ly .. ly + fh of a texture; an index outside it (none is, present::footprint) reads its last texel
struct LdsTex {
    const float4* s;
    uint32_t lx, ly, fw, fh;
    __device__ __forceinline__ void operator()(uint32_t x, uint32_t y, float rgb[3]) const {
        const uint32_t xx = min(x - lx, fw - 1u), yy = min(y - ly, fh - 1u);
        const float4 t = s[yy * fw + xx];
        rgb[0] = t.x;
        rgb[1] = t.y;
        rgb[2] = t.z;
    }
};

struct Footprint {
    uint32_t lx, ly, fw, fh;
};
__device__ __forceinline__ Footprint tile_footprint(uint32_t i0, uint32_t j0, uint32_t wt, uint32_t ht, uint32_t ws, uint32_t hs, float mx, float my) {
    Footprint f;
    present::footprint(i0, stage::TILE, wt, ws, mx, f.lx, f.fw);
    present::footprint(j0, stage::TILE, ht, hs, my, f.ly, f.fh);
    if (f.fw * f.fh > FOOT) f.fh = FOOT / f.fw;   // never: the host launches STAGED only where every tile's footprint fits
    return f;
}
// all 256 lanes; the barrier in front lets the lanes that still sample the footprint before it finish
__device__ __forceinline__ void stage_footprint(const float4* src, uint32_t ws, const Footprint& f, float4* s) {
    __syncthreads();
    const uint32_t n = f.fw * f.fh;
    for (uint32_t k = threadIdx.x; k < n; k += 256u) {
        const uint32_t y = k / f.fw, x = k - y * f.fw;
        s[k] = src[static_cast<size_t>(f.ly + y) * ws + f.lx + x];
    }
    __syncthreads();
}

struct PassArgs {
    const float4* src;        // row r's source texture at src + r * src_stride: ws x hs texels
    float4* dst;              // row r's target at dst + r * dst_stride: wt x ht texels (not in the last pass)
    size_t src_stride, dst_stride;
    uint32_t ws, hs, wt, ht;
    uint32_t rows;
    const float* intensity;   // [rows], or null in the last pass: no row blooms
    float mx, my;             // the taps' reach in source texels
    // down
    float threshold, softness;
    // up
    float lf, hp, x;          // the level's blend table entries; the tent's uv radius along x
    int composite_mode, tonemapping;
    const float4* picture;    // the last pass: [rows][ht][wt] in, bytes and (or null) the bloomed picture out
    uint32_t* rgba8;
    float4* hdr;
};

__device__ __forceinline__ bool tile_texel(uint32_t wt, uint32_t ht, uint32_t& i0, uint32_t& j0, uint32_t& i, uint32_t& j) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tiles_x = (wt + stage::TILE - 1) / stage::TILE;
    i0 = (blockIdx.x % tiles_x) * stage::TILE;
    j0 = (blockIdx.x / tiles_x) * stage::TILE;
    i = i0 + (wave & 1u) * 8u + (lane & 7u);
    j = j0 + (wave >> 1) * 8u + (lane >> 3);
    return i < wt && j < ht;
}

template <bool FIRST, bool STAGED>
__global__ __launch_bounds__(256) __attribute__((flatten)) void present_down(PassArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 s_foot[STAGED ? FOOT : 1];
    uint32_t i0, j0, i, j;
    const bool inside = tile_texel(a.wt, a.ht, i0, j0, i, j);
    Footprint f{};
    if (STAGED) f = tile_footprint(i0, j0, a.wt, a.ht, a.ws, a.hs, a.mx, a.my);
    const float u = present::pixel_uv(i, a.wt), v = present::pixel_uv(j, a.ht);
    for (uint32_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
        if (!present::blooms(a.intensity[r])) continue;   // the same in every lane of the workgroup
        const float4* src = a.src + r * a.src_stride;
        if (STAGED) stage_footprint(src, a.ws, f, s_foot);
        if (inside) {
            float out[3];
            const LdsTex staged{s_foot, f.lx, f.ly, f.fw, f.fh};
            const GlobalTex direct{src, a.ws};
            if (FIRST && STAGED) present::down_first(staged, a.ws, a.hs, u, v, a.threshold, a.softness, out);
            else if (FIRST) present::down_first(direct, a.ws, a.hs, u, v, a.threshold, a.softness, out);
            else present::down_plain(staged, a.ws, a.hs, u, v, out);
            a.dst[r * a.dst_stride + static_cast<size_t>(j) * a.wt + i] = make_float4(out[0], out[1], out[2], 0.0f);
        }
    }
}

template <bool LAST, bool STAGED>
__global__ __launch_bounds__(256) __attribute__((flatten)) void present_up(PassArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 s_foot[STAGED ? FOOT : 1];
    uint32_t i0, j0, i, j;
    const bool inside = tile_texel(a.wt, a.ht, i0, j0, i, j);
    Footprint f{};
    if (STAGED) f = tile_footprint(i0, j0, a.wt, a.ht, a.ws, a.hs, a.mx, a.my);
    const float u = present::pixel_uv(i, a.wt), v = present::pixel_uv(j, a.ht);
    const size_t texel = static_cast<size_t>(j) * a.wt + i;
    for (uint32_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
        const float intensity = a.intensity ? a.intensity[r] : 0.0f;
        const bool bloom = present::blooms(intensity);   // the same in every lane of the workgroup
        if (!LAST && !bloom) continue;
        const float4* src = a.src + r * a.src_stride;
        if (STAGED && bloom) stage_footprint(src, a.ws, f, s_foot);
        if (!inside) continue;                            // no barrier follows in this trip: the next trip's comes first
        float4* at = LAST ? nullptr : a.dst + r * a.dst_stride + texel;
        const size_t pixel = r * (static_cast<size_t>(a.wt) * a.ht) + texel;
        const float4 c = LAST ? a.picture[pixel] : *at;
        float px[3] = {c.x, c.y, c.z};
        if (bloom) {
            float t[3];
            if (STAGED) present::tent(LdsTex{s_foot, f.lx, f.ly, f.fw, f.fh}, a.ws, a.hs, u, v, a.x, present::TENT, t);
            else present::tent(GlobalTex{src, a.ws}, a.ws, a.hs, u, v, a.x, present::TENT, t);
            float lf = a.lf;
            if (a.composite_mode == present::ENERGY_CONSERVING) lf *= 1.0f - intensity;
            present::composite(a.composite_mode, (intensity + lf) * a.hp, t, px);   // present::blend_factor
        }
        if (!LAST) {
            *at = make_float4(px[0], px[1], px[2], 0.0f);
        } else {
            if (a.hdr) a.hdr[pixel] = make_float4(px[0], px[1], px[2], c.w);
            float shown[3];
            present::display(a.tonemapping, px, shown);
            a.rgba8[pixel] = present::encode(shown, c.w);
        }
    }
}

// whether every 16 x 16 tile's footprint of a pass fits the LDS array
bool footprints_fit(uint32_t wt, uint32_t ht, uint32_t ws, uint32_t hs, float mx, float my) {
    uint32_t lo, n, fw = 0, fh = 0;
    for (uint32_t i0 = 0; i0 < wt; i0 += stage::TILE) {
        present::footprint(i0, stage::TILE, wt, ws, mx, lo, n);
        fw = std::max(fw, n);
    }
    for (uint32_t j0 = 0; j0 < ht; j0 += stage::TILE) {
        present::footprint(j0, stage::TILE, ht, hs, my, lo, n);
        fh = std::max(fh, n);
    }
    return static_cast<uint64_t>(fw) * fh <= FOOT;
}
float tent_reach(float radius, uint32_t size) {
#pragma clang fp contract(off)
    return radius * static_cast<float>(size);
}
dim3 grid_of(uint32_t wt, uint32_t ht, size_t rows) {
    const uint32_t tiles = ((wt + stage::TILE - 1) / stage::TILE) * ((ht + stage::TILE - 1) / stage::TILE);
    return dim3(tiles, static_cast<unsigned>(std::min<size_t>(rows, 65535)));
}
}  // namespace

pvq_status PresentBatch::create(int device_id, const present::Settings& settings, uint32_t width, uint32_t height, std::unique_ptr<PresentBatch>& out) {
    out.reset();
    std::string err;
    if (!stage_image_ok("present batch", width, height, 0.0f, err) || !present_settings_ok("present batch", settings, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    std::unique_ptr<PresentBatch> b(new PresentBatch());
    b->device_id_ = device_id < 0 ? -1 : device_id;
    b->width_ = width;
    b->height_ = height;
    b->settings_ = present_resolved(settings);
    if (!present_plan("present batch", width, height, b->settings_.max_mip_dimension, b->plan_, err)) {
        set_last_error(err);
        return PVQ_ERR_UNSUPPORTED;
    }
    const present::Mips& m = b->plan_.mips;
    present::blend_tables(b->settings_, m.n, b->factors_);
    const float x = present::tent_x(width, height);
    // Between two mips the sizes differ by a factor of 2 (3 where a side of 3 becomes 1) and the tent reaches 0.004 * 4096 / 2 texels
    // at most: those footprints always fit.  The picture's own size is the caller's: its two passes have a form without staging.
    bool fit = true;
    for (uint32_t k = 1; k < m.n; ++k)
        fit = fit && footprints_fit(m.w[k], m.h[k], m.w[k - 1], m.h[k - 1], 2.0f, 2.0f) &&
              footprints_fit(m.w[k - 1], m.h[k - 1], m.w[k], m.h[k], tent_reach(x, m.w[k]), tent_reach(present::TENT, m.h[k]));
    if (!fit) {
        set_last_error("present batch: a mip's footprint does not fit its tile");
        return PVQ_ERR_INTERNAL;
    }
    b->staged_first_ = footprints_fit(m.w[0], m.h[0], width, height, 2.0f, 2.0f);
    b->staged_last_ = footprints_fit(width, height, m.w[0], m.h[0], tent_reach(x, m.w[0]), tent_reach(present::TENT, m.h[0]));
    out = std::move(b);
    return PVQ_OK;
}

pvq_status PresentBatch::set_workspace_limit(uint64_t bytes) {
    if (bytes == 0) {
        set_last_error("present batch: the workspace limit must be positive");
        return PVQ_ERR_INVALID_ARG;
    }
    limit_ = bytes;
    return PVQ_OK;
}

pvq_status PresentBatch::rows_device(size_t n_rows, const float* d_image, const float* d_intensity, uint8_t* d_rgba8, float* d_hdr, hipStream_t stream) {
    if (!d_image || !d_rgba8) {
        set_last_error("present batch: d_image and d_rgba8 are needed");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(d_image) | reinterpret_cast<uintptr_t>(d_hdr)) & 15) {
        set_last_error("present batch: d_image and d_hdr must be 16-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(d_rgba8) | reinterpret_cast<uintptr_t>(d_intensity)) & 3) {
        set_last_error("present batch: d_rgba8 and d_intensity must be 4-byte aligned");
        return PVQ_ERR_INVALID_ARG;
    }
    std::string err;
    if (!stage_frames_ok("present batch", n_rows, 1, err)) {
        set_last_error(err);
        return PVQ_ERR_INVALID_ARG;
    }
    if (device_id_ < 0) {
        set_last_error("the batched present stage runs on a GPU; this handle has none (pvq_present_frame is the host face)");
        return PVQ_ERR_NO_DEVICE;
    }
    if (n_rows == 0) return PVQ_OK;
    PVQ_HIP(hipSetDevice(device_id_));

    const present::Mips& m = plan_.mips;
    const size_t pixels = static_cast<size_t>(width_) * height_;
    const size_t piece = d_intensity ? present_piece_rows(n_rows, plan_, limit_) : n_rows;
    if (d_intensity)
        if (pvq_status s = chains_.reserve(piece * plan_.texels * 16)) return s;
    float4* chains = chains_.as<float4>();
    PassArgs base{};
    base.src_stride = base.dst_stride = plan_.texels;
    base.threshold = settings_.threshold;
    base.softness = settings_.threshold_softness;
    base.x = present::tent_x(width_, height_);
    base.composite_mode = settings_.composite_mode;
    base.tonemapping = settings_.tonemapping;
    for (size_t r0 = 0; r0 < n_rows; r0 += piece) {
        const size_t rows = std::min(piece, n_rows - r0);
        base.rows = static_cast<uint32_t>(rows);
        base.intensity = d_intensity ? d_intensity + r0 : nullptr;
        const float4* picture = reinterpret_cast<const float4*>(d_image) + r0 * pixels;
        if (d_intensity) {
            for (uint32_t k = 0; k < m.n; ++k) {   // down
                PassArgs a = base;
                a.src = k == 0 ? picture : chains + plan_.offset[k - 1];
                if (k == 0) a.src_stride = pixels;
                a.dst = chains + plan_.offset[k];
                a.ws = k == 0 ? width_ : m.w[k - 1];
                a.hs = k == 0 ? height_ : m.h[k - 1];
                a.wt = m.w[k];
                a.ht = m.h[k];
                a.mx = a.my = 2.0f;
                const dim3 grid = grid_of(a.wt, a.ht, rows);
                if (k > 0) hipLaunchKernelGGL((present_down<false, true>), grid, dim3(256), 0, stream, a);
                else if (staged_first_) hipLaunchKernelGGL((present_down<true, true>), grid, dim3(256), 0, stream, a);
                else hipLaunchKernelGGL((present_down<true, false>), grid, dim3(256), 0, stream, a);
            }
            for (uint32_t k = m.n - 1; k >= 1; --k) {   // up, in place
                PassArgs a = base;
                a.src = chains + plan_.offset[k];
                a.dst = chains + plan_.offset[k - 1];
                a.ws = m.w[k];
                a.hs = m.h[k];
                a.wt = m.w[k - 1];
                a.ht = m.h[k - 1];
                a.mx = tent_reach(base.x, a.ws);
                a.my = tent_reach(present::TENT, a.hs);
                a.lf = factors_.lf[k];
                a.hp = factors_.hp[k];
                const dim3 grid = grid_of(a.wt, a.ht, rows);
                hipLaunchKernelGGL((present_up<false, true>), grid, dim3(256), 0, stream, a);
            }
        }
        PassArgs a = base;   // mip 0 into the picture, transform, encode
        a.src = d_intensity ? chains + plan_.offset[0] : nullptr;
        a.ws = m.w[0];
        a.hs = m.h[0];
        a.wt = width_;
        a.ht = height_;
        a.mx = tent_reach(base.x, a.ws);
        a.my = tent_reach(present::TENT, a.hs);
        a.lf = factors_.lf[0];
        a.hp = factors_.hp[0];
        a.picture = picture;
        a.rgba8 = reinterpret_cast<uint32_t*>(d_rgba8) + r0 * pixels;
        a.hdr = d_hdr ? reinterpret_cast<float4*>(d_hdr) + r0 * pixels : nullptr;
        const dim3 grid = grid_of(a.wt, a.ht, rows);
        if (staged_last_) hipLaunchKernelGGL((present_up<true, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((present_up<true, false>), grid, dim3(256), 0, stream, a);
    }
    PVQ_HIP(hipGetLastError());
    return PVQ_OK;
}

}  // namespace pvq
