// raster_math.hpp — the one copy of the pitch balls' picture, for the host object (raster_host.cpp, g++) and the device stage
// (raster_batch.hip): what the viewer's ball material makes of a ball per pixel (pitchvis_viewer/assets/shaders/
// noisy_color_rings_2d.wgsl:395-428, named by material.rs:33-35), the camera and the ball rectangle (setup.rs:359-365, :110-112),
// and Bevy's alpha blend, restated from their behaviour.  The assumed semantics of the WGSL built-ins are DESIGN.md 6e's table.
//
// All of it is f32, FMA contraction off on both sides, components left to right.  The libm calls (sin, cos, atan2) go through
// RasterMath: the double-precision function rounded once to f32, as scene_math.hpp's; sqrt and `/` are IEEE f32.  So the model
// (tests/raster_model.py), the host face and the device carry the same bits.
#pragma once

#include <cstring>

#include "scene_math.hpp"

namespace pvq {
namespace raster {

struct RasterMath {
    static PVQ_HD float sin(float x) { return static_cast<float>(::sin(static_cast<double>(x))); }
    static PVQ_HD float cos(float x) { return static_cast<float>(::cos(static_cast<double>(x))); }
    static PVQ_HD float atan2(float y, float x) { return static_cast<float>(::atan2(static_cast<double>(y), static_cast<double>(x))); }
};

constexpr float PI_W = 3.14159265359f;                   // the shader's own constant, rounded to f32
constexpr float VIEWPORT_HEIGHT = 38.0f * 0.41421357f;   // setup.rs:361
constexpr float BALL_SIDE = 20.0f;                       // setup.rs:110
constexpr uint32_t MAX_IMAGE = 4096;

// ---- the WGSL built-ins, as WGSL defines them ----
PVQ_HD float w_mod(float x, float y) {
    PVQ_FP_STRICT
    return x - y * truncf(x / y);
}
PVQ_HD float w_step(float edge, float x) { return x >= edge ? 1.0f : 0.0f; }
PVQ_HD float w_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
PVQ_HD float w_mix(float a, float b, float t) {
    PVQ_FP_STRICT
    return a * (1.0f - t) + b * t;
}
PVQ_HD float w_smoothstep(float lo, float hi, float x) {   // also as written where lo > hi
    PVQ_FP_STRICT
    const float t = w_clamp((x - lo) / (hi - lo), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

// ---- 3-D simplex noise: the published construction of McEwan and Gustavson ("Efficient computational noise in GLSL", 2012), in
// scalar form: skew to the simplex grid, pick the two middle corners by the order of the offsets, hash each corner through the
// permutation polynomial (34 x + 1) x mod 289, map the hash onto a 7 x 7 grid folded over an octahedron for the gradient, scale
// it by the first-order inverse square root, and sum the four corners' radial falloffs (0.6 - d^2)^4 times gradient . offset.
PVQ_HD float permute(float x) {
    PVQ_FP_STRICT
    return w_mod((x * 34.0f + 1.0f) * x, 289.0f);
}

// one corner: its hash p and its offset (x, y, z) from the point; returns falloff^4 weight and gradient . offset
PVQ_HD_FLAT void corner(float p, float x, float y, float z, float& m4, float& gd) {
    PVQ_FP_STRICT
    constexpr float N7 = 1.0f / 7.0f;
    const float nsx = N7 * 2.0f - 0.0f, nsy = N7 * 0.5f - 1.0f, nsz = N7 * 1.0f - 0.0f;
    const float j = p - 49.0f * floorf(p * nsz * nsz);   // p mod 49
    const float gx_ = floorf(j * nsz);
    const float gy_ = floorf(j - 7.0f * gx_);              // j mod 7
    const float gx = gx_ * nsx + nsy;
    const float gy = gy_ * nsx + nsy;
    const float h = 1.0f - fabsf(gx) - fabsf(gy);
    const float sh = -w_step(h, 0.0f);                    // -1 on the octahedron's lower half
    const float ax = gx + (floorf(gx) * 2.0f + 1.0f) * sh;
    const float ay = gy + (floorf(gy) * 2.0f + 1.0f) * sh;
    const float norm = 1.79284291400159f - 0.85373472095314f * (ax * ax + ay * ay + h * h);
    const float px = ax * norm, py = ay * norm, pz = h * norm;
    float m = fmaxf(0.6f - (x * x + y * y + z * z), 0.0f);
    m = m * m;
    m4 = m * m;
    gd = px * x + py * y + pz * z;
}

PVQ_HD_FLAT float simplex3(float vx, float vy, float vz) {
    PVQ_FP_STRICT
    constexpr float C6 = 1.0f / 6.0f, C3 = 1.0f / 3.0f;
    const float s = vx * C3 + vy * C3 + vz * C3;
    float ix = floorf(vx + s), iy = floorf(vy + s), iz = floorf(vz + s);
    const float t = ix * C6 + iy * C6 + iz * C6;
    const float x0 = vx - ix + t, y0 = vy - iy + t, z0 = vz - iz + t;
    // the order of the three offsets picks the second and third corner
    const float gx = w_step(y0, x0), gy = w_step(z0, y0), gz = w_step(x0, z0);
    const float lx = 1.0f - gx, ly = 1.0f - gy, lz = 1.0f - gz;
    const float i1x = fminf(gx, lz), i1y = fminf(gy, lx), i1z = fminf(gz, ly);
    const float i2x = fmaxf(gx, lz), i2y = fmaxf(gy, lx), i2z = fmaxf(gz, ly);
    const float c1 = 1.0f * C6, c2 = 2.0f * C6, c3 = 3.0f * C6;
    const float x1 = x0 - i1x + c1, y1 = y0 - i1y + c1, z1 = z0 - i1z + c1;
    const float x2 = x0 - i2x + c2, y2 = y0 - i2y + c2, z2 = z0 - i2z + c2;
    const float x3 = x0 - 1.0f + c3, y3 = y0 - 1.0f + c3, z3 = z0 - 1.0f + c3;
    ix = w_mod(ix, 289.0f);
    iy = w_mod(iy, 289.0f);
    iz = w_mod(iz, 289.0f);
    const float p0 = permute(permute(permute(iz + 0.0f) + iy + 0.0f) + ix + 0.0f);
    const float p1 = permute(permute(permute(iz + i1z) + iy + i1y) + ix + i1x);
    const float p2 = permute(permute(permute(iz + i2z) + iy + i2y) + ix + i2x);
    const float p3 = permute(permute(permute(iz + 1.0f) + iy + 1.0f) + ix + 1.0f);
    float m0, m1, m2, m3, d0, d1, d2, d3;
    corner(p0, x0, y0, z0, m0, d0);
    corner(p1, x1, y1, z1, m1, d1);
    corner(p2, x2, y2, z2, m2, d2);
    corner(p3, x3, y3, z3, m3, d3);
    return 42.0f * (m0 * d0 + m1 * d1 + m2 * d2 + m3 * d3);
}

// ---- a ball, ready to be drawn: what does not depend on the pixel ----
struct Ball {
    float x, y, side, noise_z;              // centre, 20 * scale, time * 0.8
    float r, g, b, a;                       // the material colour (linear)
    float calmness, ring_strength;          // clamp(1 - calmness * 1.65, 0, 1)^3
    float dot_factor, dot_pulse;            // (acc - 0.85) / (1 - 0.85), or -1: no centre dot; 0.85 + 0.15 sin(3 t)
    float spiral, star_brightness;          // deviation * 4; mix(0.3, 1, 1 - |dev| * 2) * (0.7 + 0.3 sin(3 t))
    uint32_t box_x, box_y;                  // first | last << 16 of the pixel columns / rows that can be covered
};
static_assert(sizeof(Ball) == 64, "workspace layout");

PVQ_HD bool finite_f(float v) { return fabsf(v) <= 3.40282347e+38f; }   // false for NaN

// not drawn: visible bit clear, scale <= 0, or any of the eleven values or the time not finite
PVQ_HD bool drawable(const float xyzs[4], const float rgba[4], const float params[3], float time, bool visible) {
    bool ok = visible && xyzs[3] > 0.0f && finite_f(time);
    for (int i = 0; i < 4; ++i) ok = ok && finite_f(xyzs[i]) && finite_f(rgba[i]);
    for (int i = 0; i < 3; ++i) ok = ok && finite_f(params[i]);
    return ok;
}

// The pixel columns and rows outside of which no pixel of the ball has length(p) < 1: an acceleration only, so it errs outwards —
// by a pixel, and by the rounding of wx - x and wy - y (half an ulp of the larger operand each; 2^-22 relative covers it).
// false: nothing of the ball is on the image.
PVQ_HD bool pixel_box(float x, float y, float side, uint32_t W, uint32_t H, float vh, uint32_t& box_x, uint32_t& box_y) {
    const double s = static_cast<double>(vh / static_cast<float>(H));
    const double slack = 2.4e-7 * (fabs(static_cast<double>(x)) + fabs(static_cast<double>(y)) + s * (W + H));
    const double half = 0.5 * static_cast<double>(side) * (1.0 + 1e-6) + slack;
    double c0 = floor((x - half) / s + 0.5 * W - 0.5) - 1.0, c1 = ceil((x + half) / s + 0.5 * W - 0.5) + 1.0;
    double r0 = floor(0.5 * H - 0.5 - (y + half) / s) - 1.0, r1 = ceil(0.5 * H - 0.5 - (y - half) / s) + 1.0;
    if (!(c0 <= c1) || !(r0 <= r1)) {   // NaN (side or vh overflowed): the whole image
        c0 = r0 = 0.0;
        c1 = W - 1.0;
        r1 = H - 1.0;
    }
    if (c1 < 0.0 || r1 < 0.0 || c0 > W - 1.0 || r0 > H - 1.0) return false;
    c0 = c0 < 0.0 ? 0.0 : c0;
    r0 = r0 < 0.0 ? 0.0 : r0;
    c1 = c1 > W - 1.0 ? W - 1.0 : c1;
    r1 = r1 > H - 1.0 ? H - 1.0 : r1;
    box_x = static_cast<uint32_t>(c0) | static_cast<uint32_t>(c1) << 16;
    box_y = static_cast<uint32_t>(r0) | static_cast<uint32_t>(r1) << 16;
    return true;
}

PVQ_HD_FLAT void make_ball(const float xyzs[4], const float rgba[4], const float params[3], float time, Ball& o) {
    PVQ_FP_STRICT
    o.x = xyzs[0];
    o.y = xyzs[1];
    o.side = BALL_SIDE * xyzs[3];
    o.noise_z = time * 0.8f;
    o.r = rgba[0];
    o.g = rgba[1];
    o.b = rgba[2];
    o.a = rgba[3];
    const float calmness = params[0], accuracy = params[1], deviation = params[2];
    o.calmness = calmness;
    const float c = w_clamp(1.0f - calmness * 1.65f, 0.0f, 1.0f);
    o.ring_strength = c * c * c;
    const float threshold = 0.85f;
    o.dot_factor = accuracy < threshold ? -1.0f : (accuracy - threshold) / (1.0f - threshold);
    const float wave = RasterMath::sin(time * 3.0f);
    o.dot_pulse = 0.85f + 0.15f * wave;
    o.spiral = deviation * 4.0f;
    o.star_brightness = w_mix(0.3f, 1.0f, 1.0f - fabsf(deviation) * 2.0f) * (0.7f + 0.3f * wave);
    o.box_x = o.box_y = 0u;
}

// the ball's own coordinates of a world position: mesh uv with v running downwards
PVQ_HD void ball_uv(const Ball& q, float wx, float wy, float& u, float& v) {
    PVQ_FP_STRICT
    u = (wx - q.x) / q.side + 0.5f;
    v = 0.5f - (wy - q.y) / q.side;
}
PVQ_HD float radius_of(float u, float v, float& px, float& py) {
    PVQ_FP_STRICT
    px = u * 2.0f - 1.0f;
    py = v * 2.0f - 1.0f;
    return sqrtf(px * px + py * py);
}

// the fragment at mesh uv (u, v); r = radius_of(u, v, px, py).  Its alpha is exactly 0 where r >= 1.
PVQ_HD_FLAT void shade(const Ball& q, float u, float v, float px, float py, float r, float out[4]) {
    PVQ_FP_STRICT
    const float noise = w_clamp(simplex3(u * 4.3f, v * 4.3f, q.noise_z) - 0.15f, 0.0f, 1.0f);
    const float f = RasterMath::sin(r * sqrtf(r) * PI_W * 1.0f);
    const float ring = f * f;
    const float w = noise * q.calmness * ring;
    float dot = 0.0f;
    if (q.dot_factor >= 0.0f) dot = 1.0f * w_smoothstep(0.08f, 0.0f, r) * q.dot_factor * q.dot_pulse;
    float star = 0.0f;
    if (!(r > 0.25f || r < 0.01f)) {
        const float angle = RasterMath::atan2(py, px);
        const float spiral_angle = angle * 6.0f + r * q.spiral * PI_W * 4.0f;
        const float intensity = fmaxf(0.0f, RasterMath::cos(spiral_angle)) * (1.0f - w_smoothstep(0.15f, 0.25f, r));
        star = 1.0f * intensity * q.star_brightness;
    }
    const float add = (dot + star) * 0.4f;
    const float rgb[3] = {q.r, q.g, q.b};
    const float edge = w_smoothstep(0.96f, 1.0f, r);
    for (int c = 0; c < 3; ++c) {
        const float fin = w_mix(rgb[c], 1.0f, w) + add;
        const float col = w_mix(rgb[c], fin, q.ring_strength);
        out[c] = w_mix(col, col, edge);
    }
    const float alpha = w_mix(q.a, q.a * ring, q.ring_strength);
    out[3] = w_mix(alpha, 0.0f, edge);
}

// AlphaMode2d::Blend of a fragment over what is there
PVQ_HD void blend(const float src[4], float dst[4]) {
    PVQ_FP_STRICT
    const float k = 1.0f - src[3];
    dst[0] = src[0] * src[3] + dst[0] * k;
    dst[1] = src[1] * src[3] + dst[1] * k;
    dst[2] = src[2] * src[3] + dst[2] * k;
    dst[3] = src[3] + dst[3] * k;
}

// the world position of a pixel's centre (orthographic, FixedVertical, centred on the origin; row 0 at the top)
PVQ_HD void pixel_world(uint32_t i, uint32_t j, uint32_t W, uint32_t H, float vh, float& wx, float& wy) {
    PVQ_FP_STRICT
    const float s = vh / static_cast<float>(H);
    wx = (static_cast<float>(i) + 0.5f - 0.5f * static_cast<float>(W)) * s;
    wy = (0.5f * static_cast<float>(H) - (static_cast<float>(j) + 0.5f)) * s;
}

// every drawable ball's pixel of one pixel: dst holds the background on entry.  list: n balls back to front.
PVQ_HD_FLAT void compose_ball(const Ball& q, float wx, float wy, float dst[4]) {
    float u, v, px, py;
    ball_uv(q, wx, wy, u, v);
    const float r = radius_of(u, v, px, py);
    if (!(r < 1.0f)) return;   // alpha exactly 0: the pixel is left as it is
    float src[4];
    shade(q, u, v, px, py, r, src);
    blend(src, dst);
}

// the drawing order: ascending z (-0 as +0), ties by ascending bin.  z is finite.
PVQ_HD uint64_t order_key(float z, uint32_t bin) {
    PVQ_FP_STRICT
    const float zz = z + 0.0f;
    uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(zz);
#else
    memcpy(&bits, &zz, 4);
#endif
    bits = (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
    return static_cast<uint64_t>(bits) << 32 | bin;
}

// the clear colour: LinearRgba::from(Color::srgb(...)), mod.rs:19-21 with update.rs:914-915
PVQ_HD_FLAT void clear_color(int mode, float out[4]) {
    const bool galaxy = mode == scene::GALAXY;
    out[0] = scene::srgb_to_linear(galaxy ? 0.05f : 0.23f);
    out[1] = scene::srgb_to_linear(galaxy ? 0.0f : 0.23f);
    out[2] = scene::srgb_to_linear(galaxy ? 0.05f : 0.25f);
    out[3] = 1.0f;
}

}  // namespace raster
}  // namespace pvq
