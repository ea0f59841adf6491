// svo_sky.h -- the sky rule (INTEGRATION.md "Skybox"): from a direction to the colour of
// a ray that leaves the scene, as pure functions: no HIP types, no state, host and device, so plain g++
// compiles it (tests/sky_driver.cpp) and numpy restates it (sky.py).  Every operation is one IEEE f32
// rounding; the build contracts nothing (no fma).  Only + - * /, sqrt, floor, compares and selects: no
// libm call whose rounding could differ between host, device and numpy.
//
// The reference samples an equirectangular panorama (RaytraceCompute.compute:119-125):
//   theta = acos(direction.y) / -PI, phi = atan2(direction.x, -direction.z) / -PI * 0.5,
//   _SkyboxTexture.SampleLevel(sampler_SkyboxTexture, float2(phi, theta), 0)
// Restatement (documented): acos(y) of a unit direction is atan2(sqrt(x^2 + z^2), y), which needs no unit
// length and is well conditioned at the poles; atan2 is this header's own (atan2f32).  Mathematically
// the reference's coordinates, in other f32 operations.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SVO_SKY_FN __host__ __device__ inline
#else
#define SVO_SKY_FN inline
#endif

namespace svo_sky {

constexpr float PI = 3.14159265f;          // RaytraceCompute.compute:11
constexpr float PI_2 = PI * 0.5f;          // exact halvings of the f32 constant
constexpr float PI_4 = PI * 0.25f;
constexpr uint32_t BILINEAR = 1u;          // SVO_SKY_BILINEAR
constexpr uint32_t CLAMP_V = 2u;           // SVO_SKY_CLAMP_V
constexpr int MAX_DIM = 8192;              // largest width / height (E x 8192 <= 1/256 texel)

struct alignas(16) Texel { float r, g, b, a; };   // RGBA32F, one aligned 16-byte load; a is never read

struct Texture {
    const Texel *texels;   // texel (i, j) at texels[j * width + i]; row 0 is v = 0; null: the gradient
    int width, height;
    uint32_t flags;
};

SVO_SKY_FN float abs_(float x) { return x < 0.0f ? -x : x; }
SVO_SKY_FN bool finite_(float x) { return x - x == 0.0f; }   // inf - inf and NaN - NaN are NaN

// atan on [0, 1]: above tan(pi/8) the argument is folded by atan(a) = pi/4 + atan((a - 1) / (a + 1)),
// then the odd polynomial of Cephes' atanf on |t| <= tan(pi/8), Horner without fma.
SVO_SKY_FN float atan_unit(float a) {
    const bool fold = a > 0.4142135623730950f;
    const float t = fold ? (a - 1.0f) / (a + 1.0f) : a;
    const float z = t * t;
    float p = 8.05374449538e-2f * z;
    p = p - 1.38776856032e-1f;
    p = p * z;
    p = p + 1.99777106478e-1f;
    p = p * z;
    p = p - 3.33329491539e-1f;
    p = p * z;
    p = p * t;
    p = p + t;
    return fold ? p + PI_4 : p;
}

// atan2 in (-PI, PI] of the f32 constant PI.  atan2f32(+-0, positive) = +-0; atan2f32(0, 0) = +0 whatever
// the zeros' signs; the sign of the result is the sign of y (of a zero y too: 1 / y tells).
SVO_SKY_FN float atan2f32(float y, float x) {
    const float ay = abs_(y), ax = abs_(x);
    if (ay == 0.0f && ax == 0.0f) return 0.0f;
    const bool steep = ay > ax;
    const float a = (steep ? ax : ay) / (steep ? ay : ax);
    float r = atan_unit(a);
    if (steep) r = PI_2 - r;
    if (x < 0.0f) r = PI - r;
    const bool neg = y < 0.0f || (y == 0.0f && 1.0f / y < 0.0f);
    return neg ? -r : r;
}

// Steps 1-4: the texture coordinates (u, v) in [0, 1) (v in [0, 1] with CLAMP_V) of the direction d, used
// as given (not assumed unit).  false: d is invalid (a non-finite component, or all three zero).
SVO_SKY_FN bool direction_uv(const float d[3], uint32_t flags, float *u_out, float *v_out) {
    *u_out = 0.0f;
    *v_out = 0.0f;
    if (!(finite_(d[0]) && finite_(d[1]) && finite_(d[2]))) return false;
    const float a0 = abs_(d[0]), a1 = abs_(d[1]), a2 = abs_(d[2]);
    float m = a0 > a1 ? a0 : a1;
    m = m > a2 ? m : a2;
    if (m == 0.0f) return false;
    const float x = d[0] / m, y = d[1] / m, z = d[2] / m;   // no square overflows or vanishes below
    const float xx = x * x, zz = z * z;
    const float s = std::sqrt(xx + zz);
    const float polar = atan2f32(s, y);    // [0, PI]
    const float azim = atan2f32(x, -z);
    const float theta = polar / -PI;       // R:123
    const float phi = azim / -PI * 0.5f;   // R:124
    float u = phi - std::floor(phi);       // u always repeats
    if (u >= 1.0f) u = 0.0f;
    float v;
    if (flags & CLAMP_V) {
        v = theta + 1.0f;
        v = v > 0.0f ? v : 0.0f;
        v = v < 1.0f ? v : 1.0f;
    } else {
        v = theta - std::floor(theta);
        if (v >= 1.0f) v = 0.0f;
    }
    *u_out = u;
    *v_out = v;
    return true;
}

// Steps 5-6: the texture at (u, v).
SVO_SKY_FN void sample_uv(const Texture &tex, float u, float v, float rgb[3]) {
    const int W = tex.width, H = tex.height;
    const float fw = (float)W, fh = (float)H;
    if (!(tex.flags & BILINEAR)) {
        int i = (int)std::floor(u * fw), j = (int)std::floor(v * fh);
        i = i < W - 1 ? i : W - 1;
        j = j < H - 1 ? j : H - 1;
        const Texel t = tex.texels[(size_t)j * (size_t)W + (size_t)i];
        rgb[0] = t.r; rgb[1] = t.g; rgb[2] = t.b;
        return;
    }
    const float x = u * fw - 0.5f, y = v * fh - 0.5f;
    const float xf = std::floor(x), yf = std::floor(y);
    const float fx = x - xf, fy = y - yf;
    int i0 = (int)xf, j0 = (int)yf;
    int i1 = i0 + 1, j1 = j0 + 1;
    if (i0 < 0) i0 += W;
    if (i1 >= W) i1 -= W;
    if (tex.flags & CLAMP_V) {
        j0 = j0 > 0 ? j0 : 0;
        j1 = j1 < H - 1 ? j1 : H - 1;
    } else {
        if (j0 < 0) j0 += H;
        if (j1 >= H) j1 -= H;
    }
    const Texel t00 = tex.texels[(size_t)j0 * (size_t)W + (size_t)i0];
    const Texel t10 = tex.texels[(size_t)j0 * (size_t)W + (size_t)i1];
    const Texel t01 = tex.texels[(size_t)j1 * (size_t)W + (size_t)i0];
    const Texel t11 = tex.texels[(size_t)j1 * (size_t)W + (size_t)i1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float c00[3] = {t00.r, t00.g, t00.b}, c10[3] = {t10.r, t10.g, t10.b};
    const float c01[3] = {t01.r, t01.g, t01.b}, c11[3] = {t11.r, t11.g, t11.b};
    for (int k = 0; k < 3; ++k) {
        float lo = c00[k] * gx;
        lo = lo + c10[k] * fx;
        float hi = c01[k] * gx;
        hi = hi + c11[k] * fx;
        lo = lo * gy;
        rgb[k] = lo + hi * fy;
    }
}

// The procedural gradient (no texture set): svo_kernel.hip's sky() on the direction's y as given.
SVO_SKY_FN void gradient(float dir_y, float rgb[3]) {
    const float k = 0.5f * dir_y + 0.5f;
    rgb[0] = 0.25f + 0.5f * k;
    rgb[1] = 0.35f + 0.55f * k;
    rgb[2] = 0.6f + 0.4f * k;
}

// The rule: direction -> RGB.  An invalid direction is black with and without a texture.
SVO_SKY_FN void sample(const Texture &tex, const float d[3], float rgb[3]) {
    float u, v;
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (!direction_uv(d, tex.flags, &u, &v)) return;
    if (!tex.texels) {
        gradient(d[1], rgb);
        return;
    }
    sample_uv(tex, u, v, rgb);
}

}  // namespace svo_sky
