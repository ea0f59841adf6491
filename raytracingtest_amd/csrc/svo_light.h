// svo_light.h -- the light rule (INTEGRATION.md "Lights"): from a traced ray, its hit and a
// point light to the shadow ray toward the light and to the light's share of the pixel, as pure functions:
// no HIP types, no state, host and device, so plain g++ compiles it (tests/light_driver.cpp) and numpy
// restates it (lights.py).  Every operation is one IEEE f32 rounding; the build contracts nothing.  Only
// + - * /, sqrt, compares and selects: / and sqrt are correctly rounded on host and device (svo_sky.h).
//
// Deviation from the reference (documented): the reference has _DirectionalLight only.  The shadow ray
// leaves through the voxel face the camera ray entered by (svo_reflect.h entry_face), and its direction is
// the unnormalised vector to the light, so parameter 1 of the ray is the light itself.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "svo_reflect.h"

namespace svo_lights {

constexpr int MAX_LIGHTS = 8;           // SVO_MAX_LIGHTS
constexpr uint32_t NO_SHADOW = 1u;      // SVO_LIGHT_NO_SHADOW
constexpr float MAX_COORD = 0x1p20f;    // |position| and range
constexpr float MAX_COLOUR = 65536.0f;

struct Light {                          // == svo_light
    float position[3];
    float range;
    float colour[3];
    uint32_t flags;
};
static_assert(sizeof(Light) == 32, "svo_light layout");

// What svo_set_lights refuses in one light; null: the light is valid.
SVO_REFLECT_FN const char *light_error(const Light &l) {
    for (int k = 0; k < 3; ++k)
        if (!(l.position[k] >= -MAX_COORD && l.position[k] <= MAX_COORD))
            return "light position components must be finite and lie in [-2^20, 2^20]";
    if (!(l.range > 0.0f && l.range <= MAX_COORD)) return "light range must lie in (0, 2^20]";
    for (int k = 0; k < 3; ++k)
        if (!(l.colour[k] >= 0.0f && l.colour[k] <= MAX_COLOUR)) return "light colour components must lie in [0, 65536]";
    if (l.flags & ~NO_SHADOW) return "unknown light flag bits";
    return nullptr;
}

// Steps 2-3 of the rule from the origin Q on the entry face (axis g, out = +-1 as svo_reflect::entry_face
// gives them) and the light (p, R):
//   L_k = p_k - Q_k; facing iff L_g out > 0 (the product is exact: out = +-1);
//   d2 = (L0 L0 + L1 L1) + L2 L2, u = d2 / (R R); in range iff u < 1 (NaN: false).
// No array is indexed by g.  A light that is facing and in range has a finite, non-zero L and a finite Q:
// its shadow ray is valid by the query's classify.
SVO_REFLECT_FN void light_vector(const float Q[3], int g, float out, const float p[3], float R, float L[3], float *d2,
                                 float *u, bool *facing, bool *in_range) {
    L[0] = p[0] - Q[0];
    L[1] = p[1] - Q[1];
    L[2] = p[2] - Q[2];
    const float L_g = g == 0 ? L[0] : g == 1 ? L[1] : L[2];
    *facing = L_g * out > 0.0f;
    float s = L[0] * L[0];
    s = s + L[1] * L[1];
    s = s + L[2] * L[2];
    *d2 = s;
    *u = s / (R * R);
    *in_range = *u < 1.0f;
}

// Step 6: the factor k of a lit pixel, from the record normal n and step 2-3's L, d2, u:
//   dist = sqrt(d2); ndl = ((n0 L0 + n1 L1) + n2 L2) / dist; s = ndl > 0 ? ndl : 0, then s < 1 ? s : 1
//   (shade_hit's saturate; a NaN gives 0); w = 1 - u u, w = w w; a = w / (1 + d2); k = s a.
SVO_REFLECT_FN float light_factor(const float n[3], const float L[3], float d2, float u) {
    const float dist = std::sqrt(d2);
    float dot = n[0] * L[0];
    dot = dot + n[1] * L[1];
    dot = dot + n[2] * L[2];
    const float ndl = dot / dist;
    float s = ndl > 0.0f ? ndl : 0.0f;
    s = s < 1.0f ? s : 1.0f;
    float w = 1.0f - u * u;
    w = w * w;
    const float a = w / (1.0f + d2);
    return s * a;
}

// The fold's step for one lit light: res_c = res_c + (k c_c) alb_c.
SVO_REFLECT_FN void add_light(float res[3], float k, const float colour[3], const float alb[3]) {
    res[0] = res[0] + (k * colour[0]) * alb[0];
    res[1] = res[1] + (k * colour[1]) * alb[1];
    res[2] = res[2] + (k * colour[2]) * alb[2];
}

// One (record, light) pair on raw records: ray (8 words, svo_ray), hit (6 words, svo_hit), the voxel key.
// out (8 words) = the shadow ray {Q, t_max 1, L, 0} if the record has flag bit 0 and the light is facing and
// in range, else the dead ray (all zero but t_max +inf: invalid by the query's classify).  terms (3 words,
// nullable) = {facing, in range, the bits of k}: all zero without flag bit 0, and k is 0 unless the light
// is facing and in range.  The light's flags are not read: geometry only.
SVO_REFLECT_FN void light_entry(const uint32_t ray[8], const uint32_t hit[6], unsigned long long key, bool raw,
                                const Light &l, uint32_t out[8], uint32_t terms[3]) {
    float org[3] = {0.0f, 0.0f, 0.0f}, dir[3] = {0.0f, 0.0f, 0.0f}, t_max, k = 0.0f;
    const uint32_t inf = 0x7F800000u;
    std::memcpy(&t_max, &inf, sizeof t_max);
    bool facing = false, in_range = false;
    if ((hit[1] >> 16) & 1u) {
        float f[8], t, n[3], sgn, Q[3], L[3], d2, u;
        std::memcpy(f, ray, sizeof f);
        std::memcpy(&t, hit + 2, sizeof t);
        std::memcpy(n, hit + 3, sizeof n);
        float o[3] = {f[0], f[1], f[2]}, d[3] = {f[4], f[5], f[6]};
        svo_reflect::clamp_direction(d, raw);
        const int g = svo_reflect::entry_face(o, d, t, (int)((hit[1] >> 8) & 0xFFu), key, Q, &sgn);
        light_vector(Q, g, sgn, l.position, l.range, L, &d2, &u, &facing, &in_range);
        if (facing && in_range) {
            for (int c = 0; c < 3; ++c) { org[c] = Q[c]; dir[c] = L[c]; }
            t_max = 1.0f;
            k = light_factor(n, L, d2, u);
        }
    }
    std::memcpy(out, org, sizeof org);
    std::memcpy(out + 3, &t_max, sizeof t_max);
    std::memcpy(out + 4, dir, sizeof dir);
    out[7] = 0u;
    if (terms) {
        terms[0] = facing ? 1u : 0u;
        terms[1] = in_range ? 1u : 0u;
        std::memcpy(terms + 2, &k, sizeof k);
    }
}

}  // namespace svo_lights
