// svo_reflect.h -- the bounce rule (INTEGRATION.md "Reflections"): from a traced ray
// and its hit to the specular bounce ray, as pure functions: no HIP types, no state, host and device,
// so plain g++ compiles it (tests/reflect_driver.cpp) and numpy restates it (reflection.py
// bounce_rays).  Every operation is one IEEE f32 rounding; the build contracts nothing (no fma).
//
// Deviation from the reference (documented): Shade (RaytraceCompute.compute:97-104) restarts the ray
// at P + 0.001 n with the smooth normal n.  On voxels that origin very often lies on or inside the
// voxel just hit, and the bounce ray hits it again at t ~ 0.  Here the ray leaves through the cube
// face it entered by, and its direction is mirrored on that face when the smooth normal would send
// it back in.
//
// Where that holds: the origin stands side 2^-6 = 2^-(L + 6) SVO units off the face of a level-L voxel
// (hit_scale = 23 - L).  The addition to face_g is exact down to hit_scale 4; what the step must survive
// is the query's world -> SVO transform o' = fl(o / 32 + 1.5), spaced 2^-23 SVO units (the step is 4, 2,
// 1 and 1/2 of that at 15, 16, 17 and 18 levels), and the walk's plane rounding of up to
// 10 * 2^-23 max(1, |o'|).  Through 12 levels the step exceeds both and no ray of this origin can re-enter
// the voxel it left; none was observed through 15 levels; from 16 levels on some do (DESIGN.md 3.2c has
// the counts by depth, tests/secondary_geometry_model.py the float64 model they come from).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SVO_REFLECT_FN __host__ __device__ inline
#else
#define SVO_REFLECT_FN inline
#endif

namespace svo_reflect {

// Laine-Karras's small-direction clamp of the ray queries (svo_kernel.hip query_ray): the direction
// a query traces.  raw: SVO_QUERY_RAW_DIRECTIONS, the direction as given.
SVO_REFLECT_FN void clamp_direction(float d[3], bool raw) {
    if (raw) return;
    const float eps = 0x1p-23f;
    for (int k = 0; k < 3; ++k)
        if (std::fabs(d[k]) < eps) d[k] = std::copysign(eps, d[k]);
}

// Steps 1-3 of the bounce rule below, shared with the ambient rule (svo_ambient.h): the entry axis g
// (returned), *out = d_g > 0 ? -1 : +1, and org = the origin of a ray that leaves through that face.
// org may alias o; d is only read.
SVO_REFLECT_FN int entry_face(const float o[3], const float d[3], float t, int scale, unsigned long long key,
                              float org[3], float *out) {
    const float side = std::ldexp(1.0f, scale - 18);
    float face[3], te[3];
    for (int k = 0; k < 3; ++k) {
        const float c = (float)(uint32_t)((key >> (21 * k)) & 0x1FFFFFu);
        const float lo = c * side - 16.0f;
        const float hi = lo + side;
        face[k] = d[k] > 0.0f ? lo : hi;
        te[k] = (face[k] - o[k]) * (1.0f / d[k]);
    }
    int g = 0;
    float te_g = te[0];
    if (te[1] > te_g) { g = 1; te_g = te[1]; }
    if (te[2] > te_g) { g = 2; te_g = te[2]; }
    const float d_g = g == 0 ? d[0] : g == 1 ? d[1] : d[2];
    const float face_g = g == 0 ? face[0] : g == 1 ? face[1] : face[2];
    const float sgn = d_g > 0.0f ? -1.0f : 1.0f;
    const float tw = t * (1.0f / 64.0f);
    const float org_g = face_g + sgn * (side * 0x1p-6f);
    for (int k = 0; k < 3; ++k) {
        const float p = o[k] + tw * d[k];
        org[k] = k == g ? org_g : p;
    }
    *out = sgn;
    return g;
}

// The bounce ray of the ray (o, d) AS TRACED (a query's direction after the clamp) and its hit:
// t the record's t (2048 x SVO t), n the record's normal, scale its hit_scale, key its voxel key.
//  1. box:       side = 2^(scale - 18), lo = c side - 16, hi = lo + side (c: the key's coordinates)
//  2. entry face: face_k = d_k > 0 ? lo_k : hi_k, te_k = (face_k - o_k) (1 / d_k), g = the axis of the
//                 largest te (ordered compares from g = 0: a NaN never wins), out = d_g > 0 ? -1 : +1
//  3. origin:    P = o + (t / 64) d off the axis g, face_g + out side 2^-6 on it
//  4. direction: r = d - 2 (n . d) n, and r_g negated if it points into the face; not renormalised
// org and dir may alias o and d.
SVO_REFLECT_FN void bounce(const float o[3], const float d[3], float t, const float n[3], int scale,
                           unsigned long long key, float org[3], float dir[3]) {
    float out;
    const int g = entry_face(o, d, t, scale, key, org, &out);   // writes org only: d and n are still the inputs
    float dn = n[0] * d[0];
    dn = dn + n[1] * d[1];
    dn = dn + n[2] * d[2];
    const float dn2 = 2.0f * dn;
    for (int k = 0; k < 3; ++k) {
        float r = d[k] - dn2 * n[k];
        if (k == g && ((out > 0.0f && r < 0.0f) || (out < 0.0f && r > 0.0f))) r = -r;
        dir[k] = r;
    }
}

// One entry of svo_bounce_rays on raw records: ray (8 words, svo_ray), hit (6 words, svo_hit), the
// voxel key; out (8 words, may alias ray) = the bounce ray {origin, t_max +inf, direction, 0} if the
// record has flag bit 0, else the dead ray (all zero but t_max +inf: a zero direction, invalid by
// the query's classify).
SVO_REFLECT_FN void bounce_record(const uint32_t ray[8], const uint32_t hit[6], unsigned long long key, bool raw,
                                  uint32_t out[8]) {
    float f[8], n[3], t;
    std::memcpy(f, ray, sizeof f);
    std::memcpy(&t, hit + 2, sizeof t);
    std::memcpy(n, hit + 3, sizeof n);
    float org[3] = {0.0f, 0.0f, 0.0f}, dir[3] = {0.0f, 0.0f, 0.0f};
    if ((hit[1] >> 16) & 1u) {
        float o[3] = {f[0], f[1], f[2]}, d[3] = {f[4], f[5], f[6]};
        clamp_direction(d, raw);
        bounce(o, d, t, n, (int)((hit[1] >> 8) & 0xFFu), key, org, dir);
    }
    std::memcpy(out, org, sizeof org);
    out[3] = 0x7F800000u;
    std::memcpy(out + 4, dir, sizeof dir);
    out[7] = 0u;
}

}  // namespace svo_reflect
