// svo_object.h -- the object rule (INTEGRATION.md "Objects"): a sub-SVO of the context's
// pool placed in the world by a position, a rotation and a power-of-two scale, as pure functions: no HIP
// types, no state, host and device, so plain g++ compiles it (tests/object_driver.cpp) and numpy restates
// it (objects.py).  Every operation is one IEEE f32 rounding; the build contracts nothing (no fma); only
// + - * /, compares and selects.
//
// A world ray (o, d, t_max) and an object (root, k, p, R), s = 2^-k (exact):
//  1. classify the world ray as svo_trace_rays does (valid_ray): invalid rays have no candidate anywhere.
//  2. q_i = o_i - p_i; o'_j = ((R_0j q_0 + R_1j q_1) + R_2j q_2) s, d'_j = ((R_0j d_0 + R_1j d_1) + R_2j d_2) s
//     (object_ray).  Origin and direction take the same exact scale: the ray parameter is shared, a record's
//     t / 64 is the world ray's own parameter for the terrain and for every object.
//  3. the object ray {o', t_max, d', 0} is classified again (d' can underflow to zero, o' can overflow):
//     invalid means no candidate in this object.  Unless raw, the small-direction clamp applies to d'.
//  4. cube test (cube_span, cube_test): t_in / t_out = the walk's own entry (after its max(.., 0)) and exit
//     of the object's cube for the clamped object ray, t_entry = fl(fl(32 t_in) 64).  The object is walked
//     iff t_in <= t_out (ordered) and (the best record so far is a miss or t_entry < best.t).
//  5. the walk is the query's, started at parent = root, then the query's t (1 / 64) <= t_max filter.  The
//     record's normal is rotated to world: n_i = (R_i0 m_0 + R_i1 m_1) + R_i2 m_2 (world_normal), not
//     renormalised; position and voxel key stay object-local.
//  6. fold (replaces): candidates in the order terrain, objects 0 .. n - 1; a later hit replaces the best
//     iff the best is a miss or its t < the best t (ordered, strict: ties keep the earlier candidate).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SVO_OBJECT_FN __host__ __device__ inline
#else
#define SVO_OBJECT_FN inline
#endif

namespace svo_objects {

constexpr int MAX_OBJECTS = 8;
constexpr int MAX_SCALE_LOG2 = 8;

struct Object {   // == svo_object
    uint32_t root;
    int32_t scale_log2;
    uint32_t flags;
    float position[3];
    float rotation[9];   // row-major R, world = R * object
    uint32_t reserved;
};
static_assert(sizeof(Object) == 64, "svo_object layout");

// Why svo_set_objects / svo_trace_scene refuse an object (host only: the orthonormality check runs in
// float64); null: valid.  The root's bound is the context's capacity and is checked by the caller.
inline const char *object_error(const Object &ob) {
    if (ob.scale_log2 < -MAX_SCALE_LOG2 || ob.scale_log2 > MAX_SCALE_LOG2) return "scale_log2 must lie in [-8, 8]";
    if (ob.flags != 0u) return "unknown object flag bits";
    if (ob.reserved != 0u) return "reserved must be 0";
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(ob.position[k]) <= 0x1p20f)) return "position components must be finite and lie in [-2^20, 2^20]";
    double r[9];
    for (int k = 0; k < 9; ++k) {
        if (!std::isfinite(ob.rotation[k])) return "rotation entries must be finite";
        r[k] = (double)ob.rotation[k];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = r[3 * i] * r[3 * j] + r[3 * i + 1] * r[3 * j + 1] + r[3 * i + 2] * r[3 * j + 2] - (i == j ? 1.0 : 0.0);
            if (!(std::fabs(e) <= 0x1p-10)) return "rotation must be orthonormal (R R^T - I within 2^-10)";
        }
    const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
    if (!(det > 0.0)) return "rotation must have a positive determinant";
    return nullptr;
}

SVO_OBJECT_FN bool finite_f32(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// The query's classify (svo_kernel.hip query_ray): false for a non-finite component, a NaN t_max or an
// all-zero direction.
SVO_OBJECT_FN bool valid_ray(const float o[3], const float d[3], float t_max) {
    bool ok = !(t_max != t_max) && !(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f);
    for (int k = 0; k < 3; ++k) ok = ok && finite_f32(o[k]) && finite_f32(d[k]);
    return ok;
}

// s = 2^-k as an f32 (exact for k in [-8, 8]).
SVO_OBJECT_FN float inv_scale(int k) {
    const uint32_t b = (uint32_t)(127 - k) << 23;
    float s;
    std::memcpy(&s, &b, sizeof s);
    return s;
}

// Step 2: the world ray (o, d) in the object's frame, before the clamp.  o2 / d2 must not alias o / d.
SVO_OBJECT_FN void object_ray(const float o[3], const float d[3], const Object &ob, float o2[3], float d2[3]) {
    const float s = inv_scale(ob.scale_log2);
    const float *R = ob.rotation;
    const float q0 = o[0] - ob.position[0], q1 = o[1] - ob.position[1], q2 = o[2] - ob.position[2];
    for (int j = 0; j < 3; ++j) {
        float a = R[j] * q0;
        a = a + R[3 + j] * q1;
        a = a + R[6 + j] * q2;
        o2[j] = a * s;
        float b = R[j] * d[0];
        b = b + R[3 + j] * d[1];
        b = b + R[6 + j] * d[2];
        d2[j] = b * s;
    }
}

// Step 4's span: the walk's own cube entry and exit (svo_kernel.hip setup_ray: t_min after its max(.., 0)
// and t_max) of the object ray (o2, d2 after the clamp).  max / min as ordered selects that skip a NaN
// operand, as fmaxf / fminf do; the sign of a zero result is not defined by the walk's fmaxf and never
// reaches a compare.
SVO_OBJECT_FN float sel_max(float a, float b) { return (a > b || b != b) ? a : b; }
SVO_OBJECT_FN float sel_min(float a, float b) { return (a < b || b != b) ? a : b; }
SVO_OBJECT_FN void cube_span(const float o2[3], const float d2[3], float *t_in, float *t_out) {
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        const float x = o2[k] * (1.0f / 32.0f) + 1.5f;
        const float coef = 1.0f / -std::fabs(d2[k]);
        float bias = coef * x;
        if (d2[k] > 0.0f) bias = 3.0f * coef - bias;
        lo[k] = 2.0f * coef - bias;
        hi[k] = coef - bias;
    }
    const float tmin = sel_max(sel_max(lo[0], lo[1]), lo[2]);
    *t_out = sel_min(sel_min(hi[0], hi[1]), hi[2]);
    *t_in = tmin > 0.0f ? tmin : 0.0f;   // fmaxf(tmin, 0): a NaN gives 0
}

// t_entry: the record t (2048 x SVO t) of the cube's entry, rounded as a record's t is.
SVO_OBJECT_FN float entry_t(float t_in) { return (t_in * 32.0f) * 64.0f; }

// Step 4's decision.  best_hit / best_t: flag bit 0 and t of the best record so far.
SVO_OBJECT_FN bool cube_test(float t_in, float t_out, bool best_hit, float best_t) {
    return t_in <= t_out && (!best_hit || entry_t(t_in) < best_t);
}

// Step 5's normal: world = R * object, the record normal m of the walk; n must not alias m.
SVO_OBJECT_FN void world_normal(const float R[9], const float m[3], float n[3]) {
    for (int i = 0; i < 3; ++i) {
        float a = R[3 * i] * m[0];
        a = a + R[3 * i + 1] * m[1];
        a = a + R[3 * i + 2] * m[2];
        n[i] = a;
    }
}

// Step 6: does a candidate that hit at cand_t replace the best record so far?
SVO_OBJECT_FN bool replaces(bool best_hit, float best_t, float cand_t) { return !best_hit || cand_t < best_t; }

// One entry of svo_object_rays on a raw record: ray (8 words, svo_ray); out (8 words, may alias ray) = the
// object ray {o', t_max, d', 0} before the clamp, or svo_bounce_rays' dead ray (all zero but t_max +inf)
// when the world ray is invalid.
SVO_OBJECT_FN void object_entry(const uint32_t ray[8], const Object &ob, uint32_t out[8]) {
    float f[8];
    std::memcpy(f, ray, sizeof f);
    const float o[3] = {f[0], f[1], f[2]}, d[3] = {f[4], f[5], f[6]};
    float o2[3] = {0.0f, 0.0f, 0.0f}, d2[3] = {0.0f, 0.0f, 0.0f};
    uint32_t t_word = 0x7F800000u;
    if (valid_ray(o, d, f[3])) {
        object_ray(o, d, ob, o2, d2);
        t_word = ray[3];
    }
    std::memcpy(out, o2, sizeof o2);
    out[3] = t_word;
    std::memcpy(out + 4, d2, sizeof d2);
    out[7] = 0u;
}

}  // namespace svo_objects
