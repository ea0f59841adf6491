// svo_scene_light.h -- the scene-light rule (INTEGRATION.md "Objects in light"): the light
// rule (svo_light.h) for the records of a scene query (svo_trace_scene), whose hit may lie on a placed object
// (svo_object.h): a rotated, scaled voxel.  Pure functions: no HIP types, no state, host and device, so plain
// g++ compiles it (tests/scene_light_driver.cpp) and numpy restates it (scene_light.py).  Every operation is
// one IEEE f32 rounding; the build contracts nothing (no fma); only + - * /, sqrt, compares and selects.
// Nothing of svo_object.h, svo_reflect.h or svo_light.h is redefined here.
//
// (a) Origin and face of a scene hit.  Inputs: the traced world ray (o, d) AS GIVEN, the record (t,
//     hit_scale, the world normal n), the voxel key (object-local for an object) and the object id of
//     svo_trace_scene (-1 a miss, 0 the terrain, c + 1 object c).
//      - id -1, an id outside -1 .. n_objects, or a record without flag bit 0: nothing; every light gets the
//        dead ray.  (A device array of ids cannot be validated on the host; no table entry is read for it.)
//      - id 0: the light rule unchanged.  The clamp applies to d unless raw; svo_reflect::entry_face gives
//        g, out and Q; the face normal is N = out e_g.
//      - id c + 1, ob = objects[c] = (k, p, R):
//         1. (o', d') = svo_objects::object_ray(o, d, ob) from the world ray as given, then the
//            small-direction clamp on d' unless raw: the ray the scene query walked in the object.
//         2. (g, out, Q') = svo_reflect::entry_face(o', d', t, hit_scale, key).  The parameter t is shared
//            between the frames and the object frame's cube is the world convention's [-16, 16]^3, so the
//            function applies as it is.
//         3. Q_i = (((R_i0 Q'_0 + R_i1 Q'_1) + R_i2 Q'_2) 2^k) + p_i (the factor 2^k is exact);
//            N_i = out R_ig (exact: out = +-1): the entered face's outward normal in world space.
// (b) Toward a light (p_l, range, colour): L = p_l - Q.  An object hit is facing iff
//     (N_0 L_0 + N_1 L_1) + N_2 L_2 > 0 (ordered); the terrain keeps L_g out > 0.  d2, u and "in range" are
//     svo_lights::light_vector's.  Not facing, or out of range: the dead ray.  Otherwise the ray is
//     {Q, t_max 1, L, 0}, and the factor is svo_lights::light_factor(n, L, d2, u) with the record's world
//     normal n.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "svo_light.h"
#include "svo_object.h"

namespace svo_scene_light {

// What (a) gives for one hit: the shadow rays' common origin Q, the entered face's world normal N, and for
// the terrain its axis g and sign out (N = out e_g).
struct Face {
    float Q[3], N[3], out;
    int g;
    bool terrain;
};

// 2^k as an f32 (exact for k in [-8, 8]): svo_objects::inv_scale of -k.
SVO_OBJECT_FN float scale_of(int k) { return svo_objects::inv_scale(-k); }

// (a) for the terrain: (o, d) the world ray as given; the clamp unless raw.
SVO_OBJECT_FN void terrain_face(const float o[3], const float d[3], bool raw, float t, int scale, unsigned long long key,
                                Face &f) {
    float dc[3] = {d[0], d[1], d[2]};
    svo_reflect::clamp_direction(dc, raw);
    f.g = svo_reflect::entry_face(o, dc, t, scale, key, f.Q, &f.out);
    f.N[0] = f.g == 0 ? f.out : 0.0f;
    f.N[1] = f.g == 1 ? f.out : 0.0f;
    f.N[2] = f.g == 2 ? f.out : 0.0f;
    f.terrain = true;
}

// (a) steps 1-3 for an object hit: (o, d) the world ray as given.  No array is indexed by g.
SVO_OBJECT_FN void object_face(const float o[3], const float d[3], bool raw, float t, int scale, unsigned long long key,
                               const svo_objects::Object &ob, Face &f) {
    float o2[3], d2[3], Qp[3];
    svo_objects::object_ray(o, d, ob, o2, d2);
    svo_reflect::clamp_direction(d2, raw);
    f.g = svo_reflect::entry_face(o2, d2, t, scale, key, Qp, &f.out);
    const float s = scale_of(ob.scale_log2);
    const float *R = ob.rotation;
    for (int i = 0; i < 3; ++i) {
        float a = R[3 * i] * Qp[0];
        a = a + R[3 * i + 1] * Qp[1];
        a = a + R[3 * i + 2] * Qp[2];
        f.Q[i] = a * s + ob.position[i];
        const float R_ig = f.g == 0 ? R[3 * i] : f.g == 1 ? R[3 * i + 1] : R[3 * i + 2];
        f.N[i] = f.out * R_ig;
    }
    f.terrain = false;
}

// (b): L, d2, u and in range as svo_lights::light_vector gives them; facing by the face's own test.
SVO_OBJECT_FN void toward_light(const Face &f, const float p[3], float range, float L[3], float *d2, float *u, bool *facing,
                                bool *in_range) {
    bool facing_axis;
    svo_lights::light_vector(f.Q, f.g, f.out, p, range, L, d2, u, &facing_axis, in_range);
    float s = f.N[0] * L[0];
    s = s + f.N[1] * L[1];
    s = s + f.N[2] * L[2];
    *facing = f.terrain ? facing_axis : s > 0.0f;
}

// One (record, light) pair of svo_scene_light_rays on raw records: ray (8 words, svo_ray, the world ray as
// given), hit (6 words, svo_hit, world normal), the voxel key and the object id of svo_trace_scene; objects:
// n_objects entries (nullable with 0).  out (8 words) = the shadow ray {Q, t_max 1, L, 0}, or the dead ray
// (all zero but t_max +inf).  terms (3 words, nullable) = {facing, in range, the bits of k} as
// svo_lights::light_entry gives them.  The light's flags are not read: geometry only.
SVO_OBJECT_FN void scene_light_entry(const uint32_t ray[8], const uint32_t hit[6], unsigned long long key, int32_t id, bool raw,
                                     const svo_objects::Object *objects, int n_objects, const svo_lights::Light &l,
                                     uint32_t out[8], uint32_t terms[3]) {
    float org[3] = {0.0f, 0.0f, 0.0f}, dir[3] = {0.0f, 0.0f, 0.0f}, t_max, k = 0.0f;
    const uint32_t inf = 0x7F800000u;
    std::memcpy(&t_max, &inf, sizeof t_max);
    bool facing = false, in_range = false;
    if (((hit[1] >> 16) & 1u) && id >= 0 && id <= n_objects) {
        float fr[8], t, n[3], L[3], d2, u;
        std::memcpy(fr, ray, sizeof fr);
        std::memcpy(&t, hit + 2, sizeof t);
        std::memcpy(n, hit + 3, sizeof n);
        const float o[3] = {fr[0], fr[1], fr[2]}, d[3] = {fr[4], fr[5], fr[6]};
        const int scale = (int)((hit[1] >> 8) & 0xFFu);
        Face f;
        if (id == 0) terrain_face(o, d, raw, t, scale, key, f);
        else object_face(o, d, raw, t, scale, key, objects[id - 1], f);
        toward_light(f, l.position, l.range, L, &d2, &u, &facing, &in_range);
        if (facing && in_range) {
            for (int c = 0; c < 3; ++c) { org[c] = f.Q[c]; dir[c] = L[c]; }
            t_max = 1.0f;
            k = svo_lights::light_factor(n, L, d2, u);
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

}  // namespace svo_scene_light
