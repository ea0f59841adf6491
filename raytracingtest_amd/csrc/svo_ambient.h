// svo_ambient.h -- the ambient rule (INTEGRATION.md "Ambient"): from a traced ray and its
// hit to the N hemisphere rays that leave the voxel face the ray entered by, as pure functions: no HIP
// types, no state, host and device, so plain g++ compiles it (tests/ambient_driver.cpp) and numpy restates
// it (ambient.py ambient_rays).  Every operation is one IEEE f32 rounding; the build contracts nothing.
//
// Deviation from the reference (documented): the reference has no ambient term.  The rays are distributed
// about the normal of the entry face, not the smooth normal: a ray's direction is then a permutation of a
// table entry with one sign, and in real arithmetic no hemisphere ray can re-enter the voxel it left.  In f32
// that is derived for pools of up to 12 levels and ends where the bounce origin's promise ends (svo_reflect.h):
// with N = 4 no ray re-entered through 16 levels, 162 of 32,256 did at 17 and 6,884 of 32,008 at 18
// (DESIGN.md 3.2c, 3.2e).  A ray that re-enters counts as occluded.
#pragma once

#include <cstdint>
#include <cstring>

#include "svo_reflect.h"

namespace svo_ambient {

constexpr int MAX_RAYS = 16;      // SVO_AMBIENT_MAX_RAYS
constexpr int TABLE_ROWS = 28;    // 4 + 8 + 16

// n in {4, 8, 16}
SVO_REFLECT_FN bool valid_count(int n) { return n == 4 || n == 8 || n == 16; }

// Entry k of the table for n rays: (a, b, c) = (r cos phi, r sin phi, sqrt(1 - r^2)) with
// r = sqrt((k + 0.5) / n), phi = (k + 0.5) pi (3 - sqrt 5), computed in float64 and rounded once to f32.
// These literals are the truth (ambient.py reads them from this text): every |component| >= 2^-10, so the
// query's small-direction clamp never changes one, and c > 0.  The table for n starts at row n - 4.
// A local constant array: the host reads it as it is, the device through a scalar load when k is uniform.
SVO_REFLECT_FN void table_entry(int n, int k, float e[3]) {
    const float T[TABLE_ROWS][3] = {
        // N = 4
        {0x1.066330p-3f, 0x1.516e8ap-2f, 0x1.deeea2p-1f},
        {-0x1.192c2ap-1f, -0x1.1575c2p-2f, 0x1.94c584p-1f},
        {0x1.84a3a4p-1f, -0x1.c48a6ap-3f, 0x1.3988e2p-1f},
        {-0x1.f14d7ep-2f, 0x1.9953b0p-1f, 0x1.6a09e6p-2f},
        // N = 8
        {0x1.731268p-4f, 0x1.dd335ap-3f, 0x1.efbdecp-1f},
        {-0x1.8da354p-2f, -0x1.886340p-3f, 0x1.cd82b4p-1f},
        {0x1.12cf36p-1f, -0x1.3ffe9cp-3f, 0x1.a8872ap-1f},
        {-0x1.5fa568p-2f, 0x1.217016p-1f, 0x1.800000p-1f},
        {-0x1.2abd74p-3f, -0x1.78aacap-1f, 0x1.52a7fap-1f},
        {0x1.562bcep-1f, 0x1.f690aep-2f, 0x1.1e377ap-1f},
        {-0x1.cacfc4p-1f, 0x1.8eb67ep-4f, 0x1.bb67aep-2f},
        {0x1.473e74p-1f, -0x1.7462d6p-1f, 0x1.000000p-2f},
        // N = 16
        {0x1.066330p-4f, 0x1.516e8ap-3f, 0x1.f7efbep-1f},
        {-0x1.192c2ap-2f, -0x1.1575c2p-3f, 0x1.e768d4p-1f},
        {0x1.84a3a4p-2f, -0x1.c48a6ap-4f, 0x1.d64d52p-1f},
        {-0x1.f14d7ep-3f, 0x1.9953b0p-2f, 0x1.c48c60p-1f},
        {-0x1.a67b72p-4f, -0x1.0a580ap-1f, 0x1.b211b2p-1f},
        {0x1.e3e72cp-2f, 0x1.635e02p-2f, 0x1.9ec474p-1f},
        {-0x1.446dc4p-1f, 0x1.19eebep-4f, 0x1.8a85c2p-1f},
        {0x1.cecaf8p-2f, -0x1.075114p-1f, 0x1.752e50p-1f},
        {0x1.ed83a0p-7f, 0x1.7519ecp-1f, 0x1.5e8adep-1f},
        {-0x1.10734ap-1f, -0x1.1d56fep-1f, 0x1.465656p-1f},
        {0x1.9dd720p-1f, 0x1.bb747ep-5f, 0x1.2c2fc6p-1f},
        {-0x1.52f25ep-1f, 0x1.0f2a8cp-1f, 0x1.0f876cp-1f},
        {0x1.166722p-3f, -0x1.bf2a04p-1f, 0x1.deeea2p-2f},
        {0x1.0491ecp-1f, 0x1.8784e8p-1f, 0x1.94c584p-2f},
        {-0x1.d9367ap-1f, -0x1.d31f1cp-3f, 0x1.3988e2p-2f},
        {0x1.ba52a0p-1f, -0x1.e2eb28p-2f, 0x1.6a09e6p-3f},
    };
    const int row = n - 4 + k;
    e[0] = T[row][0];
    e[1] = T[row][1];
    e[2] = T[row][2];
}

// Direction k of n about the entry face (axis g, out = +-1 as svo_reflect::entry_face gives them):
//   (a, b, c) = table entry k; variant & 4: swap a and b; then variant & 3 times (a, b) -> (-b, a);
//   dir_g = out c, dir_{(g + 1) % 3} = a, dir_{(g + 2) % 3} = b.
// All exact: selects and sign flips.  No array is indexed by g.
SVO_REFLECT_FN void ambient_dir(int n, int k, uint32_t variant, int g, float out, float dir[3]) {
    float e[3];
    table_entry(n, k, e);
    const float a0 = (variant & 4u) ? e[1] : e[0];
    const float b0 = (variant & 4u) ? e[0] : e[1];
    const uint32_t rot = variant & 3u;
    const float a = rot == 0u ? a0 : rot == 1u ? -b0 : rot == 2u ? -a0 : b0;
    const float b = rot == 0u ? b0 : rot == 1u ? a0 : rot == 2u ? -b0 : -a0;
    const float c = out > 0.0f ? e[2] : -e[2];
    dir[0] = g == 0 ? c : g == 1 ? b : a;
    dir[1] = g == 1 ? c : g == 2 ? b : a;
    dir[2] = g == 2 ? c : g == 0 ? b : a;
}

// One entry of svo_ambient_rays on raw records: ray (8 words, svo_ray), hit (6 words, svo_hit), the voxel
// key; out (8 words) = ray k of n, {origin, t_max radius, direction k, 0}, if the record has flag bit 0,
// else the dead ray (all zero but t_max +inf: invalid by the query's classify).
SVO_REFLECT_FN void ambient_entry(const uint32_t ray[8], const uint32_t hit[6], unsigned long long key, bool raw,
                                  int n, int k, float radius, uint32_t variant, uint32_t out[8]) {
    float org[3] = {0.0f, 0.0f, 0.0f}, dir[3] = {0.0f, 0.0f, 0.0f}, t_max;
    const uint32_t inf = 0x7F800000u;
    std::memcpy(&t_max, &inf, sizeof t_max);
    if ((hit[1] >> 16) & 1u) {
        float f[8], t, sgn;
        std::memcpy(f, ray, sizeof f);
        std::memcpy(&t, hit + 2, sizeof t);
        float o[3] = {f[0], f[1], f[2]}, d[3] = {f[4], f[5], f[6]};
        svo_reflect::clamp_direction(d, raw);
        const int g = svo_reflect::entry_face(o, d, t, (int)((hit[1] >> 8) & 0xFFu), key, org, &sgn);
        ambient_dir(n, k, variant, g, sgn, dir);
        t_max = radius;
    }
    std::memcpy(out, org, sizeof org);
    std::memcpy(out + 3, &t_max, sizeof t_max);
    std::memcpy(out + 4, dir, sizeof dir);
    out[7] = 0u;
}

// All n entries of one input: out holds n x 8 words.
SVO_REFLECT_FN void ambient_record(const uint32_t ray[8], const uint32_t hit[6], unsigned long long key, bool raw,
                                   int n, float radius, uint32_t variant, uint32_t *out) {
    for (int k = 0; k < n; ++k) ambient_entry(ray, hit, key, raw, n, k, radius, variant, out + 8 * k);
}

}  // namespace svo_ambient
