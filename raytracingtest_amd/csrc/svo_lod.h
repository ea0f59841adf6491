// svo_lod.h -- the host's rule for the beam starts of a level-of-detail launch (svo_rt.hip
// beam_starts) as a pure function: no HIP, no state, so a CPU test can pin it (tests/test_lod.py).
#pragma once

#include <cmath>
#include <limits>

namespace svo_lod {

// The floor of a LOD launch's beam starts, in double; fine_depth: the finest box of
// the splat list the launch uses (side s_min = 2^-fine_depth).  A LOD hit in a voxel no larger than
// s_min lies inside a listed box, so the splat's bound holds for it.  A hit in a larger voxel (side
// >= 2 s_min) needs tc_max coef + bias >= 2 s_min, and a ray of unit direction crosses a voxel of
// side s in at most sqrt(3) s of t, so its t_min is at least
//   T' = ((2 s_min - bias) / coef) (1 - sqrt(3) coef) - sqrt(3) bias.
// -inf: no bound (the launch skips the splat); +inf (coef == 0, a depth clamp finer than 2 s_min: no
// such hit exists): the beam start alone; else T' less 2^-10 of it, rounded down to f32.
inline float lod_floor(double coef, double bias, int fine_depth) {
    const float inf = std::numeric_limits<float>::infinity();
    const double s_min = std::ldexp(1.0, -fine_depth), r3 = std::sqrt(3.0);
    if (bias >= 2.0 * s_min || r3 * coef >= 1.0) return -inf;
    if (coef == 0.0) return inf;
    const double t = ((2.0 * s_min - bias) / coef) * (1.0 - r3 * coef) - r3 * bias;
    if (!(t > 0.0)) return -inf;
    const double fl = t * (1.0 - std::ldexp(1.0, -10));
    float f = (float)fl;
    if ((double)f > fl) f = std::nextafterf(f, -inf);
    return f;
}

}  // namespace svo_lod
