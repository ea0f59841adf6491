// svo_closest.h -- the closest-voxel rule (INTEGRATION.md "Closest voxels"): which result voxel of a pool is
// nearest to a world-space point, how far it is (squared) and where its closest point lies, as pure functions:
// no HIP types, no state, host and device, so plain g++ compiles it (tests/closest_driver.cpp) and Python
// restates it (closest.py).  Every operation is one IEEE f32 rounding; the build contracts nothing.  Only
// + - *, compares and selects: no sqrt and no division -- the query reports d2, the caller takes the root.
//
// Query: an svo_shape of kind SHAPE_SPHERE, centre p, search radius q[0].  Invalid under shape_valid's rule, and
// also when its kind is SHAPE_BOX; an invalid query is not walked (flags FLAG_INVALID, visits 0, nothing found,
// mask bit 0).  r2 = q[0] q[0]; with UNBOUNDED the radius is ignored, r2 = +inf (the radius must still be valid).
//
// Frame, boxes, slots and the child descriptor index are svo_overlap.h's: the cube [-16, 16]^3, a child at
// level L with integer coordinates i has side = 2^(5 - L), lo_k = i_k side - 16, hi_k = lo_k + side, exact.
//
// Distance to a voxel box [lo, hi]: e_k = max(max(lo_k - p_k, p_k - hi_k), 0), d2 = (e0 e0 + e1 e1) + e2 e2 --
// the sphere touch test's expression in its order.  A voxel is a candidate iff d2 <= r2, so with the same shape
// "something found" equals svo_overlap_volumes' touch bit.  Result voxels are the overlap walk's: a valid child
// whose non-leaf bit is clear or whose level is coarse_level (when non-zero); a non-leaf child at MAX_LEVEL sets
// FLAG_OVERFLOW and is not entered.  The answer is the result voxel with the smallest (d2, Morton position).
// Morton position: with the aligned coordinates a_k = i_k << (22 - level), A precedes B iff, on the axis whose
// a_k ^ b_k has the highest set bit (bit positions tying: z before y before x), A's coordinate is the smaller
// -- the order in which svo_overlap_volumes reports disjoint voxels.
//
// The walk: depth-first from `root`.  bound starts at r2 and becomes the best d2 once a result voxel is found;
// the best is replaced iff the new d2 is smaller, or equal and Morton-earlier.  At a descriptor the pending
// children are the valid ones; repeatedly the pending child with the smallest (d2_c, slot c) among those with
// d2_c <= bound is taken, tested against the bound as it stands at that pick, the others dropping out as the
// bound shrinks.  When the walk returns to a descriptor the children's d2 are recomputed from (level, i); the
// stack entry stays overlap's (node, first, nonleaf | pending << 8).  `visits` counts descriptor fetches; a fetch
// that would make it exceed max_visits sets FLAG_BUDGET and ends the walk with the best so far, which may then
// not be the nearest.  An index at or past the uploaded nodes reads the zero descriptor (the caller's fetch).
// MAX_LEVEL and STACK_LEVELS are overlap's, so the walk ends on cyclic and over-deep pools.
//
// The walk is exact: it returns the voxel a brute force over all result voxels returns under the same f32
// expression, byte for byte.  Proof.  (1) Monotonicity (svo_overlap.h's lemma): a child's box lies inside its
// parent's, differences are rounded once and rounding is monotone, max, the square of a non-negative number
// and the sum are monotone under rounding, so d2 of a child is >= d2 of its parent, hence d2 of any
// descendant >= d2 of any ancestor.  (2) bound never grows, and at every moment bound >= d2 of the final
// answer V* when there is one: it starts at r2 >= d2(V*) (V* is a candidate) and is afterwards the d2 of some
// result voxel the walk met, which is >= the minimum.  (3) A child is skipped only when d2_child > bound at
// some moment -- a pick passing it over, or its parent being left with it pending -- and bound only shrinks,
// so the test would fail at every later moment as well.  By (1) every descendant of a skipped child has
// d2 > bound >= d2(V*), so it is not V* and not tied with it.  Ties are entered: d2_child == bound passes the
// test, so every result voxel with d2 == d2(V*) has all its ancestors entered (their d2 <= d2(V*) <= bound by
// (1) and (2)) and is met.  (4) Of the voxels met, the best kept is the minimum of (d2, Morton position), a
// total order on disjoint voxels, and a minimum does not depend on the order of the comparisons.  Hence
// without FLAG_BUDGET the answer is independent of the visiting order and equals the brute force; the order is
// fixed nonetheless, so that `visits` and the budget are deterministic.  FLAG_OVERFLOW voxels are no result
// voxels in either statement.
//
// Closest point: c_k = min(max(p_k, lo_k), hi_k), one of three f32 numbers, exact.  d2 == 0 iff the point lies
// in or on the voxel.
//
// Against real arithmetic.  With u = 2^-24 and no e_k e_k underflowing or overflowing (every |e_k| is 0 or
// lies in [2^-63, 2^63]), every term e_k e_k carries three roundings (the difference, counted twice by the
// square, and the product) and at most two more from the sums, so
// d2 = D (1 + t), |t| <= (1 + u)^5 - 1 =: g < 5.000002 u, D the true squared distance of that voxel.  Let V be
// the answer and M the voxel of the true minimum D_min.  d2(V) <= d2(M) <= (1 + g) D_min and
// d2(V) >= (1 - g) D(V) >= (1 - g) D_min, and D(V) <= d2(V) / (1 - g) <= D_min (1 + g) / (1 - g).  Both
// |d2(V) - D_min| and D(V) - D_min are therefore at most D_min (2 g / (1 - g)) < D_min 11 u:
// D2_REL_UNITS units of 2^-24, the bound tests/test_closest.py asserts.
#pragma once

#include "svo_overlap.h"

namespace svo_nearest {

using svo_volumes::Contact;
using svo_volumes::Node;
using svo_volumes::Shape;
using svo_volumes::MAX_LEVEL;
using svo_volumes::STACK_LEVELS;
using svo_volumes::DEFAULT_VISITS;
using svo_volumes::MAX_VISITS;

constexpr uint32_t UNBOUNDED = 1u;                      // SVO_CLOSEST_UNBOUNDED: r2 = +inf
constexpr uint32_t FLAG_FOUND = 1u, FLAG_BUDGET = 2u, FLAG_OVERFLOW = 4u, FLAG_INVALID = 0x10u;
constexpr int D2_REL_UNITS = 11;                        // |d2 - D_min| <= D_min D2_REL_UNITS 2^-24 (see above)

struct Closest {                   // == svo_closest
    float point[3];                // closest point on the voxel's closed box; not found: 0, 0, 0
    float d2;                      // squared distance by the rule; not found: +inf
    uint32_t parent, meta;         // as Contact; not found: 0xFFFFFFFF, 0
    uint32_t visits, flags;
};
static_assert(sizeof(Closest) == 32, "svo_closest layout");

SVO_OVERLAP_FN float inf_f32() {
    union { float f; uint32_t u; } b;
    b.u = 0x7F800000u;
    return b.f;
}

SVO_OVERLAP_FN Closest nothing_found(uint32_t visits, uint32_t flags) {
    return {{0.0f, 0.0f, 0.0f}, inf_f32(), 0xFFFFFFFFu, 0u, visits, flags};
}

// A query is a valid sphere: shape_valid's rule, and a box is no query.
SVO_OVERLAP_FN bool query_valid(const Shape &s) { return s.kind == svo_volumes::SHAPE_SPHERE && svo_volumes::shape_valid(s); }

// e_k e_k of the low and of the high half per axis, for the eight children of the descriptor at `level` with
// coordinates i: the children's planes are lo, mid = lo + half and hi = lo + side of the descriptor's own box
// (exact, and equal to each child's lo_k = j_k half - 16, hi_k = lo_k + half) -- touch8's numbers.
SVO_OVERLAP_FN void halves_sq(const float p[3], int level, const uint32_t i[3], float el[3], float eh[3]) {
    const float side = svo_volumes::side_of(level), half = svo_volumes::side_of(level + 1);
    for (int k = 0; k < 3; ++k) {
        const float lo = (float)i[k] * side - 16.0f, mid = lo + half, hi = lo + side;
        const float a = svo_volumes::max_f(svo_volumes::max_f(lo - p[k], p[k] - mid), 0.0f);
        const float b = svo_volumes::max_f(svo_volumes::max_f(mid - p[k], p[k] - hi), 0.0f);
        el[k] = a * a;
        eh[k] = b * b;
    }
}

// d2 of slot c from halves_sq's numbers: (e0 e0 + e1 e1) + e2 e2.
SVO_OVERLAP_FN float slot_d2(const float el[3], const float eh[3], uint32_t c) {
    const float x = (c & 1u) ? eh[0] : el[0], y = (c & 2u) ? eh[1] : el[1], z = (c & 4u) ? eh[2] : el[2];
    return (x + y) + z;
}

// Morton position: does the voxel (level_a, a) precede (level_b, b)?  Equal corners: no.
SVO_OVERLAP_FN bool morton_before(int level_a, const uint32_t a[3], int level_b, const uint32_t b[3]) {
    uint32_t aa[3], bb[3];
    for (int k = 0; k < 3; ++k) {
        aa[k] = a[k] << (MAX_LEVEL - level_a);
        bb[k] = b[k] << (MAX_LEVEL - level_b);
    }
    int axis = 2;
    uint32_t m = aa[2] ^ bb[2];
    for (int k = 1; k >= 0; --k) {
        const uint32_t x = aa[k] ^ bb[k];
        if (m < x && m < (m ^ x)) {   // x's highest set bit lies above m's
            axis = k;
            m = x;
        }
    }
    return aa[axis] < bb[axis];
}

// The walk of one valid query.  fetch(index) gives the Node (the caller guards the index: at or past the
// uploaded nodes it is the zero descriptor); stack.push(level, node, first, state) and stack.pop(level, ..)
// keep one entry per ancestor level 0 .. STACK_LEVELS - 1 (state: nonleaf8 | pending slots << 8).  max_visits
// is the resolved budget (>= 1).  `contact` receives the answer's contact record, or the unused one.
template <class Fetch, class Stack>
SVO_OVERLAP_FN Closest walk(const Shape &s, uint32_t root, uint32_t flags, uint32_t max_visits, uint32_t coarse_level,
                            Fetch &fetch, Stack &stack, Contact &contact) {
    float bound = (flags & UNBOUNDED) ? inf_f32() : s.q[0] * s.q[0];
    uint32_t visits = 0u, fl = 0u;
    uint32_t best_parent = 0xFFFFFFFFu, best_meta = 0u, best_i[3] = {0u, 0u, 0u};
    int best_level = 0;            // 0: nothing found yet (a result voxel's level is >= 1)
    uint32_t node = root, first = 0u, nonleaf = 0u, pend = 0u;
    uint32_t i[3] = {0u, 0u, 0u};
    int level = 0;
    bool enter = true, stale = true;   // stale: el, eh are not this descriptor's
    float el[3], eh[3];
    for (;;) {
        if (enter) {
            if (visits >= max_visits) {
                fl |= FLAG_BUDGET;
                break;
            }
            visits += 1u;
            const Node d = fetch(node);
            first = d.first;
            nonleaf = d.word & 0xFFu;
            pend = (d.word >> 8) & 0xFFu;
            enter = false;
        }
        // the pick: the smallest (d2_c, c) among the pending children with d2_c <= bound; the others drop out
        if (stale) halves_sq(s.p, level, i, el, eh);
        stale = false;
        uint32_t c = 8u, keep = 0u;
        float d2 = 0.0f;
        for (uint32_t k = 0u; k < 8u; ++k) {
            const float dk = slot_d2(el, eh, k);
            const bool ok = ((pend >> k) & 1u) && dk <= bound;
            keep |= ok ? 1u << k : 0u;
            if (ok && (c == 8u || dk < d2)) {
                c = k;
                d2 = dk;
            }
        }
        if (c == 8u) {
            if (level == 0) break;
            level -= 1;
            for (int k = 0; k < 3; ++k) i[k] >>= 1;
            uint32_t state;
            stack.pop(level, node, first, state);
            nonleaf = state & 0xFFu;
            pend = state >> 8;
            stale = true;
            continue;
        }
        const uint32_t bit = 1u << c;
        pend = keep & ~bit;
        const int child_level = level + 1;
        if (!(nonleaf & bit) || (uint32_t)child_level == coarse_level) {
            uint32_t j[3];
            for (int k = 0; k < 3; ++k) j[k] = 2u * i[k] + ((c >> k) & 1u);
            if (best_level == 0 || d2 < bound || morton_before(child_level, j, best_level, best_i)) {   // else d2 == bound
                bound = d2;
                best_parent = node;
                best_meta = c | (uint32_t)(23 - child_level) << 8;
                best_level = child_level;
                for (int k = 0; k < 3; ++k) best_i[k] = j[k];
            }
        } else if (child_level == MAX_LEVEL) {
            fl |= FLAG_OVERFLOW;
        } else {
            stack.push(level, node, first, nonleaf | pend << 8);
            node = first + (uint32_t)__builtin_popcount(nonleaf & (bit - 1u));
            for (int k = 0; k < 3; ++k) i[k] = 2u * i[k] + ((c >> k) & 1u);
            level = child_level;
            enter = stale = true;
        }
    }
    if (best_level == 0) {
        contact = svo_volumes::unused_contact();
        return nothing_found(visits, fl);
    }
    Closest r;
    const float side = svo_volumes::side_of(best_level);
    contact.parent = best_parent;
    contact.meta = best_meta;
    contact.key = 0ull;
    for (int k = 0; k < 3; ++k) {
        const float lo = (float)best_i[k] * side - 16.0f, hi = lo + side;
        const float up = s.p[k] > lo ? s.p[k] : lo;
        r.point[k] = up < hi ? up : hi;
        contact.key |= (unsigned long long)best_i[k] << (21 * k);
    }
    r.d2 = bound;
    r.parent = best_parent;
    r.meta = best_meta;
    r.visits = visits;
    r.flags = fl | FLAG_FOUND;
    return r;
}

}  // namespace svo_nearest
