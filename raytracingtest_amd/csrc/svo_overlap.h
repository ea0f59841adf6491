// svo_overlap.h -- the overlap rule (INTEGRATION.md "Volume queries"): which voxels of a pool does a
// world-space box or sphere touch, as pure functions: no HIP types, no state, host and device, so plain g++
// compiles it (tests/overlap_driver.cpp) and Python restates it (overlap.py).  Every operation is one IEEE
// f32 rounding; the build contracts nothing.  Only + - *, compares and selects.
//
// Frame: the tree's own world convention, the cube [-16, 16]^3.  The root descriptor is level 0; a child at
// level L with integer coordinates i has side = 2^(5 - L), lo_k = i_k side - 16, hi_k = lo_k + side -- all
// exact in f32 (i_k < 2^22, dyadic).  Slot c of a descriptor is the child at offset (c & 1, c >> 1 & 1,
// c >> 2 & 1), un-mirrored (SVOData.leaf_voxels' convention); its descriptor is
// first + popcount(nonleaf8 & ((1 << c) - 1)).
//
// Touch test of a node box [lo, hi] (closed):
//   box [p, q]:    lo_k <= q_k and hi_k >= p_k for every k -- compares of exact numbers;
//   sphere (p, r): e_k = max(max(lo_k - p_k, p_k - hi_k), 0), d2 = (e0 e0 + e1 e1) + e2 e2, touch iff
//                  d2 <= r r (ordered).
// Pruning is exact.  A child's box lies inside its parent's: lo_child >= lo_parent and hi_child <= hi_parent
// per axis.  For the box test each compare that holds for the child then holds for the parent.  For the
// sphere, lo - p and p - hi are exact differences rounded once, and rounding is monotone, so
// fl(lo_child - p) >= fl(lo_parent - p) and fl(p - hi_child) >= fl(p - hi_parent); max, the square of a
// non-negative number and the sum are monotone under rounding too, so e_k, e_k e_k and d2 of the child are
// >= the parent's.  A parent that fails the test therefore has no descendant that passes it, and the pruned
// walk reports exactly the leaves a brute force over all leaves reports under the same f32 test.
//
// The walk: depth-first from `root`, slots 0 .. 7 ascending, so results come out in Morton order.  `visits`
// counts descriptor fetches; a fetch that would make it exceed max_visits sets FLAG_BUDGET and ends the walk
// with what was found so far.  A valid child that touches is a result voxel if its non-leaf bit is clear or
// its level is coarse_level (when non-zero); else, at MAX_LEVEL, it sets FLAG_OVERFLOW and is not entered;
// else it is entered.  MAX_LEVEL is the depth limit of the guarded ray walk (svo_traverse.h: scale
// S_MAX - MAX_LEVEL = 1, one below the floor of the 21-slot stack), so the walk's own stack of STACK_LEVELS
// ancestors cannot overflow and it ends on cyclic and over-deep pools: nothing about a pool needs validating.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SVO_OVERLAP_FN __host__ __device__ inline
#else
#define SVO_OVERLAP_FN inline
#endif

namespace svo_volumes {

constexpr uint32_t SHAPE_BOX = 0u, SHAPE_SPHERE = 1u;   // SVO_SHAPE_BOX, SVO_SHAPE_SPHERE
constexpr uint32_t ANY = 1u;                            // SVO_OVERLAP_ANY: stop at the first result voxel
constexpr uint32_t FLAG_TOUCH = 1u, FLAG_BUDGET = 2u, FLAG_OVERFLOW = 4u, FLAG_INVALID = 0x10u;
constexpr uint32_t MAX_CONTACTS = 32u;
constexpr uint32_t DEFAULT_VISITS = 65536u, MAX_VISITS = 1u << 24;
constexpr int MAX_LEVEL = 22;      // a non-leaf child at this level is not entered (FLAG_OVERFLOW)
constexpr int STACK_LEVELS = 21;   // ancestors of a descriptor at level MAX_LEVEL - 1: levels 0 .. 20

struct Shape {                     // == svo_shape
    float p[3];                    // box: the low corner; sphere: the centre
    uint32_t kind;
    float q[3];                    // box: the high corner; sphere: q[0] the radius, q[1] = q[2] = 0
    uint32_t reserved;
};
static_assert(sizeof(Shape) == 32, "svo_shape layout");

struct Contact {                   // == svo_contact
    uint32_t parent;               // the descriptor holding the voxel
    uint32_t meta;                 // hit_idx | hit_scale << 8: the slot, 23 - the voxel's level
    unsigned long long key;        // x | y << 21 | z << 42 of the voxel's integer coordinates at its level
};
static_assert(sizeof(Contact) == 16, "svo_contact layout");

struct Summary {                   // == svo_overlap
    uint32_t count, visits, flags, reserved;
};
static_assert(sizeof(Summary) == 16, "svo_overlap layout");

struct Node {                      // a descriptor as the walk reads it
    uint32_t word;                 // valid8 << 8 | nonleaf8
    uint32_t first;                // absolute index of the first non-leaf child's descriptor
};

SVO_OVERLAP_FN Contact unused_contact() { return {0xFFFFFFFFu, 0u, ~0ull}; }

SVO_OVERLAP_FN bool finite_f32(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7F800000u) != 0x7F800000u;
}

// A shape is invalid with a non-finite number among p and q, p_k > q_k in a box, a negative radius or an
// unknown kind.  An invalid shape is not walked: count 0, FLAG_INVALID, no contacts, mask bit 0.
SVO_OVERLAP_FN bool shape_valid(const Shape &s) {
    bool ok = s.kind == SHAPE_BOX || s.kind == SHAPE_SPHERE;
    for (int k = 0; k < 3; ++k) ok = ok && finite_f32(s.p[k]) && finite_f32(s.q[k]);
    if (s.kind == SHAPE_BOX)
        for (int k = 0; k < 3; ++k) ok = ok && !(s.p[k] > s.q[k]);
    else
        ok = ok && !(s.q[0] < 0.0f);
    return ok;
}

// 2^(5 - level) for level in 0 .. 23, exact.
SVO_OVERLAP_FN float side_of(int level) {
    union { float f; uint32_t u; } b;
    b.u = (uint32_t)(127 + 5 - level) << 23;
    return b.f;
}

SVO_OVERLAP_FN float max_f(float a, float b) { return a > b ? a : b; }

// Bits (low half, high half) of one axis spread over the eight slots: axis 0 alternates every slot.
SVO_OVERLAP_FN uint32_t spread_axis(bool low, bool high, int axis) {
    const uint32_t lo_bits = axis == 0 ? 0x55u : axis == 1 ? 0x33u : 0x0Fu;
    return (low ? lo_bits : 0u) | (high ? (~lo_bits & 0xFFu) : 0u);
}

// The touch test on the eight children of the descriptor at `level` with coordinates i: bit c = the box of
// slot c touches the shape.  The children's planes per axis are lo, mid = lo + half and hi = lo + side of the
// descriptor's own box (exact, and equal to each child's lo_k = j_k half - 16, hi_k = lo_k + half).
SVO_OVERLAP_FN uint32_t touch8(const Shape &s, float r2, int level, const uint32_t i[3]) {
    const float side = side_of(level), half = side_of(level + 1);
    float lo[3], mid[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = (float)i[k] * side - 16.0f;
        mid[k] = lo[k] + half;
        hi[k] = lo[k] + side;
    }
    if (s.kind == SHAPE_BOX) {
        uint32_t m = 0xFFu;
        for (int k = 0; k < 3; ++k)
            m &= spread_axis(lo[k] <= s.q[k] && mid[k] >= s.p[k], mid[k] <= s.q[k] && hi[k] >= s.p[k], k);
        return m;
    }
    float el[3], eh[3];   // e_k squared of the low and of the high half
    for (int k = 0; k < 3; ++k) {
        const float a = max_f(max_f(lo[k] - s.p[k], s.p[k] - mid[k]), 0.0f);
        const float b = max_f(max_f(mid[k] - s.p[k], s.p[k] - hi[k]), 0.0f);
        el[k] = a * a;
        eh[k] = b * b;
    }
    const float s00 = el[0] + el[1], s10 = eh[0] + el[1], s01 = el[0] + eh[1], s11 = eh[0] + eh[1];
    uint32_t m = 0u;
    m |= (s00 + el[2] <= r2) ? 0x01u : 0u;
    m |= (s10 + el[2] <= r2) ? 0x02u : 0u;
    m |= (s01 + el[2] <= r2) ? 0x04u : 0u;
    m |= (s11 + el[2] <= r2) ? 0x08u : 0u;
    m |= (s00 + eh[2] <= r2) ? 0x10u : 0u;
    m |= (s10 + eh[2] <= r2) ? 0x20u : 0u;
    m |= (s01 + eh[2] <= r2) ? 0x40u : 0u;
    m |= (s11 + eh[2] <= r2) ? 0x80u : 0u;
    return m;
}

// The walk of one valid shape.  fetch(index) gives the Node (the caller guards the index: at or past the
// uploaded nodes it is the zero descriptor); stack.push(level, node, first, state) and stack.pop(level, ..)
// keep one entry per ancestor level 0 .. STACK_LEVELS - 1 (state: nonleaf8 | pending slots << 8);
// sink(k, contact) stores result k < max_contacts.  max_visits is the resolved budget (>= 1).
template <class Fetch, class Stack, class Sink>
SVO_OVERLAP_FN Summary walk(const Shape &s, uint32_t root, uint32_t flags, uint32_t max_contacts, uint32_t max_visits,
                            uint32_t coarse_level, Fetch &fetch, Stack &stack, Sink &sink) {
    Summary r = {0u, 0u, 0u, 0u};
    const float r2 = s.q[0] * s.q[0];
    uint32_t node = root, first = 0u, nonleaf = 0u, pend = 0u;
    uint32_t i[3] = {0u, 0u, 0u};
    int level = 0;
    bool enter = true;
    for (;;) {
        if (enter) {
            if (r.visits >= max_visits) {
                r.flags |= FLAG_BUDGET;
                break;
            }
            r.visits += 1u;
            const Node d = fetch(node);
            first = d.first;
            nonleaf = d.word & 0xFFu;
            pend = ((d.word >> 8) & 0xFFu) & touch8(s, r2, level, i);
            enter = false;
        }
        if (pend == 0u) {
            if (level == 0) break;
            level -= 1;
            for (int k = 0; k < 3; ++k) i[k] >>= 1;
            uint32_t state;
            stack.pop(level, node, first, state);
            nonleaf = state & 0xFFu;
            pend = state >> 8;
            continue;
        }
        const uint32_t c = (uint32_t)__builtin_ctz(pend), bit = 1u << c;
        pend &= pend - 1u;
        const int child_level = level + 1;
        if (!(nonleaf & bit) || (uint32_t)child_level == coarse_level) {
            if (r.count < max_contacts) {
                Contact ct;
                ct.parent = node;
                ct.meta = c | (uint32_t)(23 - child_level) << 8;
                ct.key = 0ull;
                for (int k = 0; k < 3; ++k)
                    ct.key |= (unsigned long long)(2u * i[k] + ((c >> k) & 1u)) << (21 * k);
                sink(r.count, ct);
            }
            r.count += 1u;
            if (flags & ANY) break;
        } else if (child_level == MAX_LEVEL) {
            r.flags |= FLAG_OVERFLOW;
        } else {
            stack.push(level, node, first, nonleaf | pend << 8);
            node = first + (uint32_t)__builtin_popcount(nonleaf & (bit - 1u));
            for (int k = 0; k < 3; ++k) i[k] = 2u * i[k] + ((c >> k) & 1u);
            level = child_level;
            enter = true;
        }
    }
    if (r.count) r.flags |= FLAG_TOUCH;
    return r;
}

}  // namespace svo_volumes
