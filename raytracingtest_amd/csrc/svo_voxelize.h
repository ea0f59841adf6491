// svo_voxelize.h -- the mesh rule (DESIGN.md "Meshes", INTEGRATION.md "Meshes"): which voxels of the 2^d grid
// a triangle makes surface leaves, which triangle owns a leaf, and the leaf's normal and colour, as pure
// functions: no HIP types, no state, host and device, so the builder's kernels (svo_build.hip), plain g++
// (tests/voxelize_driver.cpp) and numpy (voxelize.py) follow it term for term.  Every operation is one IEEE
// f32 rounding; the build contracts nothing (no fma); only + - * /, compares, selects, floor and ceil, and
// normalize_unity's square root through float64.
//
// Frame.  Positions are given in the cube's unit frame [0,1]^3; with n = 2^(max_level-1) the grid coordinate is
// g = p * n (a power of two: exact).  Everything below is in grid units.  Voxel (i,j,k) is the CLOSED box
// [i,i+1] x [j,j+1] x [k,k+1]; a triangle is the closed set of its points.
//
// Setup (setup, once per triangle; v0 v1 v2 the grid vertices, all differences before any product):
//   a = v1 - v0, b = v2 - v0, N = a x b:  N_x = a_y b_z - a_z b_y, N_y = a_z b_x - a_x b_z, N_z = a_x b_y - a_y b_x
//   W = (|N_x| + |N_y|) + |N_z|
//   degenerate  iff  normalize_unity(N) == 0, i.e. not (float)sqrt((double)((N_x N_x + N_y N_y) + N_z N_z)) > 1e-5:
//               the triangle is skipped and counted (svob_mesh_stats.degenerate).
//   mn_c / mx_c = the smaller / larger of the three vertices' coordinate c (ordered selects).
//   box: lo_c = mn_c <= 0 ? 0 : mn_c > n ? n : (int)ceil(mn_c) - 1
//        hi_c = mx_c <  0 ? -1 : mx_c >= n ? n - 1 : (int)floor(mx_c)
//        the voxels of the grid whose closed interval meets [mn_c, mx_c]; empty on an axis (lo_c > hi_c): the
//        triangle is `outside` and counted; candidates = the product of the three (hi_c - lo_c + 1).
//   for each projection q = xy, yz, zx with axes (u, v) = (q, q+1 mod 3) and each edge e (from vertex e to vertex
//   f = e+1 mod 3, opposite vertex g = e+2 mod 3), the edge's normal in the plane and the triangle's interval on it:
//        A_u = -(v_f.v - v_e.v), A_v = v_f.u - v_e.u
//        t   = A_u (v_g.u - v_e.u) + A_v (v_g.v - v_e.v)
//        lo  = t < 0 ? t : 0,   hiw = (t > 0 ? t : 0) + (|A_u| + |A_v|)
//
// Occupancy (overlaps; the voxel's integer coordinates i_c are exact in f32 up to 2^21):
//   1. box        lo_c <= i_c <= hi_c on every axis (integers: the three interval tests, exact)
//   2. plane      c_c = N_c > 0 ? i_c + 1 : i_c (the corner furthest along N);
//                 s = (N_x (c_x - v0_x) + N_y (c_y - v0_y)) + N_z (c_z - v0_z);   0 <= s <= W
//   3. edges      for every q, e:  c_u = A_u > 0 ? i_u + 1 : i_u, c_v likewise;
//                 p = A_u (c_u - v_e.u) + A_v (c_v - v_e.v);   lo <= p <= hiw
//   The voxel is a surface leaf iff some non-degenerate triangle passes 1, 2 and 3.  This is the Schwarz-Seidel
//   triangle/box test in its two-sided form: on each of the 13 separating axes (3 box normals, the plane normal,
//   9 edge normals in the three projections) the furthest box corner must reach the triangle's interval
//   (p >= lo) and the nearest must not lie beyond it (p - (|A_u| + |A_v|) <= hi, folded into hiw).  The one-sided
//   form orients the edge normals by the sign of N's component, which is the sign of a rounded difference of
//   products: two-sided, a projection of almost no area moves an interval's end by its rounding error and no more.
//   Any pruning of candidates is allowed as long as every voxel inside the box reaches 2 and 3.
//
// Error of the rule as written (u = 2^-24, first order; E = the largest coordinate extent mx_c - mn_c of the
// triangle; a voxel inside the box has every corner within E + 1 of every vertex on every axis):
//   every c - v is one rounding of a difference of an exact integer and an f32; every A, a, b one rounding;
//   p and t are sums of two such products: 4 roundings per term, |p^ - p| <= 4u (|A_u| + |A_v|) (E + 1) and
//   |t^ - t| <= 4u (|A_u| + |A_v|) E; hiw adds two sums of magnitude <= (|A_u| + |A_v|) (E + 1).  In units of the
//   box's half extent (an error eps of p moves the decision as a change eps / (|A_u| + |A_v|) of the half
//   extent does):                                         delta_edge  <= 10 u (E + 1).
//   N_c carries |N^_c - N_c| <= 4u P_c, P_c = |a_i b_j| + |a_j b_i| (cancellation: with kappa = sum P_c / sum |N_c|
//   the normal is known to 4u kappa of its 1-norm), s adds 4 roundings per term and W two sums:
//                                                         delta_plane <= 4u (E + 2) (1 + kappa).
//   Both are below                          delta = 10 u (E + 2) (1 + kappa)
//   which tests/voxelize_util.py evaluates per triangle in float64: at most 1.2e-4 voxel for a well-shaped
//   (kappa <= 2) triangle that spans a 64^3 grid.  With must / may = the float64 overlap at half extents
//   1/2 - delta / 1/2 + delta:  must <= leaves <= may.
//
// Owner.  The lowest index among the triangles that pass: min is order-independent, so is everything below.
//
// Attributes of a leaf, from its owner alone:
//   normal  normalize_unity(N) (the builder's: components divided by the magnitude), negated component by
//           component under SVOB_MESH_FLIP_WINDING.  Counter-clockwise front faces give outward normals.
//   colour  (per-vertex rgb given) at the barycentric coordinates of the voxel centre m = i + 0.5 projected
//           onto the owner's plane:  q = m - v0,  D = (N_x N_x + N_y N_y) + N_z N_z,
//             w1 = (((q x b) . N)) / D,  w2 = (((a x q) . N)) / D,  w0 = (1 - w1) - w2
//           (cross products as N above, dots as (x + y) + z), each w clamped below at 0,
//             S = (w0 + w1) + w2,  w_k = w_k / S,   rgb_c = (w0 C0_c + w1 C1_c) + w2 C2_c.
//           The winding flag does not enter.  Without colours the leaf colour is the layout's position - 1.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SVO_VOX_FN __host__ __device__ inline
#else
#define SVO_VOX_FN inline
#endif

namespace svo_voxelize {

constexpr uint32_t NO_OWNER = 0xFFFFFFFFu;
constexpr uint32_t TRI_DEGENERATE = 1u, TRI_OUTSIDE = 2u;

struct Tri {            // the per-triangle constants, 56 words
    float v[3][3];      // grid vertices
    float n[3];         // N = a x b
    float w;            // W
    float a[3][3][2];   // [projection][edge] A_u, A_v
    float lo[3][3];     // [projection][edge]
    float hiw[3][3];
    int32_t blo[3], bhi[3];   // the clipped box (inclusive)
    uint32_t flags;     // TRI_DEGENERATE | TRI_OUTSIDE
};
static_assert(sizeof(Tri) == 56 * 4, "Tri layout");

SVO_VOX_FN float absf(float x) { return x < 0.0f ? -x : x; }

// The builder's normalize_unity (Vector3.Normalize).
SVO_VOX_FN void normalize_unity(float &x, float &y, float &z) {
    const float mag = (float)sqrt((double)((x * x + y * y) + z * z));
    if (mag > 1e-5f) { x = x / mag; y = y / mag; z = z / mag; }
    else { x = 0.0f; y = 0.0f; z = 0.0f; }
}

SVO_VOX_FN void cross(const float p[3], const float q[3], float out[3]) {
    out[0] = p[1] * q[2] - p[2] * q[1];
    out[1] = p[2] * q[0] - p[0] * q[2];
    out[2] = p[0] * q[1] - p[1] * q[0];
}

SVO_VOX_FN float dot3(const float p[3], const float q[3]) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

// p: the triangle's three positions in the unit frame (9 floats, finite), n = 2^(max_level-1).
SVO_VOX_FN void setup(const float p[9], int n, Tri *t) {
    const float fn = (float)n;
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) t->v[k][c] = p[3 * k + c] * fn;
    float a[3], b[3];
    for (int c = 0; c < 3; ++c) {
        a[c] = t->v[1][c] - t->v[0][c];
        b[c] = t->v[2][c] - t->v[0][c];
    }
    cross(a, b, t->n);
    t->w = (absf(t->n[0]) + absf(t->n[1])) + absf(t->n[2]);
    uint32_t flags = 0;
    float ux = t->n[0], uy = t->n[1], uz = t->n[2];
    normalize_unity(ux, uy, uz);
    if (ux == 0.0f && uy == 0.0f && uz == 0.0f) flags |= TRI_DEGENERATE;
    for (int c = 0; c < 3; ++c) {
        float mn = t->v[0][c], mx = t->v[0][c];
        for (int k = 1; k < 3; ++k) {
            mn = t->v[k][c] < mn ? t->v[k][c] : mn;
            mx = t->v[k][c] > mx ? t->v[k][c] : mx;
        }
        t->blo[c] = mn <= 0.0f ? 0 : mn > fn ? n : (int32_t)ceilf(mn) - 1;
        t->bhi[c] = mx < 0.0f ? -1 : mx >= fn ? n - 1 : (int32_t)floorf(mx);
        if (t->blo[c] > t->bhi[c]) flags |= TRI_OUTSIDE;
    }
    for (int q = 0; q < 3; ++q) {
        const int u = q, v = (q + 1) % 3;
        for (int e = 0; e < 3; ++e) {
            const int f = (e + 1) % 3, g = (e + 2) % 3;
            const float au = -(t->v[f][v] - t->v[e][v]);
            const float av = t->v[f][u] - t->v[e][u];
            const float tt = au * (t->v[g][u] - t->v[e][u]) + av * (t->v[g][v] - t->v[e][v]);
            t->a[q][e][0] = au;
            t->a[q][e][1] = av;
            t->lo[q][e] = tt < 0.0f ? tt : 0.0f;
            t->hiw[q][e] = (tt > 0.0f ? tt : 0.0f) + (absf(au) + absf(av));
        }
    }
    t->flags = flags;
}

// Candidates of a triangle: voxels of its clipped box with z in [z0, z1] (inclusive); 0 when skipped.
SVO_VOX_FN uint64_t candidates(const Tri &t, int z0, int z1) {
    if (t.flags) return 0;
    const int zl = t.blo[2] > z0 ? t.blo[2] : z0, zh = t.bhi[2] < z1 ? t.bhi[2] : z1;
    if (zl > zh) return 0;
    return (uint64_t)(t.bhi[0] - t.blo[0] + 1) * (uint64_t)(t.bhi[1] - t.blo[1] + 1) * (uint64_t)(zh - zl + 1);
}

// Candidate `local` of a box that is bx wide and by deep, counted x first, then y, then z:
//   out = (local mod bx, (local div bx) mod by, local div (bx by)),  the last one modulo 2^32.
// Two forms of the same integers: 32-bit divisions while local and the plane bx by both fit 32 bits (every
// triangle's box up to a 1024^3 grid, and most beyond), 64-bit ones otherwise.  The builder's overlap kernel
// adds the box's (and the slab's) lower corner; a candidate of the box has out[2] below the box's height.
SVO_VOX_FN void candidate_voxel_32(uint32_t local, uint32_t bx, uint32_t plane, uint32_t out[3]) {
    const uint32_t iz = local / plane;
    const uint32_t r = local - iz * plane;
    const uint32_t iy = r / bx;
    out[0] = r - iy * bx;
    out[1] = iy;
    out[2] = iz;
}

SVO_VOX_FN void candidate_voxel_64(uint64_t local, uint32_t bx, uint64_t plane, uint32_t out[3]) {
    const uint64_t iz = local / plane;
    const uint64_t r = local - iz * plane;
    const uint64_t iy = r / bx;
    out[0] = (uint32_t)(r - iy * bx);
    out[1] = (uint32_t)iy;
    out[2] = (uint32_t)iz;
}

SVO_VOX_FN void candidate_voxel(uint64_t local, uint32_t bx, uint32_t by, uint32_t out[3]) {
    const uint64_t plane = (uint64_t)bx * by;
    if (((local | plane) >> 32) == 0) candidate_voxel_32((uint32_t)local, bx, (uint32_t)plane, out);
    else candidate_voxel_64(local, bx, plane, out);
}

// Steps 2 and 3 for voxel i (inside the box) of a triangle that is not skipped.
SVO_VOX_FN bool overlaps(const Tri &t, const int i[3]) {
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) {
        lo[c] = (float)i[c];
        hi[c] = (float)(i[c] + 1);
    }
    const float s = ((t.n[0] * ((t.n[0] > 0.0f ? hi[0] : lo[0]) - t.v[0][0]) +
                      t.n[1] * ((t.n[1] > 0.0f ? hi[1] : lo[1]) - t.v[0][1])) +
                     t.n[2] * ((t.n[2] > 0.0f ? hi[2] : lo[2]) - t.v[0][2]));
    bool ok = s >= 0.0f && s <= t.w;
    for (int q = 0; q < 3; ++q) {
        const int u = q, v = (q + 1) % 3;
        for (int e = 0; e < 3; ++e) {
            const float au = t.a[q][e][0], av = t.a[q][e][1];
            const float p = au * ((au > 0.0f ? hi[u] : lo[u]) - t.v[e][u]) + av * ((av > 0.0f ? hi[v] : lo[v]) - t.v[e][v]);
            ok = ok && p >= t.lo[q][e] && p <= t.hiw[q][e];
        }
    }
    return ok;
}

SVO_VOX_FN bool in_box(const Tri &t, const int i[3]) {
    return i[0] >= t.blo[0] && i[0] <= t.bhi[0] && i[1] >= t.blo[1] && i[1] <= t.bhi[1] && i[2] >= t.blo[2] && i[2] <= t.bhi[2];
}

// The leaf normal of an owner.
SVO_VOX_FN void leaf_normal(const Tri &t, bool flip, float out[3]) {
    float x = t.n[0], y = t.n[1], z = t.n[2];
    normalize_unity(x, y, z);
    out[0] = flip ? -x : x;
    out[1] = flip ? -y : y;
    out[2] = flip ? -z : z;
}

// The leaf colour of voxel i from its owner and the owner's three vertex colours (rgb each).
SVO_VOX_FN void leaf_color(const Tri &t, const int i[3], const float c0[3], const float c1[3], const float c2[3], float out[3]) {
    float a[3], b[3], q[3], qb[3], aq[3];
    for (int c = 0; c < 3; ++c) {
        a[c] = t.v[1][c] - t.v[0][c];
        b[c] = t.v[2][c] - t.v[0][c];
        q[c] = ((float)i[c] + 0.5f) - t.v[0][c];
    }
    const float d = dot3(t.n, t.n);
    cross(q, b, qb);
    cross(a, q, aq);
    float w1 = dot3(qb, t.n) / d;
    float w2 = dot3(aq, t.n) / d;
    float w0 = (1.0f - w1) - w2;
    w0 = w0 > 0.0f ? w0 : 0.0f;
    w1 = w1 > 0.0f ? w1 : 0.0f;
    w2 = w2 > 0.0f ? w2 : 0.0f;
    const float s = (w0 + w1) + w2;
    w0 = w0 / s;
    w1 = w1 / s;
    w2 = w2 / s;
    for (int c = 0; c < 3; ++c) out[c] = (w0 * c0[c] + w1 * c1[c]) + w2 * c2[c];
}

}  // namespace svo_voxelize
