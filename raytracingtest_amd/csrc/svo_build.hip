// svo_build.hip -- native SVO builder (include/svo_build.h).
//
// Restates the reference's RT.CS.NaiveCreator (Assets/Scripts/SVO/CompactSVO/
// NaiveCreator.cs) for MI355X:
//   * leaf classification (BuildTree leaf branch :54-73 + IsEdge :121-130) on
//     the GPU: every leaf centre of the 2^d grid (plus a one-cell halo for the
//     IsEdge probes) is sampled once per z-slab into a byte grid, surface
//     leaves are appended as Morton codes, and their finite-difference normals
//     (:58-63) are evaluated in a second kernel;
//   * tree + layout + attachments (BuildTree internal branch :77-115,
//     CompressSVOAux :138-193, GetAttachment :195-257) on the host, as a
//     direct restatement of the reference recursion over a Morton-sorted tree.
// Samplers: SampleFunctions.cs:13-48; OpenSimplex 3D with seed 7
// (Noise/Simplex.cs:190-218, :268-324).  The 3D contribution lookup is
// generated from the published OpenSimplex region logic (Kurt Spencer, 2014)
// and checked against the reference table's digest (tests/golden).
// Arithmetic: C# float/double semantics, one IEEE rounding per operation
// (-ffp-contract=off, no fast-math).
// Limits of the GPU leaf pass (svob_limits, the _ex entry points; zero = default):
//   cell_bytes     budget of one slab's byte grid, 512 MiB.  A slab holds `rows` leaf planes
//                  plus a halo plane below and above: rows = clamp(cell_bytes / (n+2)^2 - 2,
//                  1, n) (slab_rows_of, exported as svob_slab_rows).  One slab up to
//                  max_level 10; 508 + 508 + 8 rows at max_level 11; one row from max_level
//                  15, where three planes no longer fit and the buffer exceeds the budget.
//   slab_rows      overrides the rule, clamped to [1, n].
//   list_capacity  first capacity of the surface list, max(1 Mi, 4 n^2) leaves.  A slab
//                  that counts more is classified again into a list of 1.25 x count + 1024
//                  (classify_kernel stores only while k < cap); the normal pass
//                  re-allocates when all leaves exceed the capacity.
//   max_blocks     cap on each launch's blocks, 65,536; the kernels' stride loops cover the rest.
//   launch_candidates  meshes only: candidates of one mesh_overlap_kernel launch, 2^28; a slab with more takes
//                  ceil(total / launch_candidates) launches (svob_report.overlap_launches sums them).
// None of them changes a result.  svob_report says which of these paths a call took.
// The mesh pass (svob_build_mesh, "meshes" below) reads the same fields for its owner grid of 4-byte
// cells without a halo: rows = clamp(cell_bytes / (4 n^2), 1, n), and a budget below one plane is refused.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svo_build.h"
#include "svo_voxelize.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &m) { g_err = m; return code; }
constexpr int SVOB_OK = 0, SVOB_ERR_ARG = -1, SVOB_ERR_HIP = -4, SVOB_ERR_MEM = -6;

#define HIPB(expr)                                                                          \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return fail(SVOB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// ------------------------------------------------------------------ OpenSimplex
constexpr double STRETCH_3D = -1.0 / 6.0;
constexpr double SQUISH_3D = 1.0 / 3.0;
constexpr double NORM_3D = 1.0 / 103.0;
constexpr int MAX_CONTRIB = 8;
constexpr int MAX_LISTS = 32;

struct ContribList {
    int count;
    int ox[MAX_CONTRIB], oy[MAX_CONTRIB], oz[MAX_CONTRIB];
    double dx[MAX_CONTRIB], dy[MAX_CONTRIB], dz[MAX_CONTRIB];
};

struct Simplex3 {
    uint8_t perm[256];
    uint8_t perm3D[256];
    int8_t list_of_hash[2048];   // -1: no entry (value 0)
    int nlists;
    ContribList lists[MAX_LISTS];
    double grad[72];
};

// Region logic of 3D OpenSimplex: lattice offsets of the two extra vertices.
// base 0: tetrahedron at (0,0,0); 1: tetrahedron at (1,1,1); 2: octahedron.
void region_contribs(double xins, double yins, double zins, int *base, int ext[2][3]) {
    const double inSum = xins + yins + zins;
    int x0, x1, y0, y1, z0, z1;
    if (inSum <= 1) {
        *base = 0;
        int aP = 1, bP = 2;
        double aS = xins, bS = yins;
        if (aS >= bS && zins > bS) { bS = zins; bP = 4; }
        else if (aS < bS && zins > aS) { aS = zins; aP = 4; }
        const double wins = 1 - inSum;
        if (wins > aS || wins > bS) {
            const int c = bS > aS ? bP : aP;
            if ((c & 1) == 0) { x0 = -1; x1 = 0; } else { x0 = x1 = 1; }
            if ((c & 2) == 0) { y0 = y1 = 0; if ((c & 1) == 0) y1 -= 1; else y0 -= 1; } else { y0 = y1 = 1; }
            if ((c & 4) == 0) { z0 = 0; z1 = -1; } else { z0 = z1 = 1; }
        } else {
            const int c = aP | bP;
            if ((c & 1) == 0) { x0 = 0; x1 = -1; } else { x0 = x1 = 1; }
            if ((c & 2) == 0) { y0 = 0; y1 = -1; } else { y0 = y1 = 1; }
            if ((c & 4) == 0) { z0 = 0; z1 = -1; } else { z0 = z1 = 1; }
        }
    } else if (inSum >= 2) {
        *base = 1;
        int aP = 6, bP = 5;
        double aS = xins, bS = yins;
        if (aS <= bS && zins < bS) { bS = zins; bP = 3; }
        else if (aS > bS && zins < aS) { aS = zins; aP = 3; }
        const double wins = 3 - inSum;
        if (wins < aS || wins < bS) {
            const int c = bS < aS ? bP : aP;
            if (c & 1) { x0 = 2; x1 = 1; } else { x0 = x1 = 0; }
            if (c & 2) { y0 = y1 = 1; if (c & 1) y1 += 1; else y0 += 1; } else { y0 = y1 = 0; }
            if (c & 4) { z0 = 1; z1 = 2; } else { z0 = z1 = 0; }
        } else {
            const int c = aP & bP;
            if (c & 1) { x0 = 1; x1 = 2; } else { x0 = x1 = 0; }
            if (c & 2) { y0 = 1; y1 = 2; } else { y0 = y1 = 0; }
            if (c & 4) { z0 = 1; z1 = 2; } else { z0 = z1 = 0; }
        }
    } else {
        *base = 2;
        double aS, bS;
        int aP, bP;
        bool aF, bF;
        const double p1 = xins + yins;
        if (p1 > 1) { aS = p1 - 1; aP = 3; aF = true; } else { aS = 1 - p1; aP = 4; aF = false; }
        const double p2 = xins + zins;
        if (p2 > 1) { bS = p2 - 1; bP = 5; bF = true; } else { bS = 1 - p2; bP = 2; bF = false; }
        const double p3 = yins + zins;
        if (p3 > 1) {
            const double s = p3 - 1;
            if (aS <= bS && aS < s) { aS = s; aP = 6; aF = true; }
            else if (aS > bS && bS < s) { bS = s; bP = 6; bF = true; }
        } else {
            const double s = 1 - p3;
            if (aS <= bS && aS < s) { aS = s; aP = 1; aF = false; }
            else if (aS > bS && bS < s) { bS = s; bP = 1; bF = false; }
        }
        auto perm110 = [](int c, int &x, int &y, int &z) {   // permutation of (1,1,-1) omitting c's axis
            if ((c & 1) == 0) { x = -1; y = 1; z = 1; } else if ((c & 2) == 0) { x = 1; y = -1; z = 1; } else { x = 1; y = 1; z = -1; }
        };
        auto perm002 = [](int c, int &x, int &y, int &z) {   // permutation of (0,0,2) on c's axis
            if (c & 1) { x = 2; y = 0; z = 0; } else if (c & 2) { x = 0; y = 2; z = 0; } else { x = 0; y = 0; z = 2; }
        };
        if (aF == bF) {
            if (aF) { x0 = y0 = z0 = 1; perm002(aP & bP, x1, y1, z1); }
            else { x0 = y0 = z0 = 0; perm110(aP | bP, x1, y1, z1); }
        } else {
            const int c1 = aF ? aP : bP, c2 = aF ? bP : aP;
            perm110(c1, x0, y0, z0);
            perm002(c2, x1, y1, z1);
        }
    }
    ext[0][0] = x0; ext[0][1] = y0; ext[0][2] = z0;
    ext[1][0] = x1; ext[1][1] = y1; ext[1][2] = z1;
}

__host__ __device__ inline int osn_hash(double xins, double yins, double zins) {
    const double inSum = xins + yins + zins;
    return (int)(yins - zins + 1) | (int)(xins - yins + 1) << 1 | (int)(xins - zins + 1) << 2 |
           (int)inSum << 3 | (int)(inSum + zins) << 5 | (int)(inSum + yins) << 7 | (int)(inSum + xins) << 9;
}

int init_simplex(Simplex3 *s, long long seed_in) {
    std::memset(s, 0, sizeof(*s));
    // Noise/Simplex.cs:190-218 permutation from the 64-bit LCG
    uint64_t seed = (uint64_t)seed_in;
    auto step = [](uint64_t v) { return v * 6364136223846793005ULL + 1442695040888963407ULL; };
    seed = step(step(step(seed)));
    uint8_t source[256];
    for (int i = 0; i < 256; ++i) source[i] = (uint8_t)i;
    for (int i = 255; i >= 0; --i) {
        seed = step(seed);
        const int64_t sv = (int64_t)(seed + 31ULL);
        int r = (int)(sv % (int64_t)(i + 1));
        if (r < 0) r += i + 1;
        s->perm[i] = source[r];
        s->perm3D[i] = (uint8_t)((s->perm[i] % 24) * 3);
        source[r] = source[i];
    }
    // gradient set: for sign pattern k, (+-11, +-4, +-4) and its two rotations
    for (int k = 0; k < 8; ++k) {
        const double sx = (k & 1) ? 1 : -1, sy = (k & 2) ? -1 : 1, sz = (k & 4) ? -1 : 1;
        const double g[9] = { sx * 11, sy * 4, sz * 4, sx * 4, sy * 11, sz * 4, sx * 4, sy * 4, sz * 11 };
        for (int j = 0; j < 9; ++j) s->grad[k * 9 + j] = g[j];
    }
    // contribution lists per hash, by sampling the region logic at interior points
    static const int base_sets[3][6][3] = {
        { {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1} },
        { {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1} },
        { {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1} } };
    static const int base_count[3] = { 4, 4, 6 };
    for (int h = 0; h < 2048; ++h) s->list_of_hash[h] = -1;
    uint64_t rng = 0x9E3779B97F4A7C15ULL;
    auto uni = [&rng]() {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        return (double)(rng >> 11) * (1.0 / 9007199254740992.0);
    };
    for (int it = 0; it < 600000; ++it) {
        const double xi = uni(), yi = uni(), zi = uni();
        const int h = osn_hash(xi, yi, zi);
        int base, ext[2][3];
        region_contribs(xi, yi, zi, &base, ext);
        ContribList cl{};
        cl.count = base_count[base] + 2;
        for (int j = 0; j < cl.count; ++j) {
            const int *o = j < base_count[base] ? base_sets[base][j] : ext[j - base_count[base]];
            cl.ox[j] = o[0]; cl.oy[j] = o[1]; cl.oz[j] = o[2];
            const double m = (double)(o[0] + o[1] + o[2]);   // Contribution3(multiplier = sum, ...)
            cl.dx[j] = (double)(-o[0]) - m * SQUISH_3D;
            cl.dy[j] = (double)(-o[1]) - m * SQUISH_3D;
            cl.dz[j] = (double)(-o[2]) - m * SQUISH_3D;
        }
        int found = -1;
        for (int l = 0; l < s->nlists; ++l) {
            const ContribList &o = s->lists[l];
            if (o.count != cl.count) continue;
            bool same = true;
            for (int j = 0; j < cl.count && same; ++j)
                same = o.ox[j] == cl.ox[j] && o.oy[j] == cl.oy[j] && o.oz[j] == cl.oz[j];
            if (same) { found = l; break; }
        }
        if (found < 0) {
            if (s->nlists >= MAX_LISTS) return fail(SVOB_ERR_ARG, "opensimplex: too many contribution lists");
            s->lists[s->nlists] = cl;
            found = s->nlists++;
        }
        if (s->list_of_hash[h] >= 0 && s->list_of_hash[h] != found)
            return fail(SVOB_ERR_ARG, "opensimplex: hash does not determine the region");
        s->list_of_hash[h] = (int8_t)found;
    }
    return SVOB_OK;
}

__host__ __device__ inline int fast_floor(double x) {
    const int xi = (int)x;
    return x < xi ? xi - 1 : xi;
}

// Noise/Simplex.cs:268-324
__host__ __device__ inline double simplex_eval(const Simplex3 &s, double x, double y, double z) {
    const double stretchOffset = (x + y + z) * STRETCH_3D;
    const double xs = x + stretchOffset, ys = y + stretchOffset, zs = z + stretchOffset;
    const int xsb = fast_floor(xs), ysb = fast_floor(ys), zsb = fast_floor(zs);
    const double squishOffset = (double)(xsb + ysb + zsb) * SQUISH_3D;
    const double dx0 = x - ((double)xsb + squishOffset);
    const double dy0 = y - ((double)ysb + squishOffset);
    const double dz0 = z - ((double)zsb + squishOffset);
    const double xins = xs - (double)xsb, yins = ys - (double)ysb, zins = zs - (double)zsb;
    const int h = osn_hash(xins, yins, zins);
    const int li = (h >= 0 && h < 2048) ? s.list_of_hash[h] : -1;
    double value = 0.0;
    if (li < 0) return value * NORM_3D;
    const ContribList &c = s.lists[li];
    for (int j = 0; j < c.count; ++j) {
        const double dx = dx0 + c.dx[j];
        const double dy = dy0 + c.dy[j];
        const double dz = dz0 + c.dz[j];
        double attn = 2 - dx * dx - dy * dy - dz * dz;
        if (attn > 0) {
            const int px = xsb + c.ox[j], py = ysb + c.oy[j], pz = zsb + c.oz[j];
            const int i = s.perm3D[(s.perm[(s.perm[px & 0xFF] + py) & 0xFF] + pz) & 0xFF];
            const double valuePart = s.grad[i] * dx + s.grad[i + 1] * dy + s.grad[i + 2] * dz;
            attn *= attn;
            value += attn * attn * valuePart;
        }
    }
    return value * NORM_3D;
}

// RotatedCuboid's rotation, Matrix4x4.Rotate(Quaternion.Euler(45, 45, 45)) (SampleFunctions.cs:54-58),
// restated in single precision (oracle/naive_creator.py unity_rotation_matrix derives the same
// nine words and tests/test_builder.py pins them): the half angle (45 * Mathf.Deg2Rad) / 2, its
// sine and cosine correctly rounded to float, q = (qY * qX) * qZ (Unity's Z, X, Y order,
// Quaternion operator*), then Matrix4x4.Rotate's products and sums.  Unity's own native
// arithmetic for Euler -> quaternion is not public: parity with it is unpinned.
#define ROT45_M00 0x1.b504f4p-1f
#define ROT45_M01 -0x1.2bec30p-3f
#define ROT45_M02 0x1.000000p-1f
#define ROT45_M10 0x1.000000p-1f
#define ROT45_M11 0x1.fffffcp-2f
#define ROT45_M12 -0x1.6a09eap-1f
#define ROT45_M20 -0x1.2bec30p-3f
#define ROT45_M21 0x1.b504f6p-1f
#define ROT45_M22 0x1.fffffcp-2f

// SampleFunctions.cs:54-68: Cuboid(R p, radius); Mathf.Max / Mathf.Min as a > b ? a : b,
// Vector3.Magnitude as a float sum of squares through a double square root
__host__ __device__ inline float rotated_cuboid(float x, float y, float z) {
    const float px = (x - 1.5f) * 2.0f, py = (y - 1.5f) * 2.0f, pz = (z - 1.5f) * 2.0f;
    const float rx = ROT45_M00 * px + ROT45_M01 * py + ROT45_M02 * pz;   // MultiplyVector
    const float ry = ROT45_M10 * px + ROT45_M11 * py + ROT45_M12 * pz;
    const float rz = ROT45_M20 * px + ROT45_M21 * py + ROT45_M22 * pz;
    const float radius = 0.6f;
    const float dx = fabsf(rx) - radius, dy = fabsf(ry) - radius, dz = fabsf(rz) - radius;
    const float myz = dy > dz ? dy : dz;
    const float m = dx > myz ? dx : myz;
    const float mag = (float)sqrt((double)(dx * dx + dy * dy + dz * dz));
    return m < mag ? m : mag;
}

// SampleFunctions.cs:20-47 (float in, float out; C# single-precision steps)
__host__ __device__ inline float sample(const Simplex3 &s, int type, float x, float y, float z) {
    switch (type) {
    case 0:   // FlatGround (its Debug.LogFormat is dropped)
        return 0.5f - y;
    case 1: { // Sphere(p - 0.5, r = 0.25)
        const float px = x - 0.5f, py = y - 0.5f, pz = z - 0.5f;
        return px * px + py * py + pz * pz - 0.25f * 0.25f;
    }
    case 2: { // Simplex, r = 1132
        const float r = 1132.0f;
        return (float)simplex_eval(s, (double)(x * r), (double)(y * r), (double)(z * r));
    }
    case 3:   // RotatedCuboid, radius 0.6 (SampleFunctions.cs:35-38)
        return rotated_cuboid(x, y, z);
    default: { // 4: Custom1 simplex terrain
        float result = y - 1.5f;
        const float r = 3.0f;
        const float r2 = r * 8;
        result += 0.5f * (float)simplex_eval(s, (double)(x * r), (double)(y * r), (double)(z * r));
        result += 0.15f * (float)simplex_eval(s, (double)(x * r2), (double)(y * r2), (double)(z * r2));
        return result;
    }
    }
}

// ---------------------------------------------------------------- GPU kernels
// cell byte: bit0 = solid (s <= 0), bit1 = air (s > 0)
__global__ void sign_kernel(const Simplex3 *__restrict__ s, int type, int n, float size, int z_cell0, int z_cells,
                            uint8_t *__restrict__ cells) {
    const int np2 = n + 2;
    const size_t total = (size_t)np2 * np2 * z_cells;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cx = (int)(i % np2);
        const int cy = (int)((i / np2) % np2);
        const int cz = z_cell0 + (int)(i / ((size_t)np2 * np2));
        // centre of leaf (c - 1): 1 + (c - 0.5) * size, exact dyadic
        const float px = 1.0f + ((float)cx - 0.5f) * size;
        const float py = 1.0f + ((float)cy - 0.5f) * size;
        const float pz = 1.0f + ((float)cz - 0.5f) * size;
        const float v = sample(*s, type, px, py, pz);
        cells[i] = (uint8_t)((v <= 0.0f ? 1 : 0) | (v > 0.0f ? 2 : 0));
    }
}

__device__ inline uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x1F00000000FFFFULL;
    x = (x | (x << 16)) & 0x1F0000FF0000FFULL;
    x = (x | (x << 8)) & 0x100F00F00F00F00FULL;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ULL;
    x = (x | (x << 2)) & 0x1249249249249249ULL;
    return x;
}

__device__ inline uint32_t compact3(uint64_t x) {
    x &= 0x1249249249249249ULL;
    x = (x ^ (x >> 2)) & 0x10C30C30C30C30C3ULL;
    x = (x ^ (x >> 4)) & 0x100F00F00F00F00FULL;
    x = (x ^ (x >> 8)) & 0x1F0000FF0000FFULL;
    x = (x ^ (x >> 16)) & 0x1F00000000FFFFULL;
    x = (x ^ (x >> 32)) & 0x1FFFFFULL;
    return (uint32_t)x;
}

// IsEdge: solid leaf with an air 6-neighbour (NaiveCreator.cs:56,121-130)
__global__ void classify_kernel(const uint8_t *__restrict__ cells, int n, int z0, int zc, uint64_t *__restrict__ out,
                                unsigned long long *__restrict__ counter, unsigned long long cap) {
    const int np2 = n + 2;
    const size_t plane = (size_t)np2 * np2;
    const size_t total = (size_t)n * n * zc;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % n);
        const int y = (int)((i / n) % n);
        const int zl = (int)(i / ((size_t)n * n));
        // slab cell buffer starts at padded z = z0 (leaf z0 - 1)
        const size_t c = (size_t)(zl + 1) * plane + (size_t)(y + 1) * np2 + (size_t)(x + 1);
        if (!(cells[c] & 1)) continue;
        const bool edge = (cells[c + 1] & 2) || (cells[c - 1] & 2) || (cells[c + np2] & 2) ||
                          (cells[c - np2] & 2) || (cells[c + plane] & 2) || (cells[c - plane] & 2);
        if (!edge) continue;
        const unsigned long long k = atomicAdd(counter, 1ULL);
        if (k < cap) {
            const uint32_t z = (uint32_t)(z0 + zl);
            out[k] = spread3((uint32_t)x) | (spread3((uint32_t)y) << 1) | (spread3(z) << 2);
        }
    }
}

__host__ __device__ inline void normalize_unity(float &x, float &y, float &z) {
    const float mag = (float)sqrt((double)(x * x + y * y + z * z));
    if (mag > 1e-5f) { x = x / mag; y = y / mag; z = z / mag; }
    else { x = 0.0f; y = 0.0f; z = 0.0f; }
}

// finite-difference normal, normal = -Normalize(n) (NaiveCreator.cs:58-63)
__global__ void normal_kernel(const Simplex3 *__restrict__ s, int type, float size, const uint64_t *__restrict__ codes,
                              size_t count, float *__restrict__ normals) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t code = codes[i];
        const float half = size / 2;
        const float px = (1.0f + (float)compact3(code) * size) + half;
        const float py = (1.0f + (float)compact3(code >> 1) * size) + half;
        const float pz = (1.0f + (float)compact3(code >> 2) * size) + half;
        const float h = 0.001f;
        float nx = sample(*s, type, px - h, py, pz) - sample(*s, type, px, py, pz);
        float ny = sample(*s, type, px, py - h, pz) - sample(*s, type, px, py, pz);
        float nz = sample(*s, type, px, py, pz - h) - sample(*s, type, px, py, pz);
        normalize_unity(nx, ny, nz);
        normals[3 * i + 0] = -nx;
        normals[3 * i + 1] = -ny;
        normals[3 * i + 2] = -nz;
    }
}

// ------------------------------------------------------------------ host layout
inline uint64_t spread3_h(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x1F00000000FFFFULL;
    x = (x | (x << 16)) & 0x1F0000FF0000FFULL;
    x = (x | (x << 8)) & 0x100F00F00F00F00FULL;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ULL;
    x = (x | (x << 2)) & 0x1249249249249249ULL;
    return x;
}
inline uint32_t compact3_h(uint64_t x) {
    x &= 0x1249249249249249ULL;
    x = (x ^ (x >> 2)) & 0x10C30C30C30C30C3ULL;
    x = (x ^ (x >> 4)) & 0x100F00F00F00F00FULL;
    x = (x ^ (x >> 8)) & 0x1F0000FF0000FFULL;
    x = (x ^ (x >> 16)) & 0x1F00000000FFFFULL;
    x = (x ^ (x >> 32)) & 0x1FFFFFULL;
    return (uint32_t)x;
}

struct V3 { float x, y, z; };

inline float dist3(const V3 &a, const V3 &b) {   // Vector3.Distance
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (float)std::sqrt((double)(dx * dx + dy * dy + dz * dz));
}

inline int to_int_cs(float f) {   // C# (int)float: truncation, NaN/overflow -> int.MinValue
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
    return (int)f;
}

inline int compress_color(const V3 &c) {   // NaiveCreator.cs:351-356
    int color = to_int_cs(32.0f * (c.x - 0.00001f));
    color |= to_int_cs(64.0f * (c.y - 0.00001f)) << 5;
    color |= to_int_cs(32.0f * (c.z - 0.00001f)) << 11;
    return color;
}

inline float clampf_cs(float v, float lo, float hi) {   // Mathf.Clamp keeps NaN
    if (v < lo) v = lo; else if (v > hi) v = hi;
    return v;
}

inline uint32_t encode_normal16(const V3 &n) {   // NaiveCreator.cs:547-571
    const float ax = std::fabs(n.x), ay = std::fabs(n.y), az = std::fabs(n.z);
    const int axis = (ax >= std::max(ay, az)) ? 0 : (ay >= az) ? 1 : 2;
    V3 tuv;
    if (axis == 0) tuv = n;
    else if (axis == 1) tuv = { n.y, n.z, n.x };
    else tuv = { n.z, n.x, n.y };
    const uint32_t sign = tuv.x >= 0.0f ? 0u : 0x8000u;
    const uint32_t ab = (uint32_t)axis << 13;
    const float at = std::fabs(tuv.x);
    const uint32_t u = (uint32_t)((to_int_cs(clampf_cs((tuv.y / at) * 63.0f, -64.0f, 63.0f)) & 0x7F) << 6) & 0xFFFFu;
    const uint32_t v = (uint32_t)(to_int_cs(clampf_cs((tuv.z / at) * 31.0f, -32.0f, 31.0f)) & 0x3F);
    return (sign | ab | u | v) & 0xFFFFu;
}

// GetAttachment (NaiveCreator.cs:195-257)
inline void get_attachment(const bool present[8], const V3 color[8], const V3 &normal, uint32_t &w0, uint32_t &w1) {
    V3 A = { 0, 0, 0 }, B = { 0, 0, 0 };
    int numChildren = 0;
    const float bdist = 0.0f;
    for (int i = 0; i < 8; ++i) {
        if (!present[i]) continue;
        ++numChildren;
        if (numChildren == 1) A = color[i];
        else if (dist3(A, color[i]) > bdist) B = color[i];
    }
    const int ia = compress_color(A), ib = compress_color(B);
    const uint32_t inormal = encode_normal16(normal);
    V3 cand[4] = { A, B,
                   { 0.667f * A.x + 0.333f * B.x, 0.667f * A.y + 0.333f * B.y, 0.667f * A.z + 0.333f * B.z },
                   { 0.333f * A.x + 0.667f * B.x, 0.333f * A.y + 0.667f * B.y, 0.333f * A.z + 0.667f * B.z } };
    uint32_t choices = 0;
    for (int i = 0; i < 8; ++i) {
        if (!present[i]) continue;
        float best = 100.0f;
        int choice = 0;
        for (int j = 0; j < 4; ++j) {
            const float d = dist3(color[i], cand[j]);
            if (d < best) { best = d; choice = j; }
        }
        choices |= (uint32_t)choice << (i * 2);
    }
    const uint64_t att = (uint64_t)(uint32_t)ia | ((uint64_t)(uint32_t)ib << 16) | ((uint64_t)choices << 32) |
                         ((uint64_t)inormal << 48);
    w0 = (uint32_t)att;
    w1 = (uint32_t)(att >> 32);
}

struct Level {
    std::vector<uint64_t> key;
    std::vector<uint32_t> child_begin;   // into level k+1 (size = nodes + 1)
    std::vector<V3> normal, color;
};

struct Layout {
    int depth;
    std::vector<Level> lv;
    std::vector<uint64_t> nodes;
    std::vector<uint32_t> att;
    uint64_t count = 1;
    bool v1_ok = true;
};

void compress_aux(Layout &L, int k, uint32_t j, uint64_t nodeIndex) {   // CompressSVOAux
    const Level &cur = L.lv[k];
    const Level &kid = L.lv[k + 1];
    const bool kids_internal = (k + 1) < L.depth;
    const uint32_t b = cur.child_begin[j], e = cur.child_begin[j + 1];
    uint64_t childPointer = 0;
    uint32_t valid = 0;
    bool present[8] = { false };
    V3 colors[8] = {};
    for (uint32_t c = b; c < e; ++c) {
        const int slot = (int)(kid.key[c] & 7u);
        valid |= 1u << slot;
        present[slot] = true;
        colors[slot] = kid.color[c];
        if (kids_internal) {
            if (childPointer == 0) childPointer = L.count - nodeIndex;
            L.count++;
        }
    }
    if (kids_internal) {
        uint64_t cp = childPointer;
        for (uint32_t c = b; c < e; ++c) compress_aux(L, k + 1, c, nodeIndex + cp++);
    }
    const uint32_t nonleaf = kids_internal ? valid : 0u;
    if (childPointer > 0xFFFFu) L.v1_ok = false;
    const uint64_t first = nonleaf ? nodeIndex + childPointer : 0;
    L.nodes[nodeIndex] = (first << 32) | (uint64_t)((valid << 8) | nonleaf);
    get_attachment(present, colors, cur.normal[j], L.att[2 * nodeIndex], L.att[2 * nodeIndex + 1]);
}

int layout_from_sorted(int depth, std::vector<uint64_t> &codes, std::vector<V3> &normals, std::vector<V3> &colors,
                       svob_result *out) {
    Layout L;
    L.depth = depth;
    L.lv.resize(depth + 1);
    L.lv[depth].key = std::move(codes);
    L.lv[depth].normal = std::move(normals);
    L.lv[depth].color = std::move(colors);
    size_t total = 0;
    for (int k = depth - 1; k >= 0; --k) {   // BuildTree internal branch, bottom-up
        Level &cur = L.lv[k];
        const Level &kid = L.lv[k + 1];
        const size_t m = kid.key.size();
        for (size_t c = 0; c < m; ++c) {
            const uint64_t pk = kid.key[c] >> 3;
            if (cur.key.empty() || cur.key.back() != pk) {
                cur.key.push_back(pk);
                cur.child_begin.push_back((uint32_t)c);
            }
        }
        cur.child_begin.push_back((uint32_t)m);
        const size_t nn = cur.key.size();
        cur.normal.resize(nn);
        cur.color.resize(nn);
        for (size_t j = 0; j < nn; ++j) {
            V3 nsum = { 0, 0, 0 };
            float cx = 0.0f;
            int numChildren = 0;
            for (uint32_t c = cur.child_begin[j]; c < cur.child_begin[j + 1]; ++c) {
                ++numChildren;
                cx += kid.color[c].x;   // color.x += child.color.r (only r, NaiveCreator.cs:105)
                nsum.x = nsum.x + kid.normal[c].x;
                nsum.y = nsum.y + kid.normal[c].y;
                nsum.z = nsum.z + kid.normal[c].z;
            }
            const float inv = 1.0f / (float)numChildren;
            cur.color[j] = { cx * inv, 0.0f * inv, 0.0f * inv };
            normalize_unity(nsum.x, nsum.y, nsum.z);
            cur.normal[j] = nsum;
        }
        total += nn;
    }
    if (L.lv[0].key.size() != 1) return fail(SVOB_ERR_ARG, "internal: root level must hold one node");
    L.nodes.assign(total, 0);
    L.att.assign(2 * total, 0);
    compress_aux(L, 0, 0, 0);
    if (L.count != total) return fail(SVOB_ERR_ARG, "internal: layout count mismatch");

    out->n_nodes = total;
    out->depth = depth;
    out->v1_ok = L.v1_ok ? 1 : 0;
    out->n_leaves = L.lv[depth].key.size();
    out->nodes = (uint64_t *)std::malloc(total * sizeof(uint64_t));
    out->attachments = (uint32_t *)std::malloc(2 * total * sizeof(uint32_t));
    out->descriptors = (int32_t *)std::malloc(total * sizeof(int32_t));
    if (!out->nodes || !out->attachments || !out->descriptors) return fail(SVOB_ERR_MEM, "out of host memory");
    std::memcpy(out->nodes, L.nodes.data(), total * sizeof(uint64_t));
    std::memcpy(out->attachments, L.att.data(), 2 * total * sizeof(uint32_t));
    for (size_t i = 0; i < total; ++i) {
        const uint64_t nd = L.nodes[i];
        const uint32_t lo = (uint32_t)nd;
        const uint64_t first = nd >> 32;
        const uint32_t rel = (lo & 0xFFu) ? (uint32_t)(first - i) : 0u;
        out->descriptors[i] = (int32_t)((rel << 16) | lo);   // wraps exactly like C# when !v1_ok
    }
    return SVOB_OK;
}

// ------------------------------------------------------------------ limits
struct Limits {
    uint64_t cell_bytes = 512ull << 20;
    uint64_t list_capacity = 0;   // 0: max(1 Mi, 4 n^2)
    int32_t slab_rows = 0;        // 0: from cell_bytes
    int32_t max_blocks = 65536;
    uint64_t launch_candidates = 1ull << 28;   // meshes: candidates per mesh_overlap_kernel launch
};

int read_limits(const svob_limits *in, Limits *out) {
    *out = Limits();
    if (!in) return SVOB_OK;
    if (in->size < 2 * sizeof(uint32_t)) return fail(SVOB_ERR_ARG, "svob_limits.size must hold at least size and reserved");
    if (in->size > sizeof(svob_limits))
        return fail(SVOB_ERR_ARG, "svob_limits.size " + std::to_string(in->size) + " is larger than this library's (" +
                                      std::to_string(sizeof(svob_limits)) + "): a newer ABI");
    svob_limits k;
    std::memset(&k, 0, sizeof k);   // fields past the caller's size: default
    std::memcpy(&k, in, in->size);
    if (k.slab_rows < 0) return fail(SVOB_ERR_ARG, "svob_limits.slab_rows must not be negative");
    if (k.max_blocks < 0) return fail(SVOB_ERR_ARG, "svob_limits.max_blocks must not be negative");
    if (k.list_capacity > SIZE_MAX / sizeof(uint64_t)) return fail(SVOB_ERR_ARG, "svob_limits.list_capacity is too large");
    if (k.cell_bytes) out->cell_bytes = k.cell_bytes;
    out->list_capacity = k.list_capacity;
    out->slab_rows = k.slab_rows;
    if (k.max_blocks) out->max_blocks = k.max_blocks;
    if (k.launch_candidates) out->launch_candidates = k.launch_candidates;
    return SVOB_OK;
}

// Leaf planes per z-slab: the byte grid holds rows + 2 planes of (n + 2)^2 cells (one halo
// plane below, one above).  rows = clamp(cell_bytes / (n + 2)^2 - 2, 1, n); a budget of fewer
// than three planes gives 1, and the buffer then exceeds the budget.  No subtraction below
// three planes: the quotient is unsigned.
int slab_rows_of(int n, const Limits &lim) {
    if (lim.slab_rows > 0) return std::min(lim.slab_rows, n);
    const uint64_t plane = ((uint64_t)n + 2) * ((uint64_t)n + 2);   // n <= 2^21: below 2^43
    const uint64_t planes = lim.cell_bytes / plane;
    if (planes < 3) return 1;
    return (int)std::min<uint64_t>((uint64_t)n, planes - 2);
}

unsigned blocks_for(size_t items, const Limits &lim) {
    return (unsigned)std::min<size_t>((items + 255) / 256, (size_t)lim.max_blocks);
}

int surface_leaves_gpu(int device, int type, int max_level, const Limits &lim, svob_report *rep,
                       std::vector<uint64_t> &codes, std::vector<V3> &normals) {
    const int depth = max_level - 1;
    const int n = 1 << depth;
    const float size = std::ldexp(1.0f, -depth);
    Simplex3 hs;
    int rc = init_simplex(&hs, 7);   // SampleFunctions.cs:18 new OpenSimplexNoise(7)
    if (rc) return rc;
    HIPB(hipSetDevice(device));
    Simplex3 *ds = nullptr;
    uint8_t *cells = nullptr;
    uint64_t *dcodes = nullptr;
    unsigned long long *dcount = nullptr;
    auto cleanup = [&]() {
        if (ds) (void)hipFree(ds);
        if (cells) (void)hipFree(cells);
        if (dcodes) (void)hipFree(dcodes);
        if (dcount) (void)hipFree(dcount);
    };
    const size_t np2 = (size_t)n + 2;
    const int slab = slab_rows_of(n, lim);
    size_t cap = lim.list_capacity ? (size_t)lim.list_capacity : std::max<size_t>(1 << 20, (size_t)n * n * 4);
    uint32_t n_slabs = 0, n_relaunch = 0, regrown = 0;
    hipError_t e = hipMalloc(&ds, sizeof(Simplex3));
    if (e == hipSuccess) e = hipMemcpy(ds, &hs, sizeof(Simplex3), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&cells, np2 * np2 * (size_t)(slab + 2));
    if (e == hipSuccess) e = hipMalloc(&dcodes, cap * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&dcount, sizeof(unsigned long long));
    if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("builder alloc: ") + hipGetErrorString(e)); }
    codes.clear();
    for (int z0 = 0; z0 < n; z0 += slab) {
        const int zc = std::min(slab, n - z0);
        const int zcells = zc + 2;
        const size_t ncell = np2 * np2 * (size_t)zcells;
        const unsigned grid = blocks_for(ncell, lim);
        ++n_slabs;
        hipLaunchKernelGGL(sign_kernel, dim3(grid), dim3(256), 0, 0, ds, type, n, size, z0, zcells, cells);
        e = hipGetLastError();
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("builder sign launch: ") + hipGetErrorString(e)); }
        for (;;) {
            e = hipMemset(dcount, 0, sizeof(unsigned long long));
            if (e != hipSuccess) break;
            const size_t nl = (size_t)n * n * zc;
            const unsigned g2 = blocks_for(nl, lim);
            hipLaunchKernelGGL(classify_kernel, dim3(g2), dim3(256), 0, 0, cells, n, z0, zc, dcodes, dcount,
                               (unsigned long long)cap);
            e = hipGetLastError();
            if (e != hipSuccess) break;
            unsigned long long cnt = 0;
            e = hipMemcpy(&cnt, dcount, sizeof(cnt), hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            if (cnt <= cap) {
                const size_t old = codes.size();
                codes.resize(old + cnt);
                e = hipMemcpy(codes.data() + old, dcodes, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost);
                break;
            }
            // the kernel stored only the first cap codes (k < cap): grow the list and classify again
            (void)hipFree(dcodes);
            dcodes = nullptr;
            cap = (size_t)(cnt * 1.25) + 1024;
            ++n_relaunch;
            e = hipMalloc(&dcodes, cap * sizeof(uint64_t));
            if (e != hipSuccess) break;
        }
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("builder classify: ") + hipGetErrorString(e)); }
    }
    std::sort(codes.begin(), codes.end());
    const size_t cap_classified = cap;
    // normals of the sorted leaves
    normals.resize(codes.size());
    if (!codes.empty()) {
        float *dn = nullptr;
        if (codes.size() > cap) {
            (void)hipFree(dcodes);
            dcodes = nullptr;
            e = hipMalloc(&dcodes, codes.size() * sizeof(uint64_t));
            regrown = 1;
        }
        if (e == hipSuccess) e = hipMemcpy(dcodes, codes.data(), codes.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&dn, codes.size() * 3 * sizeof(float));
        if (e == hipSuccess) {
            const unsigned g3 = blocks_for(codes.size(), lim);
            hipLaunchKernelGGL(normal_kernel, dim3(g3), dim3(256), 0, 0, ds, type, size, dcodes, codes.size(), dn);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(normals.data(), dn, codes.size() * 3 * sizeof(float), hipMemcpyDeviceToHost);
        if (dn) (void)hipFree(dn);
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("builder normals: ") + hipGetErrorString(e)); }
    }
    cleanup();
    if (rep) {   // rep->size was checked by the entry point
        svob_report k;
        std::memset(&k, 0, sizeof k);
        k.slabs = n_slabs;
        k.slab_rows = (uint32_t)slab;
        k.relaunches = n_relaunch;
        k.normals_regrown = regrown;
        k.list_capacity = cap_classified;
        const size_t nb = std::min<size_t>(rep->size, sizeof k);
        k.size = (uint32_t)nb;
        std::memcpy(rep, &k, nb);
    }
    return SVOB_OK;
}

// ------------------------------------------------------------------ meshes
// svob_build_mesh / svob_mesh_leaves: triangles -> surface leaves by the rule of svo_voxelize.h.
//   mesh_setup_kernel    once per build, one lane per triangle: the rule's constants, the clipped box, the flags.
//   per z-slab of `rows` planes (an owner grid of rows x n x n uint32, all NO_OWNER):
//     mesh_count_kernel    candidates of every triangle's box in the slab; an exclusive scan over them
//     mesh_overlap_kernel  one lane per CANDIDATE VOXEL: candidate g belongs to the triangle t with
//                          scan[t] <= g < scan[t + 1], found by a search over the whole scan for the wave's first
//                          and last candidate (wave-uniform) and refined per lane between the two; the rule, and
//                          atomicMin(cell, t) on a hit.  At most svob_limits.launch_candidates (2^28) per launch;
//                          svob_report.overlap_launches counts the launches.
//     mesh_compact_kernel  occupied cells -> (morton, owner) through classify_kernel's counter / capacity protocol
//   host: sort by code (codes are unique); mesh_attr_kernel: normal and colour of every sorted leaf from its owner.
using svo_voxelize::Tri;

struct Mesh {   // svob_mesh after read_mesh
    uint32_t flags = 0;
    const float *positions = nullptr;
    size_t n_vertices = 0;
    const uint32_t *indices = nullptr;
    size_t n_triangles = 0;
    const float *colors = nullptr;
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // lane 0 holds the sum
}

__global__ void mesh_setup_kernel(const float *__restrict__ pos, const uint32_t *__restrict__ idx, uint32_t n_tri, int n,
                                  Tri *__restrict__ tris, unsigned long long *__restrict__ stats) {
    unsigned long long degenerate = 0, outside = 0, cand = 0;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tri; t += (size_t)gridDim.x * blockDim.x) {
        float p[9];
        for (int k = 0; k < 3; ++k) {
            const size_t v = idx[3 * t + k];
            p[3 * k] = pos[3 * v];
            p[3 * k + 1] = pos[3 * v + 1];
            p[3 * k + 2] = pos[3 * v + 2];
        }
        Tri *tri = &tris[t];
        svo_voxelize::setup(p, n, tri);
        const uint32_t f = tri->flags;
        if (f & svo_voxelize::TRI_DEGENERATE) ++degenerate;
        else if (f & svo_voxelize::TRI_OUTSIDE) ++outside;
        cand += svo_voxelize::candidates(*tri, 0, n - 1);
    }
    degenerate = wave_sum(degenerate);
    outside = wave_sum(outside);
    cand = wave_sum(cand);
    if ((threadIdx.x & 63u) == 0) {
        if (degenerate) atomicAdd(&stats[0], degenerate);
        if (outside) atomicAdd(&stats[1], outside);
        if (cand) atomicAdd(&stats[2], cand);
    }
}

// counts[t] = candidates of triangle t in planes [z0, z1]; counts[n_tri] = 0 (the scan's total lands there)
__global__ void mesh_count_kernel(const Tri *__restrict__ tris, uint32_t n_tri, int z0, int z1,
                                  unsigned long long *__restrict__ counts) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tri; t += (size_t)gridDim.x * blockDim.x)
        counts[t] = t < n_tri ? svo_voxelize::candidates(tris[t], z0, z1) : 0ull;
}

// Exclusive scan of counts[0 .. len) in place by ONE block of 256 threads: tiles of 256 with a running carry.
// len = triangles + 1; 1,281 tiles for the 327,680 triangles of a seven-fold icosphere.
constexpr int MESH_SCAN_ITEMS = 8;   // consecutive items per thread: tiles of 2,048
__global__ void __launch_bounds__(256) mesh_scan_kernel(unsigned long long *__restrict__ counts, size_t len) {
    __shared__ unsigned long long wave_total[4];
    __shared__ unsigned long long carry_s;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (size_t base = 0; base < len; base += 256 * MESH_SCAN_ITEMS) {
        const size_t i0 = base + (size_t)threadIdx.x * MESH_SCAN_ITEMS;
        unsigned long long item[MESH_SCAN_ITEMS];
        unsigned long long own = 0;   // the thread's items, then the exclusive scan inside the thread
        for (int k = 0; k < MESH_SCAN_ITEMS; ++k) {
            const unsigned long long c = i0 + k < len ? counts[i0 + k] : 0ull;
            item[k] = own;
            own += c;
        }
        unsigned long long v = own;   // inclusive scan of the threads' sums inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(v, o, 64);
            if (lane >= (unsigned)o) v += up;
        }
        if (lane == 63) wave_total[wave] = v;
        __syncthreads();
        unsigned long long before = carry_s;
        for (unsigned w = 0; w < wave; ++w) before += wave_total[w];
        for (int k = 0; k < MESH_SCAN_ITEMS; ++k)
            if (i0 + k < len) counts[i0 + k] = before + (v - own) + item[k];
        __syncthreads();
        if (threadIdx.x == 255) carry_s = before + v;
        __syncthreads();
    }
}

__device__ inline uint64_t uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// the largest t in [lo, hi] with scan[t] <= g (scan[lo] <= g is given)
__device__ inline uint32_t scan_find(const unsigned long long *__restrict__ scan, uint32_t lo, uint32_t hi, uint64_t g) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (scan[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Candidates [c_begin, c_end) of the slab [z0, z1], one per lane.  scan: the exclusive scan of the slab's counts.
__global__ void __launch_bounds__(256) mesh_overlap_kernel(const Tri *__restrict__ tris,
                                                           const unsigned long long *__restrict__ scan, uint32_t n_tri, int n,
                                                           int z0, int z1, uint64_t c_begin, uint64_t c_end,
                                                           uint32_t *__restrict__ grid, unsigned long long *__restrict__ hits) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    const unsigned lane = threadIdx.x & 63u;
    unsigned long long wave_hits = 0;
    for (uint64_t wb = uniform64(c_begin + (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u)); wb < c_end; wb += stride) {
        const uint64_t last = wb + 63 < c_end ? wb + 63 : c_end - 1;
        const uint32_t t_first = scan_find(scan, 0, n_tri - 1, wb);         // wave-uniform
        const uint32_t t_last = scan_find(scan, t_first, n_tri - 1, last);   // wave-uniform
        const uint64_t g = wb + lane;
        bool hit = false;
        if (g <= last) {
            const uint32_t ti = scan_find(scan, t_first, t_last, g);
            const Tri &t = tris[ti];
            const uint64_t local = g - scan[ti];
            const uint32_t bx = (uint32_t)(t.bhi[0] - t.blo[0] + 1), by = (uint32_t)(t.bhi[1] - t.blo[1] + 1);
            uint32_t at[3];
            svo_voxelize::candidate_voxel(local, bx, by, at);
            const int zl = t.blo[2] > z0 ? t.blo[2] : z0;
            const int i[3] = { t.blo[0] + (int)at[0], t.blo[1] + (int)at[1], zl + (int)at[2] };
            // inside the box and the slab by construction; the compare keeps a store inside the grid whatever the scan holds
            hit = i[0] <= t.bhi[0] && i[1] <= t.bhi[1] && i[2] <= t.bhi[2] && i[2] <= z1 && svo_voxelize::overlaps(t, i);
            if (hit) atomicMin(&grid[((size_t)(i[2] - z0) * n + (size_t)i[1]) * n + (size_t)i[0]], ti);
        }
        wave_hits += (unsigned long long)__popcll(__ballot(hit));
    }
    if (lane == 0 && wave_hits) atomicAdd(hits, wave_hits);
}

__global__ void __launch_bounds__(256) mesh_compact_kernel(const uint32_t *__restrict__ grid, int n, int z0, int zc,
                                                           uint64_t *__restrict__ codes, uint32_t *__restrict__ owners,
                                                           unsigned long long *__restrict__ counter, unsigned long long cap) {
    // A block takes tiles of 1,024 cells (four per thread, a wave reads 256 contiguous bytes at a time), counts
    // its occupied cells in LDS and reserves their list slots with ONE add on the global counter (Guideline 12):
    // the counter still ends at the slab's count whatever the capacity, as the relaunch protocol needs.
    constexpr int CELLS = 4;
    __shared__ unsigned tile_count;
    __shared__ unsigned long long tile_base;
    const size_t total = (size_t)n * n * zc;
    for (size_t base = (size_t)blockIdx.x * (256 * CELLS); base < total; base += (size_t)gridDim.x * (256 * CELLS)) {
        if (threadIdx.x == 0) tile_count = 0;
        __syncthreads();
        uint32_t o[CELLS];
        unsigned slot[CELLS];
        for (int c = 0; c < CELLS; ++c) {
            const size_t i = base + (size_t)c * 256 + threadIdx.x;
            o[c] = i < total ? grid[i] : svo_voxelize::NO_OWNER;
            slot[c] = o[c] != svo_voxelize::NO_OWNER ? atomicAdd(&tile_count, 1u) : 0u;
        }
        __syncthreads();
        if (threadIdx.x == 0 && tile_count) tile_base = atomicAdd(counter, (unsigned long long)tile_count);
        __syncthreads();
        for (int c = 0; c < CELLS; ++c) {
            if (o[c] == svo_voxelize::NO_OWNER) continue;
            const unsigned long long k = tile_base + slot[c];
            if (k < cap) {
                const size_t i = base + (size_t)c * 256 + threadIdx.x;
                const uint32_t x = (uint32_t)(i % n), y = (uint32_t)((i / n) % n);
                const uint32_t z = (uint32_t)z0 + (uint32_t)(i / ((size_t)n * n));
                codes[k] = spread3(x) | (spread3(y) << 1) | (spread3(z) << 2);
                owners[k] = o[c];
            }
        }
    }
}

__global__ void mesh_attr_kernel(const Tri *__restrict__ tris, const uint32_t *__restrict__ idx, const float *__restrict__ col,
                                 const uint64_t *__restrict__ codes, const uint32_t *__restrict__ owners, size_t count,
                                 uint32_t flip, float *__restrict__ normals, float *__restrict__ colors) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t o = owners[i];
        const Tri &t = tris[o];
        float nrm[3];
        svo_voxelize::leaf_normal(t, flip != 0, nrm);
        normals[3 * i] = nrm[0];
        normals[3 * i + 1] = nrm[1];
        normals[3 * i + 2] = nrm[2];
        if (col) {
            const uint64_t code = codes[i];
            const int v[3] = { (int)compact3(code), (int)compact3(code >> 1), (int)compact3(code >> 2) };
            const size_t i0 = idx[3 * (size_t)o], i1 = idx[3 * (size_t)o + 1], i2 = idx[3 * (size_t)o + 2];
            float c[3];
            svo_voxelize::leaf_color(t, v, col + 3 * i0, col + 3 * i1, col + 3 * i2, c);
            colors[3 * i] = c[0];
            colors[3 * i + 1] = c[1];
            colors[3 * i + 2] = c[2];
        }
    }
}

// svob_mesh is versioned by size like svob_limits; everything a launch would trust is checked here, on the host.
int read_mesh(const svob_mesh *in, Mesh *out) {
    *out = Mesh();
    if (!in) return fail(SVOB_ERR_ARG, "null mesh");
    if (in->size < 2 * sizeof(uint32_t)) return fail(SVOB_ERR_ARG, "svob_mesh.size must hold at least size and flags");
    if (in->size > sizeof(svob_mesh))
        return fail(SVOB_ERR_ARG, "svob_mesh.size " + std::to_string(in->size) + " is larger than this library's (" +
                                      std::to_string(sizeof(svob_mesh)) + "): a newer ABI");
    svob_mesh k;
    std::memset(&k, 0, sizeof k);   // fields past the caller's size: zero (no triangles, no colours)
    std::memcpy(&k, in, in->size);
    if (k.flags & ~(uint32_t)SVOB_MESH_FLIP_WINDING) return fail(SVOB_ERR_ARG, "unknown svob_mesh.flags bits");
    if (k.n_triangles >= 0xFFFFFFFFull) return fail(SVOB_ERR_ARG, "svob_mesh.n_triangles must be below 2^32 - 1");
    if (k.n_vertices > 0xFFFFFFFFull) return fail(SVOB_ERR_ARG, "svob_mesh.n_vertices must fit 32 bits (the indices do)");
    if (k.n_vertices && !k.positions) return fail(SVOB_ERR_ARG, "svob_mesh.positions is null");
    if (k.n_triangles && !k.indices) return fail(SVOB_ERR_ARG, "svob_mesh.indices is null");
    for (size_t i = 0; i < 3 * k.n_vertices; ++i)
        if (!std::isfinite(k.positions[i]))
            return fail(SVOB_ERR_ARG, "svob_mesh.positions: vertex " + std::to_string(i / 3) + " is not finite");
    for (size_t i = 0; i < 3 * k.n_triangles; ++i)
        if (k.indices[i] >= k.n_vertices)
            return fail(SVOB_ERR_ARG, "svob_mesh.indices: triangle " + std::to_string(i / 3) + " names vertex " +
                                          std::to_string(k.indices[i]) + " of " + std::to_string(k.n_vertices));
    out->flags = k.flags;
    out->positions = k.positions;
    out->n_vertices = k.n_vertices;
    out->indices = k.indices;
    out->n_triangles = k.n_triangles;
    out->colors = k.colors;
    return SVOB_OK;
}

// Planes per z-slab of the owner grid (4 n^2 bytes a plane, no halo): clamp(cell_bytes / (4 n^2), 1, n), or
// slab_rows.  A budget below one plane is an error, not an allocation beyond it.
int mesh_slab_rows(int max_level, const Limits &lim, int *rows) {
    const uint64_t n = 1ull << (max_level - 1);
    const uint64_t plane = 4 * n * n;   // n <= 2^21: 2^44
    if (plane > lim.cell_bytes)
        return fail(SVOB_ERR_ARG, "max_level " + std::to_string(max_level) + ": one plane of the owner grid takes " +
                                      std::to_string(plane) + " bytes, more than svob_limits.cell_bytes (" +
                                      std::to_string(lim.cell_bytes) + ")");
    if (lim.slab_rows > 0) *rows = (int)std::min<uint64_t>((uint64_t)lim.slab_rows, n);
    else *rows = (int)std::min<uint64_t>(n, lim.cell_bytes / plane);
    return SVOB_OK;
}

struct MeshLeaves {
    std::vector<uint64_t> codes;
    std::vector<uint32_t> owners;
    std::vector<V3> normals, colors;   // colors: empty when the mesh has none
};

// svob_mesh_profile: device-event time per kernel of the calling thread's mesh builds.  Off by default (each
// timed launch is followed by an event wait, which a build does not want).
enum { MESH_K_SETUP, MESH_K_COUNT, MESH_K_SCAN, MESH_K_OVERLAP, MESH_K_COMPACT, MESH_K_ATTR, MESH_KERNELS };
thread_local bool g_mesh_profile = false;
thread_local double g_mesh_ms[MESH_KERNELS] = { 0, 0, 0, 0, 0, 0 };

struct KernelClock {
    bool on = false;
    hipEvent_t a = nullptr, b = nullptr;
    int slot = 0;
    void open() {
        on = g_mesh_profile && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
        if (on) for (double &v : g_mesh_ms) v = 0.0;
    }
    void begin(int s) {
        slot = s;
        if (on) (void)hipEventRecord(a, 0);
    }
    void end() {
        if (!on) return;
        float ms = 0.0f;
        if (hipEventRecord(b, 0) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
            hipEventElapsedTime(&ms, a, b) == hipSuccess)
            g_mesh_ms[slot] += (double)ms;
    }
    ~KernelClock() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

void write_report(svob_report *rep, const svob_report &k0) {
    if (!rep) return;   // rep->size was checked by the entry point
    svob_report k = k0;
    const size_t nb = std::min<size_t>(rep->size, sizeof k);
    k.size = (uint32_t)nb;
    std::memcpy(rep, &k, nb);
}

void write_stats(svob_mesh_stats *st, const svob_mesh_stats &k0) {
    if (!st) return;
    svob_mesh_stats k = k0;
    const size_t nb = std::min<size_t>(st->size, sizeof k);
    k.size = (uint32_t)nb;
    std::memcpy(st, &k, nb);
}

int mesh_leaves_gpu(int device, const Mesh &mesh, int max_level, int rows, const Limits &lim, svob_report *rep,
                    svob_mesh_stats *stats, MeshLeaves &out) {
    const int depth = max_level - 1;
    const int n = 1 << depth;
    const uint32_t n_tri = (uint32_t)mesh.n_triangles;
    svob_report r;
    std::memset(&r, 0, sizeof r);
    svob_mesh_stats s;
    std::memset(&s, 0, sizeof s);
    r.slab_rows = (uint32_t)rows;
    size_t cap = lim.list_capacity ? (size_t)lim.list_capacity : std::max<size_t>(1 << 20, (size_t)n * n * 4);
    r.list_capacity = cap;
    out = MeshLeaves();
    if (n_tri == 0) {   // nothing to launch
        write_report(rep, r);
        write_stats(stats, s);
        return SVOB_OK;
    }
    HIPB(hipSetDevice(device));
    float *dpos = nullptr, *dcol = nullptr, *dnrm = nullptr, *dleafcol = nullptr;
    uint32_t *didx = nullptr, *grid = nullptr, *downers = nullptr;
    Tri *dtris = nullptr;
    unsigned long long *dscan = nullptr, *dstats = nullptr, *dcount = nullptr;
    uint64_t *dcodes = nullptr;
    auto cleanup = [&]() {
        for (void *p : { (void *)dpos, (void *)dcol, (void *)dnrm, (void *)dleafcol, (void *)didx, (void *)grid,
                         (void *)downers, (void *)dtris, (void *)dscan, (void *)dstats, (void *)dcount, (void *)dcodes })
            if (p) (void)hipFree(p);
    };
    const size_t plane = (size_t)n * n;
    hipError_t e = hipMalloc(&dpos, std::max<size_t>(1, mesh.n_vertices) * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dpos, mesh.positions, mesh.n_vertices * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&didx, (size_t)n_tri * 3 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(didx, mesh.indices, (size_t)n_tri * 3 * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && mesh.colors) {
        e = hipMalloc(&dcol, mesh.n_vertices * 3 * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(dcol, mesh.colors, mesh.n_vertices * 3 * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc(&dtris, (size_t)n_tri * sizeof(Tri));
    if (e == hipSuccess) e = hipMalloc(&dscan, ((size_t)n_tri + 1) * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&dstats, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(dstats, 0, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&dcount, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&grid, plane * (size_t)rows * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&dcodes, cap * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&downers, cap * sizeof(uint32_t));
    if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("mesh alloc: ") + hipGetErrorString(e)); }

    KernelClock clock;
    clock.open();
    clock.begin(MESH_K_SETUP);
    hipLaunchKernelGGL(mesh_setup_kernel, dim3(blocks_for(n_tri, lim)), dim3(256), 0, 0, dpos, didx, n_tri, n, dtris, dstats);
    clock.end();
    e = hipGetLastError();
    if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("mesh setup launch: ") + hipGetErrorString(e)); }

    std::vector<std::pair<uint64_t, uint32_t>> leaves;
    std::vector<uint64_t> hcodes;
    std::vector<uint32_t> howners;
    for (int z0 = 0; z0 < n; z0 += rows) {
        const int zc = std::min(rows, n - z0);
        const int z1 = z0 + zc - 1;
        ++r.slabs;
        clock.begin(MESH_K_COUNT);
        hipLaunchKernelGGL(mesh_count_kernel, dim3(blocks_for((size_t)n_tri + 1, lim)), dim3(256), 0, 0, dtris, n_tri, z0, z1,
                           dscan);
        clock.end();
        clock.begin(MESH_K_SCAN);
        hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(256), 0, 0, dscan, (size_t)n_tri + 1);
        clock.end();
        e = hipGetLastError();
        unsigned long long total = 0;
        if (e == hipSuccess) e = hipMemcpy(&total, dscan + n_tri, sizeof total, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("mesh count: ") + hipGetErrorString(e)); }
        if (total == 0) continue;   // no triangle's box reaches this slab
        e = hipMemset(grid, 0xFF, plane * (size_t)zc * sizeof(uint32_t));
        for (uint64_t c0 = 0, c1 = 0; e == hipSuccess && c0 < total; c0 = c1) {
            // 64-bit: a slab may hold more than one launch takes; the limit may be anything from 1 to 2^64 - 1
            c1 = total - c0 > lim.launch_candidates ? c0 + lim.launch_candidates : total;
            ++r.overlap_launches;
            clock.begin(MESH_K_OVERLAP);
            hipLaunchKernelGGL(mesh_overlap_kernel, dim3(blocks_for((size_t)(c1 - c0), lim)), dim3(256), 0, 0, dtris, dscan,
                               n_tri, n, z0, z1, c0, c1, grid, dstats + 3);
            clock.end();
            e = hipGetLastError();
        }
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("mesh overlap: ") + hipGetErrorString(e)); }
        for (;;) {
            e = hipMemset(dcount, 0, sizeof(unsigned long long));
            if (e != hipSuccess) break;
            clock.begin(MESH_K_COMPACT);
            hipLaunchKernelGGL(mesh_compact_kernel, dim3(blocks_for((plane * (size_t)zc + 3) / 4, lim)), dim3(256), 0, 0, grid, n, z0, zc,
                               dcodes, downers, dcount, (unsigned long long)cap);
            clock.end();
            e = hipGetLastError();
            if (e != hipSuccess) break;
            unsigned long long cnt = 0;
            e = hipMemcpy(&cnt, dcount, sizeof(cnt), hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            if (cnt <= cap) {
                hcodes.resize(cnt);
                howners.resize(cnt);
                e = hipMemcpy(hcodes.data(), dcodes, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost);
                if (e == hipSuccess) e = hipMemcpy(howners.data(), downers, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost);
                for (size_t i = 0; i < cnt; ++i) leaves.emplace_back(hcodes[i], howners[i]);
                break;
            }
            // the kernel stored only the first cap leaves (k < cap): grow the list and compact again
            (void)hipFree(dcodes);
            (void)hipFree(downers);
            dcodes = nullptr;
            downers = nullptr;
            cap = (size_t)(cnt * 1.25) + 1024;
            ++r.relaunches;
            e = hipMalloc(&dcodes, cap * sizeof(uint64_t));
            if (e == hipSuccess) e = hipMalloc(&downers, cap * sizeof(uint32_t));
            if (e != hipSuccess) break;
        }
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("mesh compact: ") + hipGetErrorString(e)); }
    }
    r.list_capacity = cap;
    std::sort(leaves.begin(), leaves.end());   // each voxel appears once: the codes are unique
    const size_t m = leaves.size();
    out.codes.resize(m);
    out.owners.resize(m);
    for (size_t i = 0; i < m; ++i) {
        out.codes[i] = leaves[i].first;
        out.owners[i] = leaves[i].second;
    }
    out.normals.resize(m);
    if (mesh.colors) out.colors.resize(m);
    if (m) {
        if (m > cap) {
            (void)hipFree(dcodes);
            (void)hipFree(downers);
            dcodes = nullptr;
            downers = nullptr;
            e = hipMalloc(&dcodes, m * sizeof(uint64_t));
            if (e == hipSuccess) e = hipMalloc(&downers, m * sizeof(uint32_t));
            r.normals_regrown = 1;
        }
        if (e == hipSuccess) e = hipMemcpy(dcodes, out.codes.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(downers, out.owners.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&dnrm, m * 3 * sizeof(float));
        if (e == hipSuccess && mesh.colors) e = hipMalloc(&dleafcol, m * 3 * sizeof(float));
        if (e == hipSuccess) {
            clock.begin(MESH_K_ATTR);
            hipLaunchKernelGGL(mesh_attr_kernel, dim3(blocks_for(m, lim)), dim3(256), 0, 0, dtris, didx, dcol, dcodes, downers, m,
                               mesh.flags & (uint32_t)SVOB_MESH_FLIP_WINDING, dnrm, dleafcol);
            clock.end();
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(out.normals.data(), dnrm, m * 3 * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess && mesh.colors)
            e = hipMemcpy(out.colors.data(), dleafcol, m * 3 * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { cleanup(); return fail(SVOB_ERR_HIP, std::string("mesh attributes: ") + hipGetErrorString(e)); }
    }
    unsigned long long hstats[4] = { 0, 0, 0, 0 };
    e = hipMemcpy(hstats, dstats, sizeof hstats, hipMemcpyDeviceToHost);
    cleanup();
    if (e != hipSuccess) return fail(SVOB_ERR_HIP, std::string("mesh stats: ") + hipGetErrorString(e));
    s.degenerate = hstats[0];
    s.outside = hstats[1];
    s.candidates = hstats[2];
    s.overlaps = hstats[3];
    write_report(rep, r);
    write_stats(stats, s);
    return SVOB_OK;
}

// What both mesh entry points check before a device is touched.
int check_mesh_call(const svob_mesh *mesh, int max_level, const svob_limits *limits, const svob_report *report,
                    const svob_mesh_stats *stats, Mesh *m, Limits *lim, int *rows) {
    if (max_level < 2 || max_level > 22) return fail(SVOB_ERR_ARG, "max_level must be in [2, 22]");
    int rc = read_mesh(mesh, m);
    if (rc) return rc;
    rc = read_limits(limits, lim);
    if (rc) return rc;
    if (report && report->size < sizeof(uint32_t)) return fail(SVOB_ERR_ARG, "svob_report.size must hold at least size");
    if (stats && stats->size < sizeof(uint32_t)) return fail(SVOB_ERR_ARG, "svob_mesh_stats.size must hold at least size");
    return mesh_slab_rows(max_level, *lim, rows);
}


// Empty tree: CompressSVO's placeholder descriptor 0 stays 0; the root's
// attachment still encodes its default normal Vector3.up (Node ctor, Util.cs)
// with no children (NaiveCreator.cs:132-136, 195-257).
int empty_tree(int depth, svob_result *out) {
    out->n_nodes = 1; out->depth = depth; out->v1_ok = 1; out->n_leaves = 0;
    out->nodes = (uint64_t *)std::calloc(1, sizeof(uint64_t));
    out->attachments = (uint32_t *)std::calloc(2, sizeof(uint32_t));
    out->descriptors = (int32_t *)std::calloc(1, sizeof(int32_t));
    if (!out->nodes || !out->attachments || !out->descriptors) return fail(SVOB_ERR_MEM, "out of host memory");
    out->attachments[1] = encode_normal16({ 0.0f, 1.0f, 0.0f }) << 16;
    return SVOB_OK;
}

int check_sampler(int type, int max_level) {
    if (type < 0 || type > 4) return fail(SVOB_ERR_ARG, "unknown sampler");
    if (max_level < 2 || max_level > 22) return fail(SVOB_ERR_ARG, "max_level must be in [2, 22]");
    return SVOB_OK;
}

}  // namespace

extern "C" {

const char *svob_last_error(void) { return g_err.c_str(); }

void svob_free_ptr(void *p) { std::free(p); }

void svob_free(svob_result *r) {
    if (!r) return;
    std::free(r->descriptors);
    std::free(r->nodes);
    std::free(r->attachments);
    std::memset(r, 0, sizeof(*r));
}

int svob_opensimplex_table(int8_t *out) {
    if (!out) return fail(SVOB_ERR_ARG, "null out");
    static Simplex3 s;
    int rc = init_simplex(&s, 7);
    if (rc) return rc;
    std::memset(out, 0, 2048 * 25);
    for (int h = 0; h < 2048; ++h) {
        const int li = s.list_of_hash[h];
        if (li < 0) continue;
        const ContribList &c = s.lists[li];
        out[h * 25] = (int8_t)c.count;
        for (int j = 0; j < c.count; ++j) {
            out[h * 25 + 1 + 3 * j] = (int8_t)c.ox[j];
            out[h * 25 + 2 + 3 * j] = (int8_t)c.oy[j];
            out[h * 25 + 3 + 3 * j] = (int8_t)c.oz[j];
        }
    }
    return SVOB_OK;
}

int svob_eval_sampler(int sampler, size_t n, const float *xyz, float *out) {
    if (!xyz || !out) return fail(SVOB_ERR_ARG, "null argument");
    if (sampler < 0 || sampler > 4) return fail(SVOB_ERR_ARG, "unsupported sampler");
    static Simplex3 s;
    static bool ready = false;
    if (!ready) {
        int rc = init_simplex(&s, 7);
        if (rc) return rc;
        ready = true;
    }
    for (size_t i = 0; i < n; ++i) out[i] = sample(s, sampler, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return SVOB_OK;
}

int svob_slab_rows(int max_level, const svob_limits *limits) {
    if (max_level < 2 || max_level > 22) return fail(SVOB_ERR_ARG, "max_level must be in [2, 22]");
    Limits lim;
    int rc = read_limits(limits, &lim);
    if (rc) return rc;
    return slab_rows_of(1 << (max_level - 1), lim);
}

int svob_surface_leaves(int device, int sampler, int max_level, size_t *n_leaves, uint64_t **morton_out,
                        float **normals_out) {
    return svob_surface_leaves_ex(device, sampler, max_level, nullptr, nullptr, n_leaves, morton_out, normals_out);
}

int svob_surface_leaves_ex(int device, int sampler, int max_level, const svob_limits *limits, svob_report *report,
                           size_t *n_leaves, uint64_t **morton_out, float **normals_out) {
    if (!n_leaves || !morton_out || !normals_out) return fail(SVOB_ERR_ARG, "null argument");
    int rc = check_sampler(sampler, max_level);
    if (rc) return rc;
    Limits lim;
    rc = read_limits(limits, &lim);
    if (rc) return rc;
    if (report && report->size < sizeof(uint32_t)) return fail(SVOB_ERR_ARG, "svob_report.size must hold at least size");
    std::vector<uint64_t> codes;
    std::vector<V3> normals;
    rc = surface_leaves_gpu(device, sampler, max_level, lim, report, codes, normals);
    if (rc) return rc;
    *n_leaves = codes.size();
    *morton_out = (uint64_t *)std::malloc(std::max<size_t>(1, codes.size()) * sizeof(uint64_t));
    *normals_out = (float *)std::malloc(std::max<size_t>(1, codes.size()) * 3 * sizeof(float));
    if (!*morton_out || !*normals_out) return fail(SVOB_ERR_MEM, "out of host memory");
    std::memcpy(*morton_out, codes.data(), codes.size() * sizeof(uint64_t));
    std::memcpy(*normals_out, normals.data(), codes.size() * 3 * sizeof(float));
    return SVOB_OK;
}

int svob_build_from_leaves(int depth, size_t n_leaves, const uint32_t *xyz, const float *normals, const float *colors,
                           svob_result *out) {
    if (!out || (n_leaves && (!xyz || !normals))) return fail(SVOB_ERR_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (depth < 1 || depth > 21) return fail(SVOB_ERR_ARG, "depth must be in [1, 21]");
    const uint32_t n = 1u << depth;
    std::vector<std::pair<uint64_t, size_t>> order(n_leaves);
    for (size_t i = 0; i < n_leaves; ++i) {
        const uint32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (x >= n || y >= n || z >= n) return fail(SVOB_ERR_ARG, "leaf coordinate outside the grid");
        order[i] = { spread3_h(x) | (spread3_h(y) << 1) | (spread3_h(z) << 2), i };
    }
    std::sort(order.begin(), order.end());
    for (size_t i = 1; i < n_leaves; ++i)
        if (order[i].first == order[i - 1].first) return fail(SVOB_ERR_ARG, "duplicate leaf coordinates");
    if (n_leaves == 0) return empty_tree(depth, out);
    std::vector<uint64_t> codes(n_leaves);
    std::vector<V3> nrm(n_leaves), col(n_leaves);
    const float inv = std::ldexp(1.0f, -depth);
    for (size_t i = 0; i < n_leaves; ++i) {
        const size_t s = order[i].second;
        codes[i] = order[i].first;
        nrm[i] = { normals[3 * s], normals[3 * s + 1], normals[3 * s + 2] };
        if (colors) col[i] = { colors[3 * s], colors[3 * s + 1], colors[3 * s + 2] };
        else col[i] = { (float)xyz[3 * s] * inv, (float)xyz[3 * s + 1] * inv, (float)xyz[3 * s + 2] * inv };
    }
    return layout_from_sorted(depth, codes, nrm, col, out);
}

int svob_build_sampler(int device, int sampler, int max_level, svob_result *out) {
    return svob_build_sampler_ex(device, sampler, max_level, nullptr, nullptr, out);
}

int svob_build_sampler_ex(int device, int sampler, int max_level, const svob_limits *limits, svob_report *report,
                          svob_result *out) {
    if (!out) return fail(SVOB_ERR_ARG, "null out");
    std::memset(out, 0, sizeof(*out));
    int rc = check_sampler(sampler, max_level);
    if (rc) return rc;
    Limits lim;
    rc = read_limits(limits, &lim);
    if (rc) return rc;
    if (report && report->size < sizeof(uint32_t)) return fail(SVOB_ERR_ARG, "svob_report.size must hold at least size");
    std::vector<uint64_t> codes;
    std::vector<V3> normals;
    rc = surface_leaves_gpu(device, sampler, max_level, lim, report, codes, normals);
    if (rc) return rc;
    const int depth = max_level - 1;
    if (codes.empty()) return empty_tree(depth, out);
    std::vector<V3> col(codes.size());
    const float inv = std::ldexp(1.0f, -depth);
    for (size_t i = 0; i < codes.size(); ++i)   // node.color = position - 1 (NaiveCreator.cs:66)
        col[i] = { (float)compact3_h(codes[i]) * inv, (float)compact3_h(codes[i] >> 1) * inv,
                   (float)compact3_h(codes[i] >> 2) * inv };
    return layout_from_sorted(depth, codes, normals, col, out);
}

int svob_mesh_leaves(int device, const svob_mesh *mesh, int max_level, const svob_limits *limits, svob_report *report,
                     svob_mesh_stats *stats, size_t *n_leaves, uint64_t **morton_out, float **normals_out,
                     float **colors_out, uint32_t **owner_out) {
    if (!n_leaves || !morton_out || !normals_out || !owner_out) return fail(SVOB_ERR_ARG, "null argument");
    *n_leaves = 0;
    *morton_out = nullptr;
    *normals_out = nullptr;
    *owner_out = nullptr;
    if (colors_out) *colors_out = nullptr;
    Mesh m;
    Limits lim;
    int rows = 0;
    int rc = check_mesh_call(mesh, max_level, limits, report, stats, &m, &lim, &rows);
    if (rc) return rc;
    MeshLeaves L;
    rc = mesh_leaves_gpu(device, m, max_level, rows, lim, report, stats, L);
    if (rc) return rc;
    const size_t k = L.codes.size(), k1 = std::max<size_t>(1, k);
    *n_leaves = k;
    *morton_out = (uint64_t *)std::malloc(k1 * sizeof(uint64_t));
    *normals_out = (float *)std::malloc(k1 * 3 * sizeof(float));
    *owner_out = (uint32_t *)std::malloc(k1 * sizeof(uint32_t));
    const bool want_col = colors_out && m.colors;
    if (want_col) *colors_out = (float *)std::malloc(k1 * 3 * sizeof(float));
    if (!*morton_out || !*normals_out || !*owner_out || (want_col && !*colors_out)) {
        std::free(*morton_out);
        std::free(*normals_out);
        std::free(*owner_out);
        if (want_col) std::free(*colors_out);
        *morton_out = nullptr;
        *normals_out = nullptr;
        *owner_out = nullptr;
        if (colors_out) *colors_out = nullptr;
        *n_leaves = 0;
        return fail(SVOB_ERR_MEM, "out of host memory");
    }
    std::memcpy(*morton_out, L.codes.data(), k * sizeof(uint64_t));
    std::memcpy(*normals_out, L.normals.data(), k * 3 * sizeof(float));
    std::memcpy(*owner_out, L.owners.data(), k * sizeof(uint32_t));
    if (want_col) std::memcpy(*colors_out, L.colors.data(), k * 3 * sizeof(float));
    return SVOB_OK;
}

int svob_mesh_profile(int enable, double *ms_out) {
    if (ms_out) std::memcpy(ms_out, g_mesh_ms, sizeof g_mesh_ms);
    g_mesh_profile = enable != 0;
    return SVOB_OK;
}

int svob_build_mesh(int device, const svob_mesh *mesh, int max_level, const svob_limits *limits, svob_report *report,
                    svob_mesh_stats *stats, svob_result *out) {
    if (!out) return fail(SVOB_ERR_ARG, "null out");
    std::memset(out, 0, sizeof(*out));
    Mesh m;
    Limits lim;
    int rows = 0;
    int rc = check_mesh_call(mesh, max_level, limits, report, stats, &m, &lim, &rows);
    if (rc) return rc;
    MeshLeaves L;
    rc = mesh_leaves_gpu(device, m, max_level, rows, lim, report, stats, L);
    if (rc) return rc;
    const int depth = max_level - 1;
    if (L.codes.empty()) return empty_tree(depth, out);
    if (!m.colors) {   // node.color = position - 1 (NaiveCreator.cs:66), as svob_build_from_leaves without colours
        L.colors.resize(L.codes.size());
        const float inv = std::ldexp(1.0f, -depth);
        for (size_t i = 0; i < L.codes.size(); ++i)
            L.colors[i] = { (float)compact3_h(L.codes[i]) * inv, (float)compact3_h(L.codes[i] >> 1) * inv,
                            (float)compact3_h(L.codes[i] >> 2) * inv };
    }
    return layout_from_sorted(depth, L.codes, L.normals, L.colors, out);
}


}  // extern "C"
