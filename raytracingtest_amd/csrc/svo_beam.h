// svo_beam.h -- the host side of the beam starts: the splat list of a pool and the
// splat's view of a camera, as plain functions of host arrays: host code, no HIP call, no state, so
// a CPU test can pin them (tests/test_beam_host.py).  svo_traverse.h is included for Camera and
// BeamParams only.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "svo_traverse.h"

namespace svo_beam {

// The splat list of a tree: every box a primary ray can first hit a voxel in, at
// a fixed depth ds = depth - back -- the non-leaf nodes at ds and the leaves above it -- as
// (x | y << 16, z | depth << 16), box [1 + i 2^-depth, 1 + (i + 1) 2^-depth]^3 in SVO space.
// Child c of a node (bit c of its masks, NVIDIASVO.compute:83-94 with slot 7 - c) takes the upper
// half on axis k iff bit k of c is set; its node is first + (non-leaf children before it).
// A child index past the n nodes reads as an empty descriptor: nothing is listed below it.
// A pool whose subtrees are shared (linked sub-SVOs) expands them once per position; once the
// boxes listed and the nodes queued for the next level reach `budget`, the walk stops descending
// and lists the nodes it reaches as boxes of their own (coarser, still a lower bound: every voxel
// of the pool lies in one of the listed boxes).
// Null: ds = min(depth - back, 16) < 1 (16-bit coordinates), no nodes, or 2^32 - 1 boxes or more.
inline std::shared_ptr<const std::vector<uint2>> build_beam_boxes(const uint32_t *lo, const uint32_t *first, size_t n,
                                                                  int depth, int back,
                                                                  size_t budget = (size_t)1 << 23) {
    const int ds = std::min(depth - back, 16);   // 16-bit coordinates
    if (ds < 1 || n == 0) return nullptr;
    auto out = std::make_shared<std::vector<uint2>>();
    struct Item { uint32_t node, x, y, z; };
    std::vector<Item> cur{{0u, 0u, 0u, 0u}}, nxt;
    for (int d = 0; d < ds && !cur.empty(); ++d) {
        nxt.clear();
        for (const Item &it : cur) {
            const uint32_t m = lo[it.node] & 0xFFu, v = (lo[it.node] >> 8) & 0xFFu;
            uint32_t rank = 0;
            const bool descend = nxt.size() + out->size() < budget;
            for (uint32_t c = 0; c < 8; ++c) {
                const bool inner = (m >> c) & 1u;
                const uint32_t child = inner ? first[it.node] + rank++ : 0u;
                if (!((v >> c) & 1u)) continue;
                const uint32_t x = 2 * it.x + (c & 1u), y = 2 * it.y + ((c >> 1) & 1u), z = 2 * it.z + ((c >> 2) & 1u);
                if (inner && d + 1 < ds && descend) {
                    if (child < n) nxt.push_back({child, x, y, z});
                } else {
                    out->push_back(make_uint2(x | (y << 16), z | ((uint32_t)(d + 1) << 16)));
                }
            }
        }
        cur.swap(nxt);
    }
    if (out->size() >= 0xFFFFFFFFull) return nullptr;
    // Morton order (coordinates at 16 bits): a splat workgroup's boxes then cover a compact patch
    // of the screen (svo_kernel.hip beam_splat_kernel's LDS window)
    auto spread = [](uint64_t v) {
        v &= 0xFFFFull;
        v = (v | (v << 16)) & 0x0000FF0000FFull;
        v = (v | (v << 8)) & 0x00F00F00F00Full;
        v = (v | (v << 4)) & 0x0C30C30C30C3ull;
        v = (v | (v << 2)) & 0x249249249249ull;
        return v;
    };
    auto morton = [&](const uint2 &b) {
        const int sh = 16 - (int)(b.y >> 16);
        return spread((uint64_t)(b.x & 0xFFFFu) << sh) | spread((uint64_t)(b.x >> 16) << sh) << 1 |
               spread((uint64_t)(b.y & 0xFFFFu) << sh) << 2;
    };
    std::vector<std::pair<uint64_t, uint2>> keyed(out->size());
    for (size_t i = 0; i < out->size(); ++i) keyed[i] = {morton((*out)[i]), (*out)[i]};
    std::sort(keyed.begin(), keyed.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t i = 0; i < keyed.size(); ++i) (*out)[i] = keyed[i].second;
    return out;
}

// The depth of the finest box actually in a splat list (its side s_min = 2^-depth; budget-coarsened
// and linked pools included: whatever the walk above listed), 0 for no list.
inline int finest_box_depth(const std::shared_ptr<const std::vector<uint2>> &boxes) {
    uint32_t d = 0;
    if (boxes)
        for (const uint2 &b : *boxes) d = std::max(d, b.y >> 16);
    return (int)d;
}

// The splat's view of a camera (svo_traverse.h BeamParams: org, minv, plane; nothing else is
// written): origin, the inverse of the pixel -> direction map and the frustum's side planes (through
// the directions of the points one pixel outside the frame's corners), in double from the render's
// own formulas (svo_kernel.hip camera_ray).  False for a camera the splat cannot bound (non-finite,
// singular, or a field of view so wide that the projection's clipping margin no longer holds: the
// longest of the centre and corner directions more than 30 times the shortest).
inline bool beam_camera(const svo::Camera &c, int width, int height, svo::BeamParams *bp) {
    double A[3], B[3], C[3];
    for (int r = 0; r < 3; ++r) {   // dir = C3 (IP (u, v, 0, 1)).xyz, u = 2 fx / W - 1, v = 2 fy / H - 1
        A[r] = B[r] = C[r] = 0.0;
        for (int k = 0; k < 3; ++k) {
            A[r] += (double)c.c2w[k * 4 + r] * c.inv_proj[0 * 4 + k];
            B[r] += (double)c.c2w[k * 4 + r] * c.inv_proj[1 * 4 + k];
            C[r] += (double)c.c2w[k * 4 + r] * c.inv_proj[3 * 4 + k];
        }
    }
    double M[3][3];
    for (int r = 0; r < 3; ++r) {
        M[r][0] = 2.0 * A[r] / width;
        M[r][1] = 2.0 * B[r] / height;
        M[r][2] = C[r] - A[r] - B[r];
    }
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
                       M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    if (!std::isfinite(det) || det == 0.0) return false;
    double inv[3][3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            const int r1 = (k + 1) % 3, r2 = (k + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            inv[r][k] = (M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]) / det;   // adjugate / det
        }
    auto dir = [&](double fx, double fy, double d[3]) {
        for (int r = 0; r < 3; ++r) d[r] = M[r][0] * fx + M[r][1] * fy + M[r][2];
    };
    auto len = [](const double d[3]) { return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); };
    double D[4][3], mid[3];
    dir(-1.0, -1.0, D[0]);
    dir(width + 1.0, -1.0, D[1]);
    dir(width + 1.0, height + 1.0, D[2]);
    dir(-1.0, height + 1.0, D[3]);
    dir(0.5 * width, 0.5 * height, mid);
    double lmin = len(mid), lmax = len(mid);
    for (int j = 0; j < 4; ++j) {
        lmin = std::min(lmin, len(D[j]));
        lmax = std::max(lmax, len(D[j]));
    }
    if (!(lmin > 0.0) || lmax > 30.0 * lmin) return false;
    for (int j = 0; j < 4; ++j) {
        const double *a = D[j], *b = D[(j + 1) % 4];
        double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double sgn = n[0] * mid[0] + n[1] * mid[1] + n[2] * mid[2] < 0.0 ? -1.0 : 1.0;
        const double l = len(n);
        if (!(l > 0.0) || !std::isfinite(l)) return false;
        for (int k = 0; k < 3; ++k) bp->plane[j][k] = (float)(sgn * n[k] / l);
    }
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            bp->minv[3 * r + k] = (float)inv[r][k];
            if (!std::isfinite(bp->minv[3 * r + k])) return false;
        }
    for (int k = 0; k < 3; ++k) {   // mul4(c2w, (0, 0, 0, 1)) then to_svo, in f32 (both steps exact or one rounding)
        const float w = c.c2w[12 + k];
        if (!std::isfinite(w)) return false;
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(c.c2w[4 * j + k])) return false;
        bp->org[k] = w * (1.0f / 32.0f) + 1.5f;
    }
    return true;
}

}  // namespace svo_beam
