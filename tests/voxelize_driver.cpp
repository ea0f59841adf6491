// voxelize_driver.cpp -- csrc/svo_voxelize.h through plain g++ (no HIP): the whole rule on the host, for
// tests/test_voxelize.py to compare with voxelize.py bit for bit.  Build with -ffp-contract=off like the library.
//   voxelize_driver in.bin out.bin
// in:  uint32 n_vertices, n_triangles, depth, flags (bit 0: colours follow, bit 1: flip), then positions (f32 x 3 v),
//      indices (u32 x 3 t), colours (f32 x 3 v).
// out: uint64 m, degenerate, outside, candidates, overlaps; then codes (u64 m), owners (u32 m), normals (f32 3m),
//      colours (f32 3m, when given).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../raytracingtest_amd/csrc/svo_voxelize.h"

using namespace svo_voxelize;

static uint64_t spread3(uint32_t v) {
    uint64_t x = 0;
    for (int b = 0; b < 21; ++b) x |= (uint64_t)((v >> b) & 1u) << (3 * b);
    return x;
}

template <class T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// voxelize_driver --decode in.bin out.bin: candidate_voxel on a list of cases.
// in:  uint64 count, then count x (uint64 local, bx, by), bx and by below 2^32.
// out: count x 9 uint32: candidate_voxel's (x, y, z), the 64-bit form's, and the 32-bit form's where local and
//      bx by fit 32 bits (zeros elsewhere).
static int decode_cases(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (fread(&count, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> cases;
    if (!read_vec(f, cases, 3 * (size_t)count)) return 2;
    fclose(f);
    std::vector<uint32_t> res(9 * (size_t)count, 0u);
    for (size_t k = 0; k < count; ++k) {
        const uint64_t local = cases[3 * k];
        const uint32_t bx = (uint32_t)cases[3 * k + 1], by = (uint32_t)cases[3 * k + 2];
        const uint64_t plane = (uint64_t)bx * by;
        candidate_voxel(local, bx, by, &res[9 * k]);
        candidate_voxel_64(local, bx, plane, &res[9 * k + 3]);
        if (((local | plane) >> 32) == 0) candidate_voxel_32((uint32_t)local, bx, (uint32_t)plane, &res[9 * k + 6]);
    }
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    if (count) fwrite(res.data(), 4, res.size(), o);
    return fclose(o) == 0 ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc == 4 && std::string(argv[1]) == "--decode") return decode_cases(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    const uint32_t nv = head[0], nt = head[1], depth = head[2];
    const bool has_col = head[3] & 1u, flip = head[3] & 2u;
    std::vector<float> pos, col;
    std::vector<uint32_t> idx;
    if (!read_vec(f, pos, 3 * (size_t)nv) || !read_vec(f, idx, 3 * (size_t)nt)) return 2;
    if (has_col && !read_vec(f, col, 3 * (size_t)nv)) return 2;
    fclose(f);

    const int n = 1 << depth;
    std::vector<Tri> tris(nt);
    std::vector<uint32_t> grid((size_t)n * n * n, NO_OWNER);
    uint64_t stats[4] = { 0, 0, 0, 0 };
    for (uint32_t t = 0; t < nt; ++t) {
        float p[9];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) p[3 * k + c] = pos[3 * (size_t)idx[3 * (size_t)t + k] + c];
        Tri &tri = tris[t];
        setup(p, n, &tri);
        if (tri.flags & TRI_DEGENERATE) { ++stats[0]; continue; }
        if (tri.flags & TRI_OUTSIDE) { ++stats[1]; continue; }
        stats[2] += candidates(tri, 0, n - 1);
        int i[3];
        for (i[2] = tri.blo[2]; i[2] <= tri.bhi[2]; ++i[2])
            for (i[1] = tri.blo[1]; i[1] <= tri.bhi[1]; ++i[1])
                for (i[0] = tri.blo[0]; i[0] <= tri.bhi[0]; ++i[0]) {
                    if (!in_box(tri, i) || !overlaps(tri, i)) continue;
                    ++stats[3];
                    uint32_t &cell = grid[((size_t)i[2] * n + i[1]) * n + i[0]];
                    cell = std::min(cell, t);
                }
    }
    std::vector<std::pair<uint64_t, uint32_t>> leaves;
    for (int z = 0; z < n; ++z)
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) {
                const uint32_t o = grid[((size_t)z * n + y) * n + x];
                if (o != NO_OWNER) leaves.emplace_back(spread3(x) | (spread3(y) << 1) | (spread3(z) << 2), o);
            }
    std::sort(leaves.begin(), leaves.end());
    const uint64_t m = leaves.size();
    std::vector<uint64_t> codes(m);
    std::vector<uint32_t> owners(m);
    std::vector<float> nrm(3 * m), leafcol(has_col ? 3 * m : 0);
    for (uint64_t k = 0; k < m; ++k) {
        codes[k] = leaves[k].first;
        owners[k] = leaves[k].second;
        const Tri &tri = tris[owners[k]];
        leaf_normal(tri, flip, &nrm[3 * k]);
        if (has_col) {
            int i[3] = { 0, 0, 0 };
            for (int b = 0; b < 21; ++b)
                for (int c = 0; c < 3; ++c) i[c] |= (int)((codes[k] >> (3 * b + c)) & 1u) << b;
            const uint32_t *v = &idx[3 * (size_t)owners[k]];
            leaf_color(tri, i, &col[3 * (size_t)v[0]], &col[3 * (size_t)v[1]], &col[3 * (size_t)v[2]], &leafcol[3 * k]);
        }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const uint64_t outhead[5] = { m, stats[0], stats[1], stats[2], stats[3] };
    fwrite(outhead, 8, 5, o);
    if (m) {   // an empty vector's data() may be null
        fwrite(codes.data(), 8, m, o);
        fwrite(owners.data(), 4, m, o);
        fwrite(nrm.data(), 4, 3 * m, o);
        if (has_col) fwrite(leafcol.data(), 4, 3 * m, o);
    }
    return fclose(o) == 0 ? 0 : 2;
}
