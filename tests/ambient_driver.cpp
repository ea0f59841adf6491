// ambient_driver -- the ambient rule of raytracingtest_amd/csrc/svo_ambient.h on the CPU, for
// tests/test_ambient.py:
//   ambient_driver tables <out>                     the 28 table rows, 3 f32 each (N = 4, 8, 16)
//   ambient_driver rays <in> <out> <raw 0|1> <n_rays> <radius bits, hex> <variant>
// <in>: records of 64 bytes {svo_ray (32), svo_hit (24), voxel key (8)}; <out>: n_rays svo_ray per record,
// svo_ambient_rays' result.  Built with g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../raytracingtest_amd/csrc/svo_ambient.h"

static int write_all(const char *path, const std::vector<uint32_t> &out) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return 4;
    const size_t n = out.empty() ? 0 : std::fwrite(out.data(), 4, out.size(), f);
    return std::fclose(f) == 0 && n == out.size() ? 0 : 5;
}

int main(int argc, char **argv) {
    std::vector<uint32_t> out;
    if (argc == 3 && std::string(argv[1]) == "tables") {
        for (int n = 4; n <= svo_ambient::MAX_RAYS; n *= 2)
            for (int k = 0; k < n; ++k) {
                float e[3];
                uint32_t w[3];
                svo_ambient::table_entry(n, k, e);
                std::memcpy(w, e, sizeof w);
                out.insert(out.end(), w, w + 3);
            }
        return write_all(argv[2], out);
    }
    if (argc != 8 || std::string(argv[1]) != "rays") {
        std::fprintf(stderr, "usage: ambient_driver tables <out> | rays <in> <out> <raw 0|1> <n_rays> <radius bits> <variant>\n");
        return 2;
    }
    const bool raw = argv[4][0] == '1';
    const int n_rays = std::atoi(argv[5]);
    const uint32_t radius_bits = (uint32_t)std::strtoul(argv[6], nullptr, 16);
    const uint32_t variant = (uint32_t)std::strtoul(argv[7], nullptr, 10);
    if (!svo_ambient::valid_count(n_rays) || variant > 7u) return 2;
    float radius;
    std::memcpy(&radius, &radius_bits, sizeof radius);
    std::FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 3;
    uint32_t rec[16], o[8 * svo_ambient::MAX_RAYS];
    while (std::fread(rec, sizeof rec, 1, in) == 1) {
        unsigned long long key;
        std::memcpy(&key, rec + 14, sizeof key);
        svo_ambient::ambient_record(rec, rec + 8, key, raw, n_rays, radius, variant, o);
        out.insert(out.end(), o, o + 8 * n_rays);
    }
    std::fclose(in);
    return write_all(argv[3], out);
}
