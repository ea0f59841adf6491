// reflect_driver -- the bounce rule of raytracingtest_amd/csrc/svo_reflect.h on the CPU, for
// tests/test_reflection.py:  reflect_driver <in> <out> <raw 0|1>
// <in>: records of 64 bytes {svo_ray (32), svo_hit (24), voxel key (8)}; <out>: one svo_ray per record,
// svo_bounce_rays' result.  Built with g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../raytracingtest_amd/csrc/svo_reflect.h"

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: reflect_driver <in> <out> <raw 0|1>\n");
        return 2;
    }
    const bool raw = argv[3][0] == '1';
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<uint32_t> out;
    uint32_t rec[16];
    while (std::fread(rec, sizeof rec, 1, in) == 1) {
        unsigned long long key;
        std::memcpy(&key, rec + 14, sizeof key);
        uint32_t o[8];
        svo_reflect::bounce_record(rec, rec + 8, key, raw, o);
        out.insert(out.end(), o, o + 8);
    }
    std::fclose(in);
    std::FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const size_t n = out.empty() ? 0 : std::fwrite(out.data(), 4, out.size(), f);
    return std::fclose(f) == 0 && n == out.size() ? 0 : 5;
}
