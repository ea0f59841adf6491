// sky_driver -- the sky rule of raytracingtest_amd/csrc/svo_sky.h on the CPU, for tests/test_sky.py:
//   sky_driver <dirs> <texels | -> <width> <height> <flags> <out>
// <dirs>: 3 floats per direction; <texels>: width x height x 4 floats, row 0 first ("-": no texture, the
// gradient); <out>: 5 floats per direction {r, g, b, u, v}.  Built with g++ -std=c++17 -O1
// -ffp-contract=off -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracingtest_amd/csrc/svo_sky.h"

static bool read_all(const char *path, std::vector<float> &v) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize(bytes > 0 ? (size_t)bytes / 4 : 0);
    const size_t n = v.empty() ? 0 : std::fread(v.data(), 4, v.size(), f);
    std::fclose(f);
    return n == v.size();
}

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: sky_driver <dirs> <texels | -> <width> <height> <flags> <out>\n");
        return 2;
    }
    std::vector<float> dirs, raw;
    if (!read_all(argv[1], dirs) || dirs.size() % 3 != 0) return 3;
    const bool textured = std::strcmp(argv[2], "-") != 0;
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    const uint32_t flags = (uint32_t)std::strtoul(argv[5], nullptr, 0);
    std::vector<svo_sky::Texel> texels;
    if (textured) {
        if (w <= 0 || h <= 0 || w > svo_sky::MAX_DIM || h > svo_sky::MAX_DIM) return 3;
        if (!read_all(argv[2], raw) || raw.size() != (size_t)w * (size_t)h * 4) return 3;
        texels.resize((size_t)w * (size_t)h);
        std::memcpy(texels.data(), raw.data(), raw.size() * 4);
    }
    const svo_sky::Texture tex = {textured ? texels.data() : nullptr, w, h, flags};
    const size_t n = dirs.size() / 3;
    std::vector<float> out(n * 5);
    for (size_t i = 0; i < n; ++i) {
        svo_sky::sample(tex, &dirs[3 * i], &out[5 * i]);
        svo_sky::direction_uv(&dirs[3 * i], flags, &out[5 * i + 3], &out[5 * i + 4]);
    }
    std::FILE *f = std::fopen(argv[6], "wb");
    if (!f) return 4;
    const size_t wr = out.empty() ? 0 : std::fwrite(out.data(), 4, out.size(), f);
    return std::fclose(f) == 0 && wr == out.size() ? 0 : 5;
}
