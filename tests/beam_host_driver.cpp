// beam_host_driver.cpp -- evaluates the host side of the beam starts (csrc/svo_beam.h: the splat
// list of a pool, the splat's view of a camera) on caller-supplied inputs.  A plain C++ program: it
// includes only that header, makes no HIP call and links no library.  tests/beam_model.py holds the
// expected outputs; tests/test_beam_host.py also runs this program under ASan + UBSan.
//
//   beam_host_driver cases.bin results.bin
//
// Both files are little-endian u32 words.
//   cases:   MAGIC, n_cases, then per case: kind, ...
//     kind 0  splat list  n, depth, back (int), budget, lo[n], first[n]
//             -> 0, listed (0: null), finest_box_depth, count, count x (x | y << 16, z | depth << 16)
//     kind 1  camera      width, height, c2w[16], inv_proj[16] (f32 bits, svo::Camera's order)
//             -> 1, accepted, org[3], minv[9], plane[12] (f32 bits; what a refusal left behind is not defined)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svo_beam.h"

namespace {

constexpr uint32_t MAGIC = 0x31484D42u;   // "BMH1"

[[noreturn]] void fail(int ci, const char *what) {
    std::fprintf(stderr, "beam_host_driver: case %d: %s\n", ci, what);
    std::exit(1);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: beam_host_driver cases.bin results.bin\n");
        return 2;
    }
    std::vector<uint32_t> f;
    {
        std::FILE *in = std::fopen(argv[1], "rb");
        if (!in) fail(-1, "cannot open the case file");
        std::fseek(in, 0, SEEK_END);
        const long sz = std::ftell(in);
        std::fseek(in, 0, SEEK_SET);
        if (sz < 8 || sz % 4) fail(-1, "bad case file length");
        f.resize((size_t)sz / 4);
        if (std::fread(f.data(), 4, f.size(), in) != f.size()) fail(-1, "short read");
        std::fclose(in);
    }
    if (f[0] != MAGIC) fail(-1, "bad magic");
    const uint32_t n_cases = f[1];
    std::vector<uint32_t> out{MAGIC, n_cases};
    size_t at = 2;
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        if (at >= f.size()) fail((int)ci, "truncated");
        const uint32_t kind = f[at++];
        out.push_back(kind);
        if (kind == 0) {
            if (at + 4 > f.size()) fail((int)ci, "truncated header");
            const size_t n = f[at];
            const int depth = (int)f[at + 1], back = (int)f[at + 2];
            const size_t budget = f[at + 3];
            at += 4;
            if (n > f.size() - at || n > (f.size() - at) / 2) fail((int)ci, "truncated pool");
            // exact-size copies: a read past the n nodes is a heap overflow the sanitizer sees
            const std::vector<uint32_t> lo(f.begin() + (long)at, f.begin() + (long)(at + n));
            const std::vector<uint32_t> first(f.begin() + (long)(at + n), f.begin() + (long)(at + 2 * n));
            at += 2 * n;
            const auto boxes = svo_beam::build_beam_boxes(lo.data(), first.data(), n, depth, back, budget);
            out.push_back(boxes ? 1u : 0u);
            out.push_back((uint32_t)svo_beam::finest_box_depth(boxes));
            out.push_back(boxes ? (uint32_t)boxes->size() : 0u);
            if (boxes)
                for (const uint2 &b : *boxes) {
                    out.push_back(b.x);
                    out.push_back(b.y);
                }
        } else if (kind == 1) {
            if (at + 34 > f.size()) fail((int)ci, "truncated camera");
            svo::Camera cam;
            std::memset(&cam, 0, sizeof cam);
            const int width = (int)f[at], height = (int)f[at + 1];
            std::memcpy(cam.c2w, &f[at + 2], 64);
            std::memcpy(cam.inv_proj, &f[at + 18], 64);
            at += 34;
            svo::BeamParams bp;
            std::memset(&bp, 0, sizeof bp);
            const bool ok = svo_beam::beam_camera(cam, width, height, &bp);
            out.push_back(ok ? 1u : 0u);
            uint32_t w[24];
            std::memcpy(w, bp.org, 12);
            std::memcpy(w + 3, bp.minv, 36);
            std::memcpy(w + 12, bp.plane, 48);
            out.insert(out.end(), w, w + 24);
        } else {
            fail((int)ci, "unknown kind");
        }
    }
    if (at != f.size()) fail((int)n_cases, "trailing words");
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) fail(-1, "cannot open the result file");
    if (std::fwrite(out.data(), 4, out.size(), o) != out.size() || std::fclose(o) != 0) fail(-1, "write failed");
    std::printf("beam_host_driver: ok, %u cases\n", n_cases);
    return 0;
}
