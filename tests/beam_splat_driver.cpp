// beam_splat_driver.cpp -- runs the beam splat of libsvo_rt.so (svo_traverse.h launch_beam_splat) on
// caller-supplied BeamParams and box lists and returns the tile-start buffer after every launch, guard
// words included.  Host code only: it has no kernel of its own.  tests/beam_model.py holds the
// expected envelope of every word.
//
//   beam_splat_driver cases.bin results.bin
//
// Both files are little-endian u32 words.
//   cases:   MAGIC, n_cases, then per case: width, height, tiles_x, tiles_y, super_x, super_y, super_off,
//            global_off, n_boxes, n_steps, boxes[2 n_boxes], then per step: gen, org[3], minv[9], plane[12]
//            (f32 bits).  The steps run in order on the case's one buffer.
//   results: MAGIC, n_cases, then per case: n_steps, then per step: the launcher's hipError_t, len, the
//            buffer's len words
// The buffer holds tiles + supers + 1 u64 keys, all-ones before the first step, and G = 64 guard words
// behind them.  diag is always 0.  The tile geometry must be the one svo_rt.hip derives from the frame
// size (a case that says otherwise is refused before anything is launched), so no key can land outside
// the buffer.  One process, one stream.  Every HIP return and the launcher's return are checked: at the
// first error the driver prints the case number and the error and exits non-zero at once.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svo_traverse.h"

namespace {

constexpr uint32_t MAGIC = 0x31505342u;   // "BSP1"
constexpr uint32_t GUARD = 0xA5C3F00Du;
constexpr size_t GUARD_WORDS = 64;
constexpr size_t MAX_WORDS = (size_t)1 << 22;   // no case needs a larger buffer or box list
constexpr size_t STEP_WORDS = 25;

int g_case = -1;

[[noreturn]] void fail(const char *what, const char *detail) {
    std::fprintf(stderr, "beam_splat_driver: case %d: %s: %s\n", g_case, what, detail);
    std::fflush(stderr);
    std::_Exit(1);   // nothing more is started on the device, not even its teardown
}

#define CK(e)                                                     \
    do {                                                          \
        const hipError_t e_ = (e);                                \
        if (e_ != hipSuccess) fail(#e, hipGetErrorString(e_));    \
    } while (0)

struct Buf {   // a device buffer of `words` documented words, all-ones, + GUARD_WORDS of GUARD
    uint32_t *d = nullptr;
    size_t words = 0;
    explicit Buf(size_t w) : words(w) {
        if (w > MAX_WORDS) fail("buffer", "larger than any case needs");
        std::vector<uint32_t> h(w + GUARD_WORDS, GUARD);
        std::fill(h.begin(), h.begin() + (long)w, 0xFFFFFFFFu);
        CK(hipMalloc(reinterpret_cast<void **>(&d), h.size() * 4));
        CK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    Buf(const Buf &) = delete;
    void emit(std::FILE *out) const {
        std::vector<uint32_t> h(words + GUARD_WORDS);
        CK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost));
        const uint32_t len = (uint32_t)h.size();
        if (std::fwrite(&len, 4, 1, out) != 1 || std::fwrite(h.data(), 4, h.size(), out) != h.size())
            fail("result file", "write failed");
    }
    ~Buf() { CK(hipFree(d)); }
};

struct Input {   // device copy of `words` words (at least 16 bytes are allocated)
    void *d = nullptr;
    Input(const uint32_t *src, size_t words) {
        if (words > MAX_WORDS) fail("input", "larger than any case needs");
        CK(hipMalloc(&d, words ? words * 4 : 16));
        if (words) CK(hipMemcpy(d, src, words * 4, hipMemcpyHostToDevice));
    }
    Input(const Input &) = delete;
    ~Input() { CK(hipFree(d)); }
};

void put(std::FILE *out, uint32_t v) {
    if (std::fwrite(&v, 4, 1, out) != 1) fail("result file", "write failed");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: beam_splat_driver cases.bin results.bin\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) fail("case file", "cannot open");
    std::vector<uint32_t> f;
    {
        std::fseek(in, 0, SEEK_END);
        const long sz = std::ftell(in);
        std::fseek(in, 0, SEEK_SET);
        if (sz < 8 || sz % 4) fail("case file", "bad length");
        f.resize((size_t)sz / 4);
        if (std::fread(f.data(), 4, f.size(), in) != f.size()) fail("case file", "short read");
        std::fclose(in);
    }
    if (f[0] != MAGIC) fail("case file", "bad magic");
    const uint32_t n_cases = f[1];
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) fail("result file", "cannot open");
    put(out, MAGIC);
    put(out, n_cases);

    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    size_t at = 2;
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        g_case = (int)ci;
        if (at + 10 > f.size()) fail("case file", "truncated header");
        int p[8];
        for (int k = 0; k < 8; ++k) p[k] = (int)f[at + k];
        const size_t n_boxes = f[at + 8], n_steps = f[at + 9];
        at += 10;
        const int width = p[0], height = p[1];
        if (width <= 0 || height <= 0 || width > 4096 || height > 4096) fail("case", "bad frame size");
        const int tx = (width + 7) / 8, ty = (height + 7) / 8, sx = (width + 63) / 64, sy = (height + 63) / 64;
        if (p[2] != tx || p[3] != ty || p[4] != sx || p[5] != sy || p[6] != tx * ty || p[7] != tx * ty + sx * sy)
            fail("case", "tile geometry other than the frame size's");
        if (n_boxes > MAX_WORDS / 2 || 2 * n_boxes > f.size() - at) fail("case file", "truncated boxes");
        const uint32_t *boxes = f.data() + at;
        at += 2 * n_boxes;
        if (n_steps > 16 || n_steps * STEP_WORDS > f.size() - at) fail("case file", "truncated steps");
        for (size_t i = 0; i < n_boxes; ++i) {   // coordinates inside the cube at the box's depth
            const uint32_t d = boxes[2 * i + 1] >> 16;
            if (d < 1 || d > 16 || (boxes[2 * i] & 0xFFFFu) >> d || (boxes[2 * i] >> 16) >> d ||
                (boxes[2 * i + 1] & 0xFFFFu) >> d)
                fail("case", "a box outside the cube");
        }
        const Input dev_boxes(boxes, 2 * n_boxes);
        const Buf buf(2 * ((size_t)p[7] + 1));
        put(out, (uint32_t)n_steps);
        for (size_t s = 0; s < n_steps; ++s, at += STEP_WORDS) {
            svo::BeamParams bp;
            std::memset(&bp, 0, sizeof bp);
            bp.boxes = static_cast<const uint2 *>(dev_boxes.d);
            bp.n_boxes = (uint32_t)n_boxes;
            bp.tile_start = reinterpret_cast<unsigned long long *>(buf.d);
            bp.gen = f[at];
            if (bp.gen == 0 || bp.gen == 0xFFFFFFFFu) fail("case", "generation 0 or 2^32 - 1");
            bp.diag = 0;
            bp.tiles_x = tx;
            bp.tiles_y = ty;
            bp.super_x = sx;
            bp.super_y = sy;
            bp.super_off = p[6];
            bp.global_off = p[7];
            bp.width = width;
            bp.height = height;
            std::memcpy(bp.org, &f[at + 1], 12);
            std::memcpy(bp.minv, &f[at + 4], 36);
            std::memcpy(bp.plane, &f[at + 13], 48);
            for (size_t k = 1; k < STEP_WORDS; ++k)
                if ((f[at + k] & 0x7F800000u) == 0x7F800000u) fail("case", "a camera field that is not finite");
            const hipError_t e = svo::launch_beam_splat(bp, stream);
            CK(e);
            CK(hipStreamSynchronize(stream));
            put(out, (uint32_t)e);
            buf.emit(out);
        }
    }
    if (at != f.size()) fail("case file", "trailing words");
    CK(hipStreamDestroy(stream));
    if (std::fclose(out) != 0) fail("result file", "close failed");
    std::printf("beam_splat_driver: ok, %u cases\n", n_cases);
    return 0;
}
