// placement_driver.cpp -- runs the placement-only kernels of libsvo_rt.so (tile order, strip
// order, query keys + sort) on caller-supplied inputs and returns everything they wrote, guard
// words included.  Host code only: it calls the launchers of csrc/svo_traverse.h and has no
// kernel of its own.  tests/placement_model.py holds the expected outputs.
//
//   placement_driver cases.bin results.bin
//
// Both files are little-endian u32 words.
//   cases:   MAGIC, n_cases, then per case: kind, p[8], len0, len1 (words), blob0, blob1
//   results: MAGIC, n_cases, then per case: kind, launcher's hipError_t, n_blobs, (len, words) per blob
//   kind 0  tile order   p = n, with_stats                         blob0 = cost (u16, n entries)
//           -> order [n + 4 + G], stats [16 + G]
//   kind 1  strip order  p = n, tiles_x, seg_cap, kpack, spread, with_part, expected error, with_stats
//                                                                   blob0 = cost, blob1 = part_cost (u16, 8 n)
//           -> order [order_strips_entries + G], stats [16 + G]
//   kind 2  query keys   p = n, flags                               blob0 = rays (32 n bytes)
//           -> keys, index, keys_out, index_out [n + G each]
// G = 64 guard words behind each buffer's documented size; every buffer is filled with GUARD
// before the launch, so an entry the kernel never wrote shows too.  The cost buffer holds
// order_cost_capacity(n) entries, its tail beyond n filled with 0xFFFF.
// All cases run on one stream.  Every HIP return and every launcher's return is checked: at the
// first error the driver prints the case number and the error and exits non-zero at once.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svo_traverse.h"

namespace {

constexpr uint32_t MAGIC = 0x31434C50u;   // "PLC1"
constexpr uint32_t GUARD = 0xA5C3F00Du;
constexpr size_t GUARD_WORDS = 64;
constexpr size_t MAX_WORDS = (size_t)1 << 26;   // no case needs a larger buffer

int g_case = -1;

[[noreturn]] void fail(const char *what, const char *detail) {
    std::fprintf(stderr, "placement_driver: case %d: %s: %s\n", g_case, what, detail);
    std::fflush(stderr);
    std::_Exit(1);   // nothing more is started on the device, not even its teardown
}

#define CK(e)                                                     \
    do {                                                          \
        const hipError_t e_ = (e);                                \
        if (e_ != hipSuccess) fail(#e, hipGetErrorString(e_));    \
    } while (0)

struct Buf {   // a device buffer of `words` documented words + GUARD_WORDS, all GUARD
    uint32_t *d = nullptr;
    size_t words = 0;
    explicit Buf(size_t w) : words(w) {
        if (w > MAX_WORDS) fail("buffer", "larger than any case needs");
        const std::vector<uint32_t> h(w + GUARD_WORDS, GUARD);
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

// device copy of `bytes` of src inside a buffer of `cap_bytes`, the rest filled with 0xFF
struct Input {
    void *d = nullptr;
    Input(const void *src, size_t bytes, size_t cap_bytes) {
        if (cap_bytes < bytes || cap_bytes > MAX_WORDS * 4) fail("input", "bad size");
        std::vector<unsigned char> h(cap_bytes ? cap_bytes : 16, 0xFF);
        std::memcpy(h.data(), src, bytes);
        CK(hipMalloc(&d, h.size()));
        CK(hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice));
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
        std::fprintf(stderr, "usage: placement_driver cases.bin results.bin\n");
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
        if (at + 11 > f.size()) fail("case file", "truncated header");
        const uint32_t kind = f[at];
        int p[8];
        for (int k = 0; k < 8; ++k) p[k] = (int)f[at + 1 + k];
        const size_t len0 = f[at + 9], len1 = f[at + 10];
        at += 11;
        if (len0 > f.size() - at || len1 > f.size() - at - len0) fail("case file", "truncated blob");
        const uint32_t *blob0 = f.data() + at, *blob1 = blob0 + len0;
        at += len0 + len1;
        const int n = p[0];
        if (n <= 0 || (size_t)n > MAX_WORDS / 16) fail("case", "bad n");
        put(out, kind);
        if (kind == 0 || kind == 1) {
            if (len0 * 2 < (size_t)n) fail("case", "cost blob shorter than n");
            const Input cost(blob0, (size_t)n * 2, svo::order_cost_capacity(n) * 2);
            const Buf stats(16);
            hipError_t e;
            if (kind == 0) {
                const Buf order((size_t)n + 4);
                e = svo::launch_order_tiles(static_cast<const uint16_t *>(cost.d), order.d, n, stream,
                                            p[1] ? stats.d : nullptr);
                CK(e);
                CK(hipStreamSynchronize(stream));
                put(out, (uint32_t)e);
                put(out, 2);
                order.emit(out);
                stats.emit(out);
            } else {
                const int tiles_x = p[1], seg_cap = p[2], kpack = p[3], spread = p[4], with_part = p[5];
                const hipError_t want = (hipError_t)p[6];
                if (tiles_x <= 0 || seg_cap < 0 || n % 8) fail("case", "bad strip shape");
                if (with_part && len1 * 2 < (size_t)n * svo::SEG_KMAX) fail("case", "part_cost blob shorter than 8 n");
                // a refused launch writes nothing: the buffer is then the plain order's size
                size_t entries = svo::order_strips_entries(n, seg_cap, svo::seg_kmax_of(kpack));
                if (want != hipSuccess) entries = svo::order_strips_entries(n, 0, 1);
                const Buf order(entries);
                const Input part(blob1, with_part ? (size_t)n * svo::SEG_KMAX * 2 : 0,
                                 with_part ? (size_t)n * svo::SEG_KMAX * 2 : 0);
                e = svo::launch_order_strips(static_cast<const uint16_t *>(cost.d), order.d, n, tiles_x, stream,
                                             p[7] ? stats.d : nullptr, seg_cap,
                                             with_part ? static_cast<const uint16_t *>(part.d) : nullptr, kpack, spread);
                if (e != want) fail("launch_order_strips", hipGetErrorString(e));
                CK(hipStreamSynchronize(stream));
                put(out, (uint32_t)e);
                put(out, 2);
                order.emit(out);
                stats.emit(out);
            }
        } else if (kind == 2) {
            if (len0 < (size_t)n * 8) fail("case", "ray blob shorter than n");
            const Input rays(blob0, (size_t)n * 32, (size_t)n * 32);
            const Buf keys(n), index(n), keys_out(n), index_out(n);
            svo::QueryArgs q;
            std::memset(&q, 0, sizeof q);
            q.rays = static_cast<const svo::QueryRay *>(rays.d);
            q.n = (uint32_t)n;
            q.flags = (uint32_t)p[1];
            const size_t temp_bytes = svo::query_sort_bytes(q.n);
            if (temp_bytes == 0 || temp_bytes > MAX_WORDS * 4) fail("query_sort_bytes", "no size");
            void *temp = nullptr;
            CK(hipMalloc(&temp, temp_bytes));
            CK(svo::launch_query_keys(q, keys.d, index.d, stream));
            CK(svo::launch_query_sort(keys.d, keys_out.d, index.d, index_out.d, q.n, temp, temp_bytes, stream));
            CK(hipStreamSynchronize(stream));
            CK(hipFree(temp));
            put(out, (uint32_t)hipSuccess);
            put(out, 4);
            keys.emit(out);
            index.emit(out);
            keys_out.emit(out);
            index_out.emit(out);
        } else {
            fail("case", "unknown kind");
        }
    }
    CK(hipStreamDestroy(stream));
    if (std::fclose(out) != 0) fail("result file", "close failed");
    std::printf("placement_driver: ok, %u cases\n", n_cases);
    return 0;
}
