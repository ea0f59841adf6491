// closest_driver -- the closest-voxel rule of raytracingtest_amd/csrc/svo_closest.h on the CPU, for
// tests/test_closest.py:
//   closest_driver <nodes> <queries> <nearest out> <contacts out> <root> <flags> <max_visits> <coarse_level>
// <nodes>: V2 words (first << 32 | valid8 << 8 | nonleaf8), the uploaded pool; <queries>: svo_shape records of 32
// bytes.  <nearest out>: one svo_closest per query; <contacts out>: one svo_contact per query, as
// svo_closest_voxels writes them.  max_visits 0: the default budget.  Parameters out of range: exit 6.
// Built with g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracingtest_amd/csrc/svo_closest.h"

namespace cl = svo_nearest;

template <class T>
static bool read_all(const char *path, std::vector<T> &out) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    T rec;
    while (std::fread(&rec, sizeof rec, 1, f) == 1) out.push_back(rec);
    std::fclose(f);
    return true;
}

template <class T>
static int write_all(const char *path, const std::vector<T> &out) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return 4;
    const size_t n = out.empty() ? 0 : std::fwrite(out.data(), sizeof(T), out.size(), f);
    return std::fclose(f) == 0 && n == out.size() ? 0 : 5;
}

struct Fetch {
    const std::vector<uint64_t> &nodes;
    cl::Node operator()(uint32_t i) const {
        if (i >= nodes.size()) return {0u, 0u};   // at or past the uploaded nodes: the zero descriptor
        return {(uint32_t)(nodes[i] & 0xFFFFu), (uint32_t)(nodes[i] >> 32)};
    }
};

struct Stack {
    uint32_t node[cl::STACK_LEVELS], first[cl::STACK_LEVELS], state[cl::STACK_LEVELS];
    void push(int level, uint32_t n, uint32_t f, uint32_t s) {
        if (level < 0 || level >= cl::STACK_LEVELS) std::abort();   // the rule says this cannot happen
        node[level] = n;
        first[level] = f;
        state[level] = s;
    }
    void pop(int level, uint32_t &n, uint32_t &f, uint32_t &s) const {
        if (level < 0 || level >= cl::STACK_LEVELS) std::abort();
        n = node[level];
        f = first[level];
        s = state[level];
    }
};

int main(int argc, char **argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: closest_driver <nodes> <queries> <nearest out> <contacts out> <root> <flags> "
                             "<max_visits> <coarse_level>\n");
        return 2;
    }
    std::vector<uint64_t> nodes;
    std::vector<cl::Shape> queries;
    if (!read_all(argv[1], nodes) || !read_all(argv[2], queries)) return 3;
    const uint32_t root = (uint32_t)std::strtoul(argv[5], nullptr, 10), flags = (uint32_t)std::strtoul(argv[6], nullptr, 10),
                   coarse = (uint32_t)std::strtoul(argv[8], nullptr, 10);
    uint32_t max_visits = (uint32_t)std::strtoul(argv[7], nullptr, 10);
    if ((flags & ~cl::UNBOUNDED) || max_visits > cl::MAX_VISITS || coarse > (uint32_t)cl::MAX_LEVEL) return 6;
    if (max_visits == 0) max_visits = cl::DEFAULT_VISITS;
    std::vector<cl::Closest> nearest(queries.size());
    std::vector<cl::Contact> contacts(queries.size(), svo_volumes::unused_contact());
    Fetch fetch{nodes};
    for (size_t i = 0; i < queries.size(); ++i) {
        if (!cl::query_valid(queries[i])) {
            nearest[i] = cl::nothing_found(0u, cl::FLAG_INVALID);
            continue;
        }
        Stack stack;
        nearest[i] = cl::walk(queries[i], root, flags, max_visits, coarse, fetch, stack, contacts[i]);
    }
    const int rc = write_all(argv[3], nearest);
    return rc ? rc : write_all(argv[4], contacts);
}
