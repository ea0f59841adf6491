// object_driver -- the object rule of raytracingtest_amd/csrc/svo_object.h on the CPU, for tests/test_objects.py:
//   object_driver <in> <objects> <out> <raw 0|1>
// <in>: records of 64 bytes {svo_ray (32), best hit bit (u32), best t (f32), walk normal m (3 f32), candidate t
// (f32), 2 spare words}; <objects>: 1..8 svo_object records of 64 bytes.  <out>: 20 words per (record, object):
// {svo_object_rays' ray (8), the object ray is valid (1), the traced direction (3), t_in, t_out, t_entry, the
// cube test (4), the world normal (3), the fold's `replaces` (1)}.  An object that svo_set_objects would refuse:
// exit 6.  Built with g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracingtest_amd/csrc/svo_object.h"
#include "../raytracingtest_amd/csrc/svo_reflect.h"

static uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: object_driver <in> <objects> <out> <raw 0|1>\n");
        return 2;
    }
    const bool raw = argv[4][0] == '1';
    std::vector<svo_objects::Object> objects;
    {
        std::FILE *of = std::fopen(argv[2], "rb");
        if (!of) return 3;
        svo_objects::Object ob;
        while (std::fread(&ob, sizeof ob, 1, of) == 1) objects.push_back(ob);
        std::fclose(of);
    }
    if (objects.empty() || objects.size() > (size_t)svo_objects::MAX_OBJECTS) return 2;
    for (const svo_objects::Object &ob : objects)
        if (svo_objects::object_error(ob)) return 6;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<uint32_t> out;
    uint32_t rec[16];
    while (std::fread(rec, sizeof rec, 1, in) == 1) {
        float f[16];
        std::memcpy(f, rec, sizeof f);
        const bool best_hit = rec[8] != 0u;
        const float best_t = f[9], m[3] = {f[10], f[11], f[12]}, cand_t = f[13];
        for (const svo_objects::Object &ob : objects) {
            uint32_t o[8];
            svo_objects::object_entry(rec, ob, o);
            float g[8];
            std::memcpy(g, o, sizeof g);
            const float o2[3] = {g[0], g[1], g[2]};
            float d2[3] = {g[4], g[5], g[6]};
            const bool valid = svo_objects::valid_ray(o2, d2, g[3]);
            svo_reflect::clamp_direction(d2, raw);
            float t_in, t_out, n[3];
            svo_objects::cube_span(o2, d2, &t_in, &t_out);
            svo_objects::world_normal(ob.rotation, m, n);
            out.insert(out.end(), o, o + 8);
            const uint32_t tail[12] = {valid ? 1u : 0u, bits(d2[0]), bits(d2[1]), bits(d2[2]), bits(t_in), bits(t_out),
                                       bits(svo_objects::entry_t(t_in)),
                                       svo_objects::cube_test(t_in, t_out, best_hit, best_t) ? 1u : 0u,
                                       bits(n[0]), bits(n[1]), bits(n[2]),
                                       svo_objects::replaces(best_hit, best_t, cand_t) ? 1u : 0u};
            out.insert(out.end(), tail, tail + 12);
        }
    }
    std::fclose(in);
    std::FILE *wf = std::fopen(argv[3], "wb");
    if (!wf) return 4;
    const size_t w = out.empty() ? 0 : std::fwrite(out.data(), 4, out.size(), wf);
    return std::fclose(wf) == 0 && w == out.size() ? 0 : 5;
}
