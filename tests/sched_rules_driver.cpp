// Evaluates the launch scheduling rules (raytracingtest_amd/csrc/svo_sched.h) on a table of cases:
// one case per line of stdin, "<rule> <arguments...>", one line of results each on stdout
// (tests/test_sched_rules.py).  A key is written width/seg/kpack; every other field of it is fixed.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "svo_sched.h"

using namespace svo_sched;

static Geo read_key(std::istream &in) {
    std::string tok;
    in >> tok;
    Geo g;
    g.local_rows = g.rows = 8;
    g.rank = 0;
    g.count = 1;
    g.xcd = 2;
    g.n_tiles = 80;
    if (std::sscanf(tok.c_str(), "%d/%d/%d", &g.width, &g.seg, &g.kpack) != 3) g.width = -2;
    return g;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string rule;
        if (!(in >> rule)) continue;
        if (rule == "loop") {
            unsigned long long T;
            uint32_t M;
            double slots, ratio, thin_ratio;
            int seg_min_chain, prior, prior_lat;
            in >> T >> M >> slots >> ratio >> thin_ratio >> seg_min_chain >> prior >> prior_lat;
            const LoopForm f = loop_form(T, M, slots, ratio, thin_ratio, seg_min_chain, prior != 0, prior_lat != 0);
            std::printf("%d %d %d\n", (int)f.lat, (int)f.is_short, (int)f.thin);
        } else if (rule == "slots") {
            int num_cus;
            unsigned long long lds;
            in >> num_cus >> lds;
            std::printf("%.0f\n", lean_slots(num_cus, (size_t)lds));
        } else if (rule == "stats") {
            uint32_t w[16];
            for (uint32_t &x : w) in >> x;
            const Stats s = reduce_stats(w);
            std::printf("%llu %u\n", (unsigned long long)s.T, s.M);
        } else if (rule == "class") {
            int a[10];
            for (int &x : a) in >> x;
            const ClassTable c = class_table(a[0], a[1], a[2] != 0, a[3] != 0, a[4] != 0, a[5] != 0, a[6], a[7], a[8], a[9]);
            std::printf("%d %d\n", c.kpack, c.seg);
        } else if (rule == "pick") {
            long long n, at[2];
            in >> n >> at[0] >> at[1];
            Geo keys[2];
            keys[0] = read_key(in);
            keys[1] = read_key(in);
            const Geo okey = read_key(in), key = read_key(in);
            std::printf("%d\n", pick_build(n, at, keys, okey, key));
        } else if (rule == "layout") {
            int a[8];
            for (int &x : a) in >> x;
            std::printf("%d\n", (int)other_layout(a[0] != 0, a[1] != 0, a[2], a[3], a[4], a[5], a[6], a[7]));
        } else if (rule == "refresh") {
            long long a[11];
            for (long long &x : a) in >> x;
            std::printf("%d\n", (int)needs_refresh(a[0] != 0, (uint64_t)a[1], (int)a[2], a[3] != 0, a[4] != 0, a[5] != 0,
                                                   a[6] != 0, a[7] != 0, a[8] != 0, (uint64_t)a[9], (int)a[10]));
        } else {
            std::printf("unknown rule %s\n", rule.c_str());
            return 2;
        }
        if (!in) {
            std::printf("bad arguments: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
