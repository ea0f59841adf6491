// svo_sched.h -- the host's scheduling rules of a render launch (svo_rt.hip launch) as pure
// functions of a handful of integers: no HIP, no state, so a CPU test can pin them
// (tests/test_sched_rules.py).  The measurements behind each rule stand where launch() applies it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace svo_sched {

// The tile-order cache key: the exact geometry (and deal) an order was built for.
struct Geo {
    int width = -1, local_rows = -1, rows = -1, rank = -1, count = -1, xcd = -1, n_tiles = -1;
    int seg = 0;    // the order's seg_cap (segmented heavy tiles, svo_kernel.hip render_seg_kernel) ...
    int kpack = 0;  // ... and the K of each cost class (launch_order_strips' seg_kpack)
    uint64_t deal = 0;
    bool operator==(const Geo &o) const {
        return width == o.width && local_rows == o.local_rows && rows == o.rows && rank == o.rank &&
               count == o.count && xcd == o.xcd && n_tiles == o.n_tiles && seg == o.seg && kpack == o.kpack &&
               deal == o.deal;
    }
    bool operator!=(const Geo &o) const { return !(*this == o); }
};

// An order build's statistics (16 host-visible words: per XCD the max and the sum of the tile
// costs the order kernel saw): the heaviest tile M and the summed wave trips T.
struct Stats { uint64_t T; uint32_t M; };
inline Stats reduce_stats(const volatile uint32_t *st16) {
    Stats r{0, 0};
    for (int x = 0; x < 8; ++x) {
        r.M = std::max(r.M, (uint32_t)st16[2 * x]);
        r.T += st16[2 * x + 1];
    }
    return r;
}

// The lean loop's resident waves on the chip: its stack takes lds_bytes of a CU's 160 KiB per wave.
inline double lean_slots(int num_cus, size_t lds_bytes) {
    return (double)num_cus * (double)std::min<size_t>(32, (160 * 1024) / lds_bytes);
}

// Loop form: latency-bound when T < ratio x slots x M, with 15 % hysteresis around the ratio once
// this geometry and mode have a decision (prior); is_short: the heaviest chain is below
// seg_min_chain trips; thin: latency-bound and T below thin_ratio x slots x M (no hysteresis).
struct LoopForm { bool lat, is_short, thin; double bound; };   // bound: the ratio applied (the decision trace)
inline LoopForm loop_form(uint64_t T, uint32_t M, double slots, double ratio, double thin_ratio, int seg_min_chain,
                          bool prior, bool prior_lat) {
    LoopForm f;
    const double bound = f.bound = !prior ? ratio : prior_lat ? ratio * 1.15 : ratio / 1.15;
    f.lat = M > 0 && (double)T < bound * slots * (double)M;
    f.is_short = M < (uint32_t)seg_min_chain;
    f.thin = f.lat && (double)T < thin_ratio * slots * (double)M;
    return f;
}

// The class table (the K of each cost class) and seg_cap of the order a launch asks for.
struct ClassTable { int kpack, seg; };
inline ClassTable class_table(int seg_all, int seg_cap, bool latency_bound, bool lat_short, bool lat_thin, bool jittered,
                              int seg_jitter, int kpack_lat, int kpack_issue, int kpack_thin) {
    const bool short_chains = latency_bound && !seg_all && lat_short;
    ClassTable c;
    c.kpack = seg_all ? seg_all * 0x111111 : short_chains || (jittered && seg_jitter == 0) ? 0
            : latency_bound ? (lat_thin ? kpack_thin : kpack_lat) : kpack_issue;
    c.seg = seg_cap && c.kpack ? seg_cap : 0;
    if (!c.seg) c.kpack = 0;
    return c;
}

// Which of the two built orders launch n dispatches in (-1: none).  Eligible: a build the launch
// follows by >= 2 launches.  The newest built for okey; else the newest at the geometry `key`
// with its own class table -- but no segmented order for a launch that does not segment.
inline int pick_build(long long n, const long long build_at[2], const Geo build_key[2], const Geo &okey, const Geo &key) {
    int use = -1;
    for (int i = 0; i < 2; ++i) {
        if (build_at[i] < 0 || build_at[i] > n - 2) continue;
        if (build_key[i] == okey && (use < 0 || build_at[i] > build_at[use])) use = i;
    }
    if (use < 0) {   // none for this class table yet: the newest at this geometry, with its own table
        for (int i = 0; i < 2; ++i) {
            if (build_at[i] < 0 || build_at[i] > n - 2) continue;
            Geo g = build_key[i];
            if (g.seg && !okey.seg) continue;   // part entries only where this launch segments
            g.seg = g.kpack = 0;
            if (g == key && (use < 0 || build_at[i] > build_at[use])) use = i;
        }
    }
    return use;
}

// Whether a launch ran in an order of another class layout than the one it asked for (okey_*):
// seg / kmax / used_kpack are those of the order it dispatched in.
inline bool other_layout(bool enabled, bool has_order, int seg, int kmax, int used_kpack, int okey_seg, int okey_kmax,
                         int okey_kpack) {
    return enabled && has_order && (seg != okey_seg || (okey_seg && kmax != okey_kmax) || used_kpack != okey_kpack);
}

// Whether the order is rebuilt behind launch n (since_build: n - the launch of the last build).
inline bool needs_refresh(bool key_changed, uint64_t n, int order_every, bool drift, bool mode_changed, bool own_layout,
                          bool held_splat, bool view_changed, bool moving, uint64_t since_build, int move_every) {
    return key_changed || (n % order_every == 0 && drift) || mode_changed || own_layout || held_splat ||
           (view_changed && (!moving || since_build >= (uint64_t)move_every));
}

}  // namespace svo_sched
