// Which tmpc_solve_batch_device calls of a handle may run side by side (tmpc_api.cpp: the launch lanes): the byte ranges a
// call reads and writes, and the overlap predicate.  Plain C++, no HIP: tests/test_call_hazards.py drives it on the host
// through tmpc_debug_calls_conflict.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tmpc {

struct ByteRange {
    uintptr_t lo = 0, hi = 0;            // [lo, hi); lo == hi: nothing (a NULL optional pointer, B = 0)
};

// Half-open ranges: touching at a boundary is no overlap, and an empty range overlaps nothing -- not even a range it lies inside.
inline bool ranges_overlap(const ByteRange &a, const ByteRange &b) {
    return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi;
}

// What one call touches.  A solve call reads x_k, ref, variant and writes u_nom, x_nom0, xu_ss, x_nom, status, iters; a sensitivity call
// (tmpc_sens.cpp) reads eight arrays and writes four; an explicit-law call (tmpc_law.cpp) reads four and writes eight.  Unused slots are
// empty ranges.
struct CallRanges {
    static constexpr int NR = 8, NW = 8;
    ByteRange reads[NR], writes[NW];
    ByteRange hull;                      // covers every range above (empty: the call touches nothing)
};

inline ByteRange byte_range(const void *p, size_t bytes) {
    ByteRange r;
    if (p != nullptr && bytes != 0) { r.lo = reinterpret_cast<uintptr_t>(p); r.hi = r.lo + bytes; }
    return r;
}

// The ranges of tmpc_solve_batch_device(B, ...) on a problem with nx states, nu inputs and horizon N (include/tmpc.h has the
// sizes); a NULL pointer is an empty range.
inline CallRanges solve_call_ranges(int64_t B, int nx, int nu, int N, const void *x_k, const void *ref, const void *variant, const void *u_nom,
                                    const void *x_nom0, const void *xu_ss, const void *x_nom, const void *status, const void *iters) {
    const size_t b = B > 0 ? static_cast<size_t>(B) : 0, d = sizeof(double);
    CallRanges c;
    c.reads[0] = byte_range(x_k, b * nx * d);
    c.reads[1] = byte_range(ref, b * nx * d);
    c.reads[2] = byte_range(variant, b);
    c.writes[0] = byte_range(u_nom, b * N * nu * d);
    c.writes[1] = byte_range(x_nom0, b * nx * d);
    c.writes[2] = byte_range(xu_ss, b * (nx + nu) * d);
    c.writes[3] = byte_range(x_nom, b * (N + 1) * nx * d);
    c.writes[4] = byte_range(status, b * sizeof(int32_t));
    c.writes[5] = byte_range(iters, b * sizeof(int32_t));
    auto grow = [&c](const ByteRange &r) {
        if (r.lo >= r.hi) return;
        if (c.hull.lo >= c.hull.hi) { c.hull = r; return; }
        if (r.lo < c.hull.lo) c.hull.lo = r.lo;
        if (r.hi > c.hull.hi) c.hull.hi = r.hi;
    };
    for (const ByteRange &r : c.reads) grow(r);
    for (const ByteRange &r : c.writes) grow(r);
    return c;
}

// True when `later` must not run beside `earlier`: it reads what the earlier call writes (RAW), writes what it writes (WAW) or
// writes what it reads (WAR).  Two calls that only read the same bytes do not conflict.
inline bool calls_conflict(const CallRanges &earlier, const CallRanges &later) {
    if (!ranges_overlap(earlier.hull, later.hull)) return false;
    for (const ByteRange &w : earlier.writes) {
        for (const ByteRange &r : later.reads) if (ranges_overlap(w, r)) return true;
        for (const ByteRange &w2 : later.writes) if (ranges_overlap(w, w2)) return true;
    }
    for (const ByteRange &r : earlier.reads)
        for (const ByteRange &w2 : later.writes) if (ranges_overlap(r, w2)) return true;
    return false;
}

// ---- The launch lanes and the elastic grid: the policy, host code with no HIP in it (tmpc_api.cpp applies it to the handle's lanes;
// tests/test_elastic_policy.py drives it through tmpc_debug_plan_lanes, tmpc_debug_elastic_grid and tmpc_debug_busy_union).

constexpr int MAX_LANES = 4;             // TMPC_MAX_LANES of include/tmpc.h

// What the choice of a call's lane reads of every lane: whether it has been created, whether it holds unfinished calls, and
// whether one of those conflicts with the new call (calls_conflict).
struct LaneView {
    bool exists = false, busy = false, conflicts = false;
};
// The choice: the call's lane, whether that lane has to be created first, and the other lanes whose latest end event the call's
// lane waits for (a bit per lane).  A call with no such wait runs beside what the other lanes hold.
struct LanePick {
    int lane = 0;
    bool create = false;
    unsigned wait_mask = 0;
};

// The lane of a call, `cur` being the lane of the call before it and `lanes` (1 ... MAX_LANES) the lanes the handle may use.
//  - The call conflicts with unfinished calls of lane `cur`: it stays there, behind them.
//  - Otherwise it goes to the next lane in rotation order that holds a call it conflicts with, behind that call, or, with no conflict
//    at all, to the next lane of the rotation.  The rotation goes over the lanes in use: a lane that does not exist yet is
//    created when every existing lane holds unfinished work (there is something to run beside), else the rotation starts over at
//    lane 0.
//  - In both cases the chosen lane waits for every OTHER lane that holds a conflicting call.
// With lanes = 2 this is the rule of the two-lane handle.
inline LanePick pick_lane_policy(const LaneView *v, int lanes, int cur) {
    LanePick p;
    if (lanes <= 1) return p;
    if (cur < 0 || cur >= lanes) cur = 0;
    int target = -1;
    if (v[cur].exists && v[cur].conflicts) target = cur;
    for (int k = 1; k < lanes && target < 0; ++k) {
        const int l = (cur + k) % lanes;
        if (v[l].exists && v[l].conflicts) target = l;
    }
    if (target < 0) {
        target = (cur + 1) % lanes;
        if (!v[target].exists) {
            bool all_busy = true;
            for (int l = 0; l < lanes; ++l)
                if (v[l].exists && !v[l].busy) all_busy = false;
            if (all_busy) p.create = true;
            else target = target == 1 ? cur : 0;      // (the second lane of an idle handle: the call stays where it is)
        }
    }
    p.lane = target;
    for (int l = 0; l < lanes; ++l)
        if (l != target && v[l].exists && v[l].conflicts) p.wait_mask |= 1u << l;
    return p;
}

// Elastic grid of a wave-kernel launch: the POLICY only.  No launch uses it yet -- the kernel side that was built on it was taken out after a
// device fault whose cause was not found (DESIGN.md 5.1 "Between launches"); it is kept, and tested on the host, for whoever takes that up.
// The launch keeps n_cu workgroups; the first `core` of them take static first items and
// always work, the surplus ones read the launch's followers word once and leave when younger calls fill the card.
//  - core size: every lane but one can be expected to hold a younger call, so a launch is sure of n_cu / (lanes - 1) CUs
inline int elastic_core(int n_cu, int lanes) {
    if (n_cu < 1) return 1;
    if (lanes <= 2) return n_cu;
    return (n_cu + lanes - 2) / (lanes - 1);
}
//  - a launch is elastic when it has at least two items per resident wave (below that the grid rule is the one of a small batch) and
//    the handle runs no variant on the block kernel (such a handle keeps two lanes)
inline bool elastic_eligible(int64_t B, int n_cu, int wpb, bool block_variant) {
    return !block_variant && n_cu > 0 && wpb > 0 && B >= 2 * static_cast<int64_t>(n_cu) * wpb;
}
//  - the decision of a surplus workgroup: `followers` younger calls were enqueued beside this one while it was unfinished
inline bool surplus_yields(unsigned followers, int lanes) { return lanes >= 2 && followers >= static_cast<unsigned>(lanes - 1); }
//  - whose followers words a new call raises: those of the unfinished calls of every OTHER lane, when the new call's lane waits for
//    none of them (it runs beside them); a bit per lane
inline unsigned follower_lanes(const LanePick &p, const LaneView *v, int lanes) {
    unsigned m = 0;
    if (p.wait_mask != 0) return 0;
    for (int l = 0; l < lanes; ++l)
        if (l != p.lane && v[l].exists && v[l].busy) m |= 1u << l;
    return m;
}

// The handle's busy time (tmpc_kernel_ms_total): every call, in the order of the calls, adds the time by which it extended the busy
// period so far -- from the later of its own start and the end of the call that ended last among those before it (`busy`) to its own
// end.  own(i): end_i - start_i; past(j, i): end_i - end_j; lane(i): the call's lane.  Calls of one lane follow each other, so a call
// on the lane of `busy` adds its own time in full; a call of any other lane may have started before that end, on any number of lanes.
template <class Own, class Past, class LaneOf>
inline double busy_union(size_t n, Own own, Past past, LaneOf lane, bool *ok = nullptr) {
    double sum = 0.0;
    size_t busy = 0;
    if (ok) *ok = true;
    for (size_t i = 0; i < n; ++i) {
        double ms = 0.0;
        if (!own(i, &ms)) { if (ok) *ok = false; return sum; }
        if (i > 0 && lane(i) != lane(busy)) {
            double p = 0.0;
            if (!past(busy, i, &p)) { if (ok) *ok = false; return sum; }
            if (p <= 0.0) continue;          // ended inside the busy period: extends nothing
            if (p < ms) ms = p;
        }
        busy = i;
        sum += ms;
    }
    return sum;
}

}  // namespace tmpc
