// Which tmpc_solve_batch_device calls of a handle may run side by side (tmpc_api.cpp: the two launch lanes): the byte ranges a
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

}  // namespace tmpc
