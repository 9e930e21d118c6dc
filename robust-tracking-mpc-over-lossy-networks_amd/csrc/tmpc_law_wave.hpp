// The explicit law's arithmetic as one wavefront runs it: the test of the candidates of a table and the winner's output row.  Shared by
// law_kernel (tmpc_law.hip) and the fused closed loop through the law (closed_loop_law, tmpc_kernels.hip with FUSED = 3), which
// are compared by bytes (tests/test_law_loop_gpu.py): the same source, the same order of fused multiply-adds over q = 0 .. np-1 starting
// from the row's constant.  Included after the HIP runtime (or tests/wavesim/hip_sim.hpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "tmpc_law.hpp"

namespace tmpc {

__device__ inline bool law_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }          // (false for NaN)

// s + sum_q col[q stride] p[q], eight loads in flight at a time: one candidate's chunk is a chain of dependent fused multiply-adds behind
// loads that do not depend on each other, and issued one by one they cost an L2 round trip each
__device__ inline double law_dot(const double *col, int stride, const double *p, int np, double s) {
    int q = 0;
    for (; q + 8 <= np; q += 8, col += 8 * static_cast<size_t>(stride)) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = col[static_cast<size_t>(i) * stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fma(v[i], p[q + i], s);
    }
    if (q + 4 <= np) {
        double v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = col[static_cast<size_t>(i) * stride];
#pragma unroll
        for (int i = 0; i < 4; ++i) s = fma(v[i], p[q + i], s);
        q += 4;
        col += 4 * static_cast<size_t>(stride);
    }
    for (; q < np; ++q, col += stride) s = fma(*col, p[q], s);
    return s;
}

// The lowest row of region Sr ([np + 1][nrowp]) that fails at p, or -1 where every row holds.  The lanes take the rows 64 at a time and a
// ballot ends the test at the first chunk with a failing row (a NaN row fails).  Wave-uniform.
__device__ inline int law_fail_row(const double *Sr, int nrowp, int np, const double *p, int lane) {
    for (int base = 0; base < nrowp; base += 64) {
        const double *col = Sr + base + lane;
        double s = col[static_cast<size_t>(np) * nrowp];
        s = law_dot(col, nrowp, p, np, s);
        const unsigned long long fail = __ballot(!(s >= 0.0));
        if (fail != 0ull) return base + __builtin_ctzll(fail);
    }
    return -1;
}

// The id stored under key k in the open-addressed table slot [n_slot] (n_slot a power of two, at least half of it empty: -1), or -1
__device__ inline int law_lookup(const unsigned long long *key, const int32_t *slot, int n_slot, unsigned long long k) {
    const unsigned mask = static_cast<unsigned>(n_slot - 1);
    unsigned j = static_cast<unsigned>(k) & mask;
    for (int n = 0; n < n_slot; ++n, j = (j + 1u) & mask) {
        const int id = slot[j];
        if (id < 0) return -1;
        if (key[id] == k) return id;
    }
    return -1;
}

// How a chain of hops ended (LawHopEnd; the index of its counter among the six of include/tmpc.h, of which [1] counts the chain's tests)
constexpr int LAW_HOP_NONE = -1, LAW_HOP_HIT = 0, LAW_HOP_ABSENT = 2, LAW_HOP_CAP = 3, LAW_HOP_CYCLE = 4, LAW_HOP_PAR = 5;

// The region of the table t (a pointer to a LawTable, in whichever address space the caller reads it through: S [R][np + 1][nrowp], search
// order `order` [n_order], the keys and their hash) that holds p (in LDS, read as a broadcast), or -1, after
// at most max_tries candidates (<= 0: all); `tried` counts them.
//   The chain: it starts at the hint h where that is a valid id -- with max_hops > 0 otherwise at order[0].  The region is tested; where
// it fails and max_hops > 0, the search hops to the region across the facet of the LOWEST failing row i, found through the hash under
// key[r] ^ law_key_bit(i), and tests that one, and so on.  The chain ends at a parameter-only row (i >= nc), at a region without a key,
// at a neighbour the table does not hold, at the region it came from (a two-cycle), after max_hops hops, or at max_tries -- the
// conditions are looked at in this order, and chain_end names the first that held.
//   The walk: the search order without the chain's start.  Regions the chain has visited are tested again.
// max_hops = 0 is the hint, then the order without it.  Wave-uniform; all of the chain's state is scalar.
template <class Table>
__device__ inline int law_find(const Table t, int np, const double *p, int h, int max_tries, int lane, int &tried, int max_hops, int &chain_tests,
                               int &chain_end) {
    const double *const S = t->S;
    const int32_t *const order = t->order;
    const int R = t->R, n_order = t->n_order, nrowp = t->nrowp;
    const size_t rstride = static_cast<size_t>(np + 1) * nrowp;
    const bool hop = max_hops > 0 && t->key != nullptr && t->n_slot > 0;
    const int start = h >= 0 && h < R ? h : (max_hops > 0 && n_order > 0 ? order[0] : -1);
    tried = 0;
    chain_tests = 0;
    chain_end = LAW_HOP_NONE;
    if (start >= 0) {
        int r = start, prev = -1, hops = 0;
        for (;;) {
            ++tried;
            const int i = law_fail_row(S + static_cast<size_t>(r) * rstride, nrowp, np, p, lane);
            if (max_hops > 0) ++chain_tests;
            if (i < 0) {
                if (max_hops > 0) chain_end = LAW_HOP_HIT;
                return r;
            }
            if (max_hops <= 0) break;
            if (i >= t->nc) { chain_end = LAW_HOP_PAR; break; }
            if (!hop) break;
            const unsigned long long kr = t->key[r];
            if (kr == LAW_NO_KEY) break;
            const int nb = law_lookup(t->key, t->slot, t->n_slot, kr ^ law_key_bit(i));
            if (nb < 0 || nb >= R) { chain_end = LAW_HOP_ABSENT; break; }
            if (nb == prev) { chain_end = LAW_HOP_CYCLE; break; }
            if (hops == max_hops) { chain_end = LAW_HOP_CAP; break; }
            if (max_tries > 0 && tried == max_tries) break;
            prev = r;
            r = nb;
            ++hops;
        }
    }
    for (int c = 0; c < n_order && (max_tries <= 0 || tried < max_tries); ++c) {
        const int r = order[c];
        if (r == start) continue;
        ++tried;
        if (law_fail_row(S + static_cast<size_t>(r) * rstride, nrowp, np, p, lane) < 0) return r;
    }
    return -1;
}

// The chain's counters (stats [LAW_HOP_STATS], or NULL), by lane 0
__device__ inline void law_count_hops(unsigned long long *stats, int chain_tests, int chain_end) {
    if (!stats || chain_tests <= 0) return;
    atomicAdd(stats + 1, static_cast<unsigned long long>(chain_tests));
    if (chain_end >= 0) atomicAdd(stats + chain_end, 1ull);
}

// Entry j of y = Ky p + ky of region `win` (K [R][np + 1][ny])
__device__ inline double law_row(const double *K, int win, int ny, int np, const double *p, int j) {
    const double *col = K + static_cast<size_t>(win) * (np + 1) * ny + j;
    return law_dot(col, ny, p, np, col[static_cast<size_t>(np) * ny]);
}

}  // namespace tmpc
