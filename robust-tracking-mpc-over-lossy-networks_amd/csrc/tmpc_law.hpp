// The explicit control law (tmpc_law.hip): what tmpc_law.cpp and the kernel share.  include/tmpc.h has the entry points (tmpc_law_*,
// tmpc_qp_law_eval) and the meaning of a region.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tmpc {

// The limits of the sensitivity entries (tmpc_sens.hpp): a region is built from what they return
constexpr int LAW_MAX_NV = 128, LAW_MAX_NP = 32, LAW_MAX_NY = 4096, LAW_MAX_NC = 1 << 20;
constexpr int LAW_MAX_NX = LAW_MAX_NP / 2;       // a handle's p = [x_k | ref]

// The acceptance thresholds (include/tmpc.h: TMPC_LAW_FEAS_TOL, TMPC_LAW_MULT_TOL), compile-time constants shared with the numpy twin
// (LinearMPCOverNetworks/explicit_law.py).  A row of a region is accepted when its value is >= -tol; the host folds the tolerance
// into the row's constant, so the kernel compares with zero.  Both are absolute, on the unscaled rows of tmpc_get_condensed, and a
// tenth of the 1e-9 that the certificates of the solve's outputs allow on a primal residual and on a negative multiplier.
constexpr double LAW_FEAS_TOL = 1e-10;   // primal slack of a row outside the working set, and the parameter-only rows
constexpr double LAW_MULT_TOL = 1e-10;   // multiplier of a row of the working set

constexpr double LAW_RANK_TOL = 1e-13;   // a working set is refused when a diagonal entry of M's Cholesky factor is <= LAW_RANK_TOL times the largest

constexpr int LAW_WAVES = 4;             // instances per workgroup, one per wavefront
constexpr int LAW_TODO_DONE = 0xFF;      // selector byte of an instance that needs no solve

// The key of a working set is the XOR of law_key_bit(i) over its rows i (include/tmpc.h: splitmix64 of i + 1; the empty set has key 0), so
// the set across the facet of row i has the key of this one ^ law_key_bit(i), whichever side of it row i is on.
constexpr unsigned long long law_key_bit(int i) {
    unsigned long long x = (static_cast<unsigned long long>(i) + 1ull) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
constexpr unsigned long long LAW_NO_KEY = ~0ull;        // a region without a working set (a refused set of tmpc_qp_law_eval): no chain leaves it
constexpr int LAW_HOP_STATS = 6;         // counters per variant: chain hits, chain tests, chains ended by an absent neighbour / the cap / a two-cycle / a parameter-only row

// The regions of one problem variant on the device.  Row i of region r is  sum_q S[r][q][i] p_q + S[r][np][i] >= 0.
struct LawTable {
    int nrow = 0;            // nc + npar
    int nrowp = 0;           // nrow rounded up to 64; the padding rows are 0 p + 1
    int R = 0;               // regions stored
    int n_order = 0;         // length of the search order
    const double *S = nullptr;        // [R][np + 1][nrowp]
    const double *K = nullptr;        // [R][np + 1][ny]: y_j = sum_q K[r][q][j] p_q + K[r][np][j]
    const int32_t *order = nullptr;   // [n_order] region ids
    unsigned long long *hits = nullptr;       // [R] or NULL
    // the hops (LawArgs::max_hops): rows < nc belong to a working set's bit; the key of each region and the open-addressed table of ids
    // over them (-1: empty; n_slot the power of two >= max(64, 2 R), ids inserted in increasing order at key & (n_slot - 1), linear probing)
    int nc = 0;
    const unsigned long long *key = nullptr;  // [R] or NULL: no hops
    const int32_t *slot = nullptr;            // [n_slot]
    int n_slot = 0;
};

// One launch over B instances.  All pointers are device pointers.
struct LawArgs {
    int np, ny, nvariants;
    const LawTable *t;       // [nvariants], in device memory: the tables change between launches only, and the kernel reads the one of its instance
    int64_t B;
    int np0;                 // p = [P0[b][0..np0) | P1[b][0..np - np0)]
    const double *P0, *P1;
    const uint8_t *variant;  // or NULL
    const int32_t *hint;     // or NULL
    int max_tries;           // <= 0: all
    int ny0, ny1;            // y = [Y0[b][0..ny0) | Y1[b][0..ny1) | Y2[b][0..ny - ny0 - ny1)]
    double *Y0, *Y1, *Y2;
    // the nominal trajectory x_{i+1} = A x_i + Bm u_i from x_0 = Y1[b] with u = Y0[b] (ny0 = N nu, ny1 = nx), or x_nom == NULL
    double *x_nom;           // [B][N + 1][nx]
    const double *A, *Bm;    // [nx][nx], [nx][nu]
    int nx, nu, N;
    int32_t *status;         // [B] or NULL
    int32_t *iters;          // [B] or NULL
    int32_t *region;         // [B]
    int32_t *tries;          // [B] or NULL
    uint8_t *todo;           // [B] or NULL: the variant id of a miss, LAW_TODO_DONE otherwise
    int fallback;            // 1: a miss leaves y, x_nom, status and iters to the solve launches that follow
    // A closed loop's step (tmpc_mc_set_law; all NULL / 0 elsewhere): an instance with skip[b] != 0 (a trajectory that has stopped) is
    // passed over, a non-finite p is a miss like any other (the solve that follows gives its verdict as it does without the law),
    // hits and candidates add up per trajectory, and a miss appends its p and variant to the log through one counter.
    const uint8_t *skip;     // [B] or NULL
    int32_t *acc_hits;       // [B] or NULL
    long long *acc_tries;    // [B] or NULL
    unsigned long long *miss_n;       // one counter, or NULL: no log
    long long miss_cap;      // rows of the log; the counter goes on counting beyond
    double *miss_p;          // [miss_cap][np]
    uint8_t *miss_var;       // [miss_cap]
    int max_hops = 0;        // > 0: a failed hint (or order[0]) hops to the neighbour across its lowest failing row, at most so often (tmpc_law_wave.hpp)
    unsigned long long *hop_stats = nullptr;  // [nvariants][LAW_HOP_STATS] or NULL; touched with max_hops > 0 only
};

// What the fused closed loop (closed_loop_law, tmpc_fused_law.hip) reads of the law: in device memory, read through the constant
// address space like the loop's own record.  The tables are those of the handle at the start of the run.
struct LawLoop {
    LawTable t[2];
    int max_tries;           // <= 0: all
    int32_t *region;         // [B]: the hint of a step going in, its region coming out (-1: a miss)
    int32_t *hits;           // [B]
    long long *tries;        // [B]
    unsigned long long *miss_n;
    long long miss_cap;
    double *miss_p;          // [miss_cap][np]
    uint8_t *miss_var;       // [miss_cap]
    int max_hops = 0;        // as LawArgs
    unsigned long long *hop_stats = nullptr;  // [2][LAW_HOP_STATS] or NULL
};

unsigned law_blocks(int64_t B, int n_cu);
hipError_t launch_law(const LawArgs &a, unsigned blocks, hipStream_t stream);

}  // namespace tmpc
