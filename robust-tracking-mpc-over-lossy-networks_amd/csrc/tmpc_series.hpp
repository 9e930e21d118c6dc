// Ensemble statistics of the loops' per-step record (tmpc_series.hip): what tmpc_loops.cpp and the host execution model of tests/wavesim
// see of it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tmpc {

constexpr int SERIES_MAX_Q = 16;         // = TMPC_SER_MAX_Q
constexpr int SERIES_INT_TABLES = 10;    // n_alive, n_nan, lost_up, lost_down, adopted, tube, not_optimal, overrun, age_max, iters_max
constexpr int SERIES_LONG_TABLES = 2;    // age_sum, iters_sum
constexpr int SERIES_REAL_TABLES = 2;    // e_sum, e_max

// One reduction: column (t, g) = the entries [t][member[i]], start[g] <= i < start[g + 1], of the record e / word ([T][B], include/tmpc.h).
// All pointers are device pointers; every output table is written for every column.
struct SeriesStats {
    int64_t B;
    int T, G, n_q;
    const double *e;                     // [T][B]
    const uint32_t *word;                // [T][B]
    const int32_t *member;               // trajectories sorted by group (those in no group left out)
    const int32_t *start;                // [G + 1] first member of every group; start[G] = number of members
    const double *q;                     // [n_q] quantiles in [0, 1] (behind a pointer: an array inside the by-value kernel argument,
                                         // indexed by the thread, would be copied to private memory)
    int32_t *out_i;                      // [SERIES_INT_TABLES][T * G]
    int64_t *out_l;                      // [SERIES_LONG_TABLES][T * G]
    double *out_d;                       // [SERIES_REAL_TABLES][T * G]
    double *out_q;                       // [T * G][n_q]
};

hipError_t launch_series_stats(const SeriesStats &a, hipStream_t stream);

}  // namespace tmpc
