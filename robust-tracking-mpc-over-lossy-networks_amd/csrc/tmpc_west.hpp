// Disturbance-set estimation (tmpc_west.hip): what tmpc_offline.cpp and the host execution model of tests/wavesim see of it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tmpc {

constexpr int WEST_NX = 4;               // the cart-pole: nx = 4, nu = 1
constexpr int WEST_DIGIT_BITS = 11;      // radix select: 2048 bins per pass
constexpr int WEST_BINS = 1 << WEST_DIGIT_BITS;
constexpr int WEST_PASSES = 6;           // 5 x 11 + 9 bits
constexpr int WEST_MAX_RANKS = 8;        // ranks of one column selected side by side (more: further groups)

// One closed loop u = -K x per trajectory on the RK4 cart-pole, the one-step prediction error w_k = x_k - Acl x_{k-1} of the linear model
// sampled at every period boundary k = 1 .. T - 1.
struct WestRollout {
    double Acl[WEST_NX * WEST_NX];       // A - B K, row-major
    double K[WEST_NX];
    double par[7];                       // M, m, b, I, g, l, Th (mcstep::cartpole_rhs)
    double lo[WEST_NX], hi[WEST_NX];     // box of the drawn initial states
    int substeps, T, draw;               // draw != 0: x0 from Philox4x64 with key (seed, first + b), counter 0
    int64_t n_traj, first;
    unsigned long long seed;
    const double *x0;                    // [n_traj][4]  (draw == 0)
    double *x0_used;                     // [n_traj][4]
    double *samples;                     // [4][T - 1][n_traj]
    double *xnorm;                       // [n_traj]  |x_T|_2
    unsigned long long *minmax;          // [8] order-preserving keys: min of the four components (start: all ones), max (start: 0)
    const double *par_traj;              // [n_traj][7] the cart-pole of every trajectory (tmpc_estimate_w_models), or nullptr: par
};

hipError_t launch_west_rollout(const WestRollout &a, hipStream_t stream);

// Exact order statistics of ncol columns of n doubles (column c starts at data + c * col_stride).  ranks: n_rank ranks (device memory),
// the same for every column.  out[c][r]: the value of rank r among the values of column c that are not NaN (NaN where there are
// fewer); nonfinite[c]: how many values of column c are NaN or +-inf.  ws: west_select_ws_words(ncol) words of scratch.
size_t west_select_ws_words(int ncol);
hipError_t launch_west_select(const double *data, int64_t n, int64_t col_stride, int ncol, int n_rank, const unsigned long long *ranks,
                              unsigned long long *ws, double *out, unsigned long long *nonfinite, hipStream_t stream);

// order-preserving map of a double's bits, and back (host and device)
__host__ __device__ inline unsigned long long west_key(unsigned long long u) { return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
__host__ __device__ inline unsigned long long west_unkey(unsigned long long k) { return (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k; }

}  // namespace tmpc
