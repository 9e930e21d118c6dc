// The explicit control law on the device (gfx950; include/tmpc.h: tmpc_law_eval, tmpc_law_solve, tmpc_qp_law_eval).  Nothing is solved
// here: the minimiser of  min 1/2 z'Hz + (F p)'z  s.t.  G z <= g0 + Ebar p  is affine in p on each critical region, and a table of
// regions (tmpc_law.cpp builds them on the host from working sets the solver has produced) holds per region the polyhedron
// S p + s >= 0 -- primal slack of the rows outside the working set, multipliers of the rows inside, the parameter-only rows -- and the
// output map y = Ky p + ky.  A region whose polyhedron holds p satisfies the KKT conditions of the strictly convex QP at p: its y IS
// the minimiser's, whatever the table's history.
//
// One wavefront per instance, LAW_WAVES instances per workgroup, a fixed grid takes the instances round robin.  Per instance:
//
//   1  p is read a lane per entry and checked; it goes to the wave's LDS slice, from where every lane reads it as a broadcast;
//   2  the candidates: the hint when it is a valid id, then the search order without the hint, at most max_tries of them; with
//      max_hops > 0 a failed hint (or first entry of the order) hops to the region across its lowest failing row first, through a hash
//      of the working sets' keys (tmpc_law_wave.hpp: law_find);
//   3  per candidate the lanes take the rows 64 at a time -- S is stored [np + 1][nrowp], a row per lane, so that a wave reads
//      np + 1 runs of 512 contiguous bytes per chunk -- and a ballot rejects the candidate at the first chunk with a failing row;
//   4  the winner's y = Ky p + ky with the lanes over the rows of y (Ky stored [np + 1][ny] for the same reason), the nominal
//      trajectory rolled out from x_nom0 through LDS, one atomic add on the region's hit counter;
//   5  a miss marks the instance for the solve launches that follow (the selector byte of tmpc_solve_batch_device's kernels).
//
// No barrier: the waves of a workgroup share nothing.  All sizes are run-time values; no private arrays, no scratch
// (tests/test_explicit_law.py reads the code-object notes).  The kernel is bound by the L2 reads of (np + 1) nrowp doubles per
// candidate tried in full; a candidate that fails in its first chunk costs (np + 1) 512 bytes.
#ifdef TMPC_HOST_SIM
#include "hip_sim.hpp"      // tests/wavesim: this very source compiled for the CPU under sanitizers (never in the product)
#else
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "tmpc_device.hpp"
#include "tmpc_launch.hpp"
#include "tmpc_law.hpp"
#include "tmpc_law_wave.hpp"

namespace tmpc {

namespace {

constexpr int LAW_THREADS = 64 * LAW_WAVES;
constexpr int LAW_LDS_P = LAW_MAX_NP, LAW_LDS_U = LAW_MAX_NV, LAW_LDS_X = 2 * LAW_MAX_NX;
constexpr int LAW_LDS_WAVE = LAW_LDS_P + LAW_LDS_U + LAW_LDS_X;      // doubles of LDS per wave: p | u_nom | x_i, x_{i+1}

#ifdef TMPC_HOST_SIM
__device__ inline void law_lds_fence() { sim::wave_fence(); }
#else
// Orders one wave's LDS traffic for the compiler (the hardware runs the DS instructions of a wave in issue order).
__device__ inline void law_lds_fence() { asm volatile("" ::: "memory"); }
#endif

// Entry j of y = [Y0 | Y1 | Y2] of instance b
__device__ inline double *law_y(const LawArgs &a, int64_t b, int j) {
    if (j < a.ny0) return a.Y0 + b * a.ny0 + j;
    if (j < a.ny0 + a.ny1) return a.Y1 + b * a.ny1 + (j - a.ny0);
    return a.Y2 + b * (a.ny - a.ny0 - a.ny1) + (j - a.ny0 - a.ny1);
}

__device__ inline void law_fill_nan(const LawArgs &a, int64_t b, int lane) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int j = lane; j < a.ny; j += 64) *law_y(a, b, j) = nan;
    if (a.x_nom) {
        const int n = (a.N + 1) * a.nx;
        for (int j = lane; j < n; j += 64) a.x_nom[b * n + j] = nan;
    }
}

__global__ __launch_bounds__(LAW_THREADS) void law_kernel(const LawArgs a) {
#ifdef TMPC_HOST_SIM
    double *law_smem = sim::lds<double>();
#else
    extern __shared__ __attribute__((aligned(16))) double law_smem[];
#endif
    const int np = a.np, ny = a.ny;
    // (the wave index through readfirstlane: the compiler then knows that the instance, its table and the loops below are wave-uniform)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), nwave = blockDim.x >> 6;
    double *pv = law_smem + static_cast<size_t>(wave) * LAW_LDS_WAVE, *uv = pv + LAW_LDS_P, *xv = uv + LAW_LDS_U;

    for (int64_t b = static_cast<int64_t>(blockIdx.x) * nwave + wave; b < a.B; b += static_cast<int64_t>(gridDim.x) * nwave) {
        // ---- 1: inputs
        if (a.skip && a.skip[b]) {        // (a closed loop's trajectory that has stopped: nothing is evaluated, counted or solved)
            if (lane == 0 && a.todo) a.todo[b] = LAW_TODO_DONE;
            continue;
        }
        const int var = a.variant ? a.variant[b] : 0;
        double v = 0.0;
        if (lane < np) v = lane < a.np0 ? a.P0[b * a.np0 + lane] : a.P1[b * (np - a.np0) + (lane - a.np0)];
        const bool finite = __ballot(!law_finite(v)) == 0ull;
        const bool looped = a.acc_hits != nullptr;       // (a closed loop's step: a non-finite p is left to the solve as a miss)
        const bool refused = (!finite && !looped) || var >= a.nvariants;
        if (refused) {
            law_fill_nan(a, b, lane);
            if (lane == 0) {
                if (a.status) a.status[b] = TMPC_STATUS_NUMERICAL;
                if (a.iters) a.iters[b] = 0;
                a.region[b] = -1;
                if (a.tries) a.tries[b] = 0;
                if (a.todo) a.todo[b] = LAW_TODO_DONE;
            }
            continue;
        }
        law_lds_fence();                  // (the previous instance's reads of the slice are done)
        if (lane < np) pv[lane] = v;
        law_lds_fence();

        // ---- 2, 3: the candidates
        const LawTable t = a.t[var];
        const int h = a.hint ? a.hint[b] : -1;
        int tried = 0, chain_tests = 0, chain_end = LAW_HOP_NONE;
        const int win = finite ? law_find(&t, np, pv, h, a.max_tries, lane, tried, a.max_hops, chain_tests, chain_end) : -1;
        if (lane == 0 && a.max_hops > 0 && a.hop_stats) law_count_hops(a.hop_stats + var * LAW_HOP_STATS, chain_tests, chain_end);

        // ---- 5: a miss
        if (win < 0) {
            if (!a.fallback) law_fill_nan(a, b, lane);
            if (a.miss_n) {               // the log: the row's slot through the one counter, which counts on past the capacity
                unsigned long long slot = 0;
                if (lane == 0) slot = atomicAdd(a.miss_n, 1ull);
                const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(slot & 0xffffffffull)));
                const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(slot >> 32)));
                const long long at = static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
                if (at < a.miss_cap) {
                    if (lane < np) a.miss_p[at * np + lane] = v;
                    if (lane == 0) a.miss_var[at] = static_cast<uint8_t>(var);
                }
            }
            if (lane == 0) {
                if (!a.fallback) {
                    if (a.status) a.status[b] = TMPC_STATUS_NUMERICAL;
                    if (a.iters) a.iters[b] = 0;
                }
                a.region[b] = -1;
                if (a.tries) a.tries[b] = tried;
                if (a.acc_tries) a.acc_tries[b] += tried;
                if (a.todo) a.todo[b] = static_cast<uint8_t>(var);
            }
            continue;
        }

        // ---- 4: the winner's law
        for (int j = lane; j < ny; j += 64) {
            const double s = law_row(t.K, win, ny, np, pv, j);
            *law_y(a, b, j) = s;
            if (a.x_nom) {
                if (j < a.ny0) uv[j] = s;
                else if (j < a.ny0 + a.ny1) xv[j - a.ny0] = s;
            }
        }
        if (a.x_nom) {
            const int nx = a.nx, nu = a.nu;
            double *xn = a.x_nom + b * static_cast<int64_t>(a.N + 1) * nx;
            law_lds_fence();
            if (lane < nx) xn[lane] = xv[lane];
            for (int i = 0; i < a.N; ++i) {
                const double *xi = xv + (i & 1) * LAW_MAX_NX;
                double *xo = xv + ((i + 1) & 1) * LAW_MAX_NX;
                if (lane < nx) {
                    double s = 0.0;
#pragma unroll 1
                    for (int k = 0; k < nx; ++k) s = fma(a.A[lane * nx + k], xi[k], s);
#pragma unroll 1
                    for (int m = 0; m < nu; ++m) s = fma(a.Bm[lane * nu + m], uv[i * nu + m], s);
                    xo[lane] = s;
                    xn[static_cast<size_t>(i + 1) * nx + lane] = s;
                }
                law_lds_fence();
            }
        }
        if (lane == 0) {
            if (a.status) a.status[b] = TMPC_STATUS_OPTIMAL;
            if (a.iters) a.iters[b] = 0;
            a.region[b] = win;
            if (a.tries) a.tries[b] = tried;
            if (a.acc_tries) a.acc_tries[b] += tried;
            if (a.acc_hits) a.acc_hits[b] += 1;
            if (a.todo) a.todo[b] = LAW_TODO_DONE;
            if (t.hits) atomicAdd(t.hits + win, 1ull);
        }
    }
}

}  // namespace

// Workgroups of a launch over B instances on a card with n_cu compute units: at most eight per unit (32 waves, the kernel's registers allow it)
unsigned law_blocks(int64_t B, int n_cu) {
    const int64_t need = (B + LAW_WAVES - 1) / LAW_WAVES, cap = 8 * static_cast<int64_t>(n_cu > 0 ? n_cu : 1);
    return static_cast<unsigned>(need < 1 ? 1 : need < cap ? need : cap);
}

hipError_t launch_law(const LawArgs &a, unsigned blocks, hipStream_t stream) {
    if (a.np < 1 || a.np > LAW_MAX_NP || a.ny < 1 || a.ny > LAW_MAX_NY || a.B < 1 || blocks < 1 || a.nvariants < 1 || a.nvariants > 2 || !a.t || !a.region ||
        a.np0 < 0 || a.np0 > a.np || !a.P0 || (a.np0 < a.np && !a.P1) || a.max_hops < 0)
        return hipErrorInvalidValue;
    if (a.x_nom && (a.nx < 1 || a.nx > LAW_MAX_NX || a.nu < 1 || a.N < 1 || a.N * a.nu > LAW_MAX_NV || a.ny0 != a.N * a.nu || a.ny1 != a.nx || !a.A || !a.Bm))
        return hipErrorInvalidValue;
    return launch_grid(law_kernel, blocks, LAW_THREADS, static_cast<size_t>(LAW_WAVES) * LAW_LDS_WAVE * sizeof(double), stream, a);
}

}  // namespace tmpc
