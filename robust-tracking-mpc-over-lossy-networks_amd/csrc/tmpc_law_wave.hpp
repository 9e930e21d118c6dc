// The explicit law's arithmetic as one wavefront runs it: the test of the candidates of a table and the winner's output row.  Shared by
// law_kernel (tmpc_law.hip) and the fused closed loop through the law (closed_loop_law, tmpc_kernels.hip with FUSED = 3), which
// are compared by bytes (tests/test_law_loop_gpu.py): the same source, the same order of fused multiply-adds over q = 0 .. np-1 starting
// from the row's constant.  Included after the HIP runtime (or tests/wavesim/hip_sim.hpp).
#pragma once
#include <cstddef>
#include <cstdint>

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

// The region of the table (S [R][np + 1][nrowp], search order `order` [n_order]) that holds p (in LDS, read as a broadcast), or -1: the
// hint h first when it is a valid id, then the search order without it, at most max_tries candidates (<= 0: all).  The lanes take the
// rows 64 at a time and a ballot rejects a candidate at its first chunk with a failing row.  Wave-uniform; `tried` counts the candidates.
__device__ inline int law_find(const double *S, const int32_t *order, int R, int n_order, int nrowp, int np, const double *p, int h, int max_tries,
                               int lane, int &tried) {
    const bool hinted = h >= 0 && h < R;
    const size_t rstride = static_cast<size_t>(np + 1) * nrowp;
    tried = 0;
    for (int c = hinted ? -1 : 0; c < n_order && (max_tries <= 0 || tried < max_tries); ++c) {
        const int r = c < 0 ? h : order[c];
        if (c >= 0 && hinted && r == h) continue;
        ++tried;
        const double *Sr = S + static_cast<size_t>(r) * rstride;
        bool inside = true;
        for (int base = 0; base < nrowp; base += 64) {
            const double *col = Sr + base + lane;
            double s = col[static_cast<size_t>(np) * nrowp];
            s = law_dot(col, nrowp, p, np, s);
            if (__ballot(!(s >= 0.0)) != 0ull) { inside = false; break; }
        }
        if (inside) return r;
    }
    return -1;
}

// Entry j of y = Ky p + ky of region `win` (K [R][np + 1][ny])
__device__ inline double law_row(const double *K, int win, int ny, int np, const double *p, int j) {
    const double *col = K + static_cast<size_t>(win) * (np + 1) * ny + j;
    return law_dot(col, ny, p, np, col[static_cast<size_t>(np) * ny]);
}

}  // namespace tmpc
