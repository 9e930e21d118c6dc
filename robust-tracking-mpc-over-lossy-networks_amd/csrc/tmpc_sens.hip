// Sensitivity of the condensed QP's minimiser to its parameters (gfx950; include/tmpc.h: tmpc_sens_jacobian, tmpc_sens_vjp,
// tmpc_qp_sensitivity).  Nothing is solved here: the minimiser z of  min 1/2 z'Hz + (F p)'z  s.t.  G z <= g0 + Ebar p  is given, and
// on its critical region  z = -H^-1 (F p + G_A' lambda_A)  is affine in p, with  M = G_A H^-1 G_A',
//      lambda_A = -M^-1 (G_A H^-1 F p + g0_A + Ebar_A p),   dlambda/dp = -M^-1 (G_A H^-1 F + Ebar_A),   dz/dp = -H^-1 (F + G_A' dlambda/dp).
//
// One workgroup per instance (one wave up to nv = 32, four waves beyond), instances taken round robin by a fixed grid.  Per instance:
//
//   1  the inputs are checked (status, finite), z is rebuilt from the solve's outputs where the caller is a handle (z = Rec [y | p]);
//   2  the rows are scanned in ascending order, a thread per row and blockDim rows at a time (from transposed copies of G and Ebar, so that the
//      threads of a wave read neighbouring words): slack_i = g0_i + Ebar_i p - G_i z; the rows
//      with slack <= act_tol are the candidates -- a ballot per wave, the masks in LDS, so that every thread walks the same candidates in
//      row order.  No list of candidates is kept: their number is not limited by registers or by LDS;
//   3  each candidate i goes through one step of the row-by-row Cholesky factorisation of M: its row of M against the k rows kept so
//      far, m_j = W_i . G_aj (W = G H^-1, from the host) and m_k = W_i . G_i, then l = L^-1 m and the pivot d = m_k - l'l.  A candidate
//      with d <= SENS_RANK_TOL m_k (or one that arrives when nv rows are kept: it cannot be independent) is dropped and the instance
//      flagged DEPENDENT; otherwise it becomes row k of the working set.  What LDS keeps is L^-1 ([k][k], lower triangular, at most
//      128 x 129 doubles = 129 KB of the 160 KB), extended by the row  [-l'L^-1 | 1] / sqrt(d): the triangular solve of the NEXT candidate
//      is then a matrix-vector product, a thread per row with no dependence between them, and every product with M^-1 = L^-T L^-1
//      further down is two of those.  Three barriers per candidate;
//   4  multipliers and flags: lambda = -L^-T L^-1 c,  WEAK, NOT_KKT (stationarity of the GIVEN z on this working set);
//   5  forward mode: the np columns  C = W_A F + Ebar_A,  D = -L^-T L^-1 C,  dz = -H^-1 F - W_A' D,  J = Y dz + Yp -- the blocks C, D, dz
//      ([nv][np] each) live in a slice of device workspace per workgroup (L2), every entry written by one thread and read after a
//      barrier;  reverse mode: one column through the same system,  v = Y'ybar,  q = L^-T L^-1 (W_A v),  pbar = Yp'ybar - F'(H^-1 v - W_A' q)
//      + Ebar_A' q, all in LDS.
//
// The GEMM-shaped products of the forward mode -- the right-hand-side block C = W_A F + Ebar_A, dz and J -- run on v_mfma_f64_16x16x4_f64
// where nv >= 16 (sens_gemm_mfma below) and on plain FMA below that.  The rows of M are formed one candidate at a time against the rows KEPT so far, which
// the previous pivot decides: matrix-vector products, plain FMA.
// No private arrays, no scratch (tests/test_sensitivity.py reads the code-object notes).
#ifdef TMPC_HOST_SIM
#include "hip_sim.hpp"      // tests/wavesim: this very source compiled for the CPU under sanitizers (never in the product)
#else
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "tmpc_device.hpp"
#include "tmpc_launch.hpp"
#include "tmpc_sens.hpp"

namespace tmpc {

namespace {

constexpr int SENS_MAX_THREADS = 256;

__device__ inline bool sens_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }        // (false for NaN)

// The GEMM-shaped products of the forward mode on the FP64 matrix cores (v_mfma_f64_16x16x4_f64) where nv >= 16 -- the right-hand-side
// block  C = W_A F + Ebar_A  (k x nv by nv x np),  dz = -H^-1 F - W_A' D  (nv x k by k x np)  and  J = Yp + Y dz  (ny x nv by nv x np):
// a wave per 16 x 16 tile of the result, the tiles dealt round robin to the workgroup's waves, K / 4 instructions per tile.
// A operand (16 x 4 per step): lane l holds A[i0 + l % 16][4 ks + l / 16]; B operand (4 x 16): lane l holds B[4 ks + l / 16][j0 + l % 16];
// C/D: lane l holds rows (l / 16) + 4 reg, column l % 16 of the tile (the layout tmpc_kernels.hip and tmpc_block.hip use).  The operands
// come straight from device memory, one f64 per lane and step; rows past M, columns past N and the tail of K are zeros in the loads
// and never stored.  Control flow is uniform per wave: every lane issues every instruction.
constexpr int SENS_MFMA_MIN_NV = 16;
typedef double sens_v4d __attribute__((ext_vector_type(4)));
template <class FA, class FB, class FS>
__device__ inline void sens_gemm_mfma(int M, int N, int K, int tid, int nt, FA A, FB B, FS store) {
    const int lane = tid & 63, wave = tid >> 6, nwave = nt >> 6;
    const int tj = (N + 15) / 16, ntile = ((M + 15) / 16) * tj;
    for (int t = wave; t < ntile; t += nwave) {
        const int i0 = (t / tj) * 16, j0 = (t - (t / tj) * tj) * 16;
        const int ar = i0 + (lane & 15), bc = j0 + (lane & 15), kk = lane >> 4;
        sens_v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
        for (int c0 = 0; c0 < K; c0 += 4) {
            const int c = c0 + kk;
            const double av = (ar < M && c < K) ? A(ar, c) : 0.0;
            const double bv = (bc < N && c < K) ? B(c, bc) : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = i0 + (lane >> 4) + 4 * reg, col = j0 + (lane & 15);
            if (row < M && col < N) store(row, col, acc[reg]);
        }
    }
}

// (four waves per SIMD: the register budget of 128 that tests/test_sensitivity.py holds the kernel to)
__global__ __launch_bounds__(SENS_MAX_THREADS, 4) void sens_kernel(const SensArgs a) {
#ifdef TMPC_HOST_SIM
    double *sens_smem = sim::lds<double>();
#else
    extern __shared__ __attribute__((aligned(16))) double sens_smem[];
#endif
    const int nv = a.nv, nc = a.nc, np = a.np, ny = a.ny, ld = nv | 1;
    const int tid = threadIdx.x, nt = blockDim.x, nwave = nt >> 6;
    // LDS: L^-1 [nv][ld]; ten vectors of nv + 1; p; the ballot masks; the working set; one word for block-wide decisions
    double *Li = sens_smem;
    double *wi = Li + static_cast<size_t>(nv) * ld;
    double *mv = wi + (nv + 1), *lv = mv + (nv + 1), *fv = lv + (nv + 1), *zv = fv + (nv + 1), *lam = zv + (nv + 1), *tv = lam + (nv + 1),
           *av = tv + (nv + 1), *bv = av + (nv + 1), *vv = bv + (nv + 1);
    double *pv = vv + (nv + 1);
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(pv + np);
    int *alist = reinterpret_cast<int *>(masks + 4);
    int *sbad = alist + nv;
    const int nzin = a.Rec ? a.nz0 + a.nz1 + a.nz2 : nv;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const size_t nout = a.mode == SENS_MODE_VJP ? static_cast<size_t>(np) : static_cast<size_t>(ny) * np;
    double *wsC = a.ws ? a.ws + static_cast<size_t>(blockIdx.x) * 2 * nv * np : nullptr, *wsT = wsC ? wsC + static_cast<size_t>(nv) * np : nullptr;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int var = a.variant ? a.variant[b] : 0;
        const bool bad_variant = var >= a.nvariants;
        if (bad_variant ? a.my_variant != 0 : var != a.my_variant) continue;          // (uniform: another launch writes this instance)
        double *out = a.out + static_cast<size_t>(b) * nout;
        uint32_t *act = a.active ? a.active + static_cast<size_t>(b) * a.nwords : nullptr;

        // ---- 1: inputs
        if (tid == 0) sbad[0] = (bad_variant || (a.status && a.status[b] >= TMPC_STATUS_INFEASIBLE)) ? 1 : 0;
        __syncthreads();
        bool bad = false;
        for (int i = tid; i < np; i += nt) {
            const double v = i < a.np0 ? a.P0[b * a.np0 + i] : a.P1[b * (np - a.np0) + (i - a.np0)];
            pv[i] = v;
            bad |= !sens_finite(v);
        }
        for (int i = tid; i < nzin; i += nt) {
            const double v = i < a.nz0 ? a.Z0[b * a.nz0 + i] : i < a.nz0 + a.nz1 ? a.Z1[b * a.nz1 + (i - a.nz0)] : a.Z2[b * a.nz2 + (i - a.nz0 - a.nz1)];
            if (!a.Rec) zv[i] = v;
            bad |= !sens_finite(v);
        }
        if (a.mode == SENS_MODE_VJP)
            for (int i = tid; i < ny; i += nt) bad |= !sens_finite(a.ybar[b * ny + i]);
        if (bad) sbad[0] = 1;
        __syncthreads();
        if (sbad[0]) {
            for (size_t i = tid; i < nout; i += nt) out[i] = nan;
            for (int w = tid; act && w < a.nwords; w += nt) act[w] = 0u;
            for (int c = tid; c < nv; c += nt) {             // (nothing of this instance enters the sums of sens_wgrad)
                if (a.adj) a.adj[static_cast<size_t>(b) * nv + c] = 0.0;
                if (a.zrec) a.zrec[static_cast<size_t>(b) * nv + c] = 0.0;
            }
            if (tid == 0) { a.flag[b] = TMPC_SENS_SKIPPED; a.n_active[b] = 0; }
            __syncthreads();
            continue;
        }
        if (a.Rec) {
            const int nin = nzin + np;
            for (int c = tid; c < nv; c += nt) {
                const double *R = a.Rec + static_cast<size_t>(c) * nin;
                double s = 0.0;
                for (int i = 0; i < a.nz0; ++i) s += R[i] * a.Z0[b * a.nz0 + i];
                for (int i = 0; i < a.nz1; ++i) s += R[a.nz0 + i] * a.Z1[b * a.nz1 + i];
                for (int i = 0; i < a.nz2; ++i) s += R[a.nz0 + a.nz1 + i] * a.Z2[b * a.nz2 + i];
                for (int i = 0; i < np; ++i) s += R[nzin + i] * pv[i];
                zv[c] = s;
            }
            __syncthreads();
        }

        // ---- 2, 3: candidates in row order through the factorisation
        int k = 0, flag = 0;
        for (int base = 0; base < nc; base += nt) {
            const int row = base + tid;
            bool cand = false;
            if (row < nc) {
                double s = a.g0[row];
                for (int i = 0; i < np; ++i) s += a.EbarT[static_cast<size_t>(i) * nc + row] * pv[i];
                for (int c = 0; c < nv; ++c) s -= a.Gt[static_cast<size_t>(c) * nc + row] * zv[c];
                cand = s <= a.act_tol;
            }
            const unsigned long long m = __ballot(cand);
            if ((tid & 63) == 0) masks[tid >> 6] = m;
            __syncthreads();
            for (int w = 0; w < nwave; ++w) {
                unsigned long long mask = masks[w];
                while (mask) {
                    const int i = base + w * 64 + __builtin_ctzll(mask);
                    mask &= mask - 1;
                    if (k >= nv) { flag |= TMPC_SENS_DEPENDENT; continue; }
                    const double *Wi = a.W + static_cast<size_t>(i) * nv;
                    for (int c = tid; c < nv; c += nt) wi[c] = Wi[c];
                    __syncthreads();
                    if (tid <= k) {
                        const double *Gr = a.G + static_cast<size_t>(tid < k ? alist[tid] : i) * nv;
                        double s = 0.0;
                        for (int c = 0; c < nv; ++c) s += wi[c] * Gr[c];
                        mv[tid] = s;
                    }
                    __syncthreads();
                    if (tid < k) {
                        double s = 0.0;
                        for (int t = 0; t <= tid; ++t) s += Li[tid * ld + t] * mv[t];
                        lv[tid] = s;
                    }
                    __syncthreads();
                    const double mkk = mv[k];
                    double d = mkk;
                    for (int j = 0; j < k; ++j) d -= lv[j] * lv[j];
                    if (!(d > SENS_RANK_TOL * mkk)) { flag |= TMPC_SENS_DEPENDENT; continue; }        // (the next step's first barrier orders its writes behind these reads)
                    const double r = 1.0 / sqrt(d);
                    if (tid < k) {
                        double s = 0.0;
                        for (int j = tid; j < k; ++j) s += lv[j] * Li[j * ld + tid];
                        Li[k * ld + tid] = -r * s;
                    } else if (tid == k) {
                        Li[k * ld + k] = r;
                        alist[k] = i;
                    }
                    ++k;
                    __syncthreads();
                }
            }
            __syncthreads();              // (the masks are read: the next chunk may write them)
        }

        // ---- 4: multipliers and flags
        for (int c = tid; c < nv; c += nt) {
            double s = 0.0;
            for (int i = 0; i < np; ++i) s += a.F[static_cast<size_t>(c) * np + i] * pv[i];
            fv[c] = s;
        }
        __syncthreads();
        double fnorm = 0.0;
        for (int c = 0; c < nv; ++c) fnorm = fmax(fnorm, fabs(fv[c]));
        const double thr = SENS_KKT_TOL * (1.0 + fnorm);
        if (tid < k) {
            const int r = alist[tid];
            const double *Wr = a.W + static_cast<size_t>(r) * nv, *E = a.Ebar + static_cast<size_t>(r) * np;
            double s = a.g0[r];
            for (int i = 0; i < np; ++i) s += E[i] * pv[i];
            for (int c = 0; c < nv; ++c) s += Wr[c] * fv[c];
            tv[tid] = s;
        }
        __syncthreads();
        if (tid < k) {
            double s = 0.0;
            for (int t = 0; t <= tid; ++t) s += Li[tid * ld + t] * tv[t];
            av[tid] = s;
        }
        __syncthreads();
        if (tid < k) {
            double s = 0.0;
            for (int t = tid; t < k; ++t) s += Li[t * ld + tid] * av[t];
            lam[tid] = -s;
        }
        __syncthreads();
        if (k > 0) {
            double linf = 0.0, lmin = lam[0];
            for (int j = 0; j < k; ++j) { linf = fmax(linf, fabs(lam[j])); lmin = fmin(lmin, lam[j]); }
            if (lmin <= SENS_MULT_TOL * fmax(1.0, linf)) flag |= TMPC_SENS_WEAK;
            if (lmin < -thr) flag |= TMPC_SENS_NOT_KKT;
        }
        for (int c = tid; c < nv; c += nt) {
            double s = fv[c];
            const double *Hr = a.H + static_cast<size_t>(c) * nv;
            for (int j = 0; j < nv; ++j) s += Hr[j] * zv[j];
            for (int j = 0; j < k; ++j) s += a.G[static_cast<size_t>(alist[j]) * nv + c] * lam[j];
            bv[c] = fabs(s);
        }
        __syncthreads();
        {
            double res = 0.0;
            for (int c = 0; c < nv; ++c) res = fmax(res, bv[c]);
            if (!(res <= thr)) flag |= TMPC_SENS_NOT_KKT;
        }
        __syncthreads();                  // (bv is reused below)

        // ---- 5
        if (a.mode == SENS_MODE_JACOBIAN) {
            if (nv >= SENS_MFMA_MIN_NV) {
                sens_gemm_mfma(k, np, nv, tid, nt, [&](int i, int c) { return a.W[static_cast<size_t>(alist[i]) * nv + c]; },
                               [&](int c, int q) { return a.F[static_cast<size_t>(c) * np + q]; },
                               [&](int i, int q, double v) { wsC[i * np + q] = v + a.Ebar[static_cast<size_t>(alist[i]) * np + q]; });
            } else {
                for (int idx = tid; idx < k * np; idx += nt) {
                    const int j = idx / np, q = idx - j * np, r = alist[j];
                    const double *Wr = a.W + static_cast<size_t>(r) * nv;
                    double s = a.Ebar[static_cast<size_t>(r) * np + q];
                    for (int c = 0; c < nv; ++c) s += Wr[c] * a.F[static_cast<size_t>(c) * np + q];
                    wsC[idx] = s;
                }
            }
            __syncthreads();
            for (int idx = tid; idx < k * np; idx += nt) {
                const int j = idx / np, q = idx - j * np;
                double s = 0.0;
                for (int t = 0; t <= j; ++t) s += Li[j * ld + t] * wsC[t * np + q];
                wsT[idx] = s;
            }
            __syncthreads();
            for (int idx = tid; idx < k * np; idx += nt) {
                const int j = idx / np, q = idx - j * np;
                double s = 0.0;
                for (int t = j; t < k; ++t) s += Li[t * ld + j] * wsT[t * np + q];
                wsC[idx] = -s;            // D = dlambda/dp
            }
            __syncthreads();
            if (nv >= SENS_MFMA_MIN_NV) {
                sens_gemm_mfma(nv, np, k, tid, nt, [&](int c, int j) { return a.W[static_cast<size_t>(alist[j]) * nv + c]; },
                               [&](int j, int q) { return wsC[j * np + q]; },
                               [&](int c, int q, double v) { wsT[c * np + q] = -a.HinvF[c * np + q] - v; });       // dz/dp
                __syncthreads();
                sens_gemm_mfma(ny, np, nv, tid, nt, [&](int y, int c) { return a.Y[static_cast<size_t>(y) * nv + c]; },
                               [&](int c, int q) { return wsT[c * np + q]; },
                               [&](int y, int q, double v) { out[y * np + q] = a.Yp[y * np + q] + v; });
            } else {
                for (int idx = tid; idx < nv * np; idx += nt) {
                    const int c = idx / np, q = idx - c * np;
                    double s = -a.HinvF[idx];
                    for (int j = 0; j < k; ++j) s -= a.W[static_cast<size_t>(alist[j]) * nv + c] * wsC[j * np + q];
                    wsT[idx] = s;         // dz/dp
                }
                __syncthreads();
                for (int idx = tid; idx < ny * np; idx += nt) {
                    const int y = idx / np, q = idx - y * np;
                    const double *Yr = a.Y + static_cast<size_t>(y) * nv;
                    double s = a.Yp[idx];
                    for (int c = 0; c < nv; ++c) s += Yr[c] * wsT[c * np + q];
                    out[idx] = s;
                }
            }
        } else {
            const double *yb = a.ybar + static_cast<size_t>(b) * ny;
            for (int c = tid; c < nv; c += nt) {
                double s = 0.0;
                for (int y = 0; y < ny; ++y) s += a.Y[static_cast<size_t>(y) * nv + c] * yb[y];
                vv[c] = s;
            }
            __syncthreads();
            if (tid < k) {
                const double *Wr = a.W + static_cast<size_t>(alist[tid]) * nv;
                double s = 0.0;
                for (int c = 0; c < nv; ++c) s += Wr[c] * vv[c];
                tv[tid] = s;
            }
            __syncthreads();
            if (tid < k) {
                double s = 0.0;
                for (int t = 0; t <= tid; ++t) s += Li[tid * ld + t] * tv[t];
                av[tid] = s;
            }
            __syncthreads();
            if (tid < k) {
                double s = 0.0;
                for (int t = tid; t < k; ++t) s += Li[t * ld + tid] * av[t];
                lam[tid] = s;             // q
            }
            __syncthreads();
            for (int c = tid; c < nv; c += nt) {
                const double *Hr = a.Hinv + static_cast<size_t>(c) * nv;
                double s = 0.0;
                for (int j = 0; j < nv; ++j) s += Hr[j] * vv[j];
                for (int j = 0; j < k; ++j) s -= a.W[static_cast<size_t>(alist[j]) * nv + c] * lam[j];
                bv[c] = s;
                if (a.zrec) a.zrec[static_cast<size_t>(b) * nv + c] = zv[c];
            }
            __syncthreads();
            for (int q = tid; q < np; q += nt) {
                double s = 0.0;
                for (int y = 0; y < ny; ++y) s += a.Yp[static_cast<size_t>(y) * np + q] * yb[y];
                for (int c = 0; c < nv; ++c) s -= a.F[static_cast<size_t>(c) * np + q] * bv[c];
                for (int j = 0; j < k; ++j) s += a.Ebar[static_cast<size_t>(alist[j]) * np + q] * lam[j];
                out[q] = s;
            }
            if (a.adj) {
                // a_b for the weight gradients: bv after one step of refinement on the constraint rows.  The exact a has G_A a = 0;
                // bv is the rounded difference of two terms, and what it leaves in G_A bv is taken out through the same factor,
                // a = bv - W_A' M^-1 (G_A bv).  (With |A| = nv the exact a is zero and bv is rounding alone.)  pbar above used bv and is untouched.
                if (tid < k) {
                    const double *Gr = a.G + static_cast<size_t>(alist[tid]) * nv;
                    double s = 0.0;
                    for (int c = 0; c < nv; ++c) s += Gr[c] * bv[c];
                    tv[tid] = s;
                }
                __syncthreads();
                if (tid < k) {
                    double s = 0.0;
                    for (int t = 0; t <= tid; ++t) s += Li[tid * ld + t] * tv[t];
                    av[tid] = s;
                }
                __syncthreads();
                if (tid < k) {
                    double s = 0.0;
                    for (int t = tid; t < k; ++t) s += Li[t * ld + tid] * av[t];
                    mv[tid] = s;
                }
                __syncthreads();
                for (int c = tid; c < nv; c += nt) {
                    double s = bv[c];
                    for (int j = 0; j < k; ++j) s -= a.W[static_cast<size_t>(alist[j]) * nv + c] * mv[j];
                    a.adj[static_cast<size_t>(b) * nv + c] = s;
                }
            }
        }
        for (int w = tid; act && w < a.nwords; w += nt) {
            uint32_t word = 0u;
            for (int j = 0; j < k; ++j)
                if ((alist[j] >> 5) == w) word |= 1u << (alist[j] & 31);
            act[w] = word;
        }
        if (tid == 0) { a.flag[b] = flag; a.n_active[b] = k; }
        __syncthreads();                  // (LDS and the workspace slice go to the next instance)
    }
}

// The batch reduction of the weight gradients, first kernel (tmpc_sens.hpp: SensWgradArgs): C = A' Z with A = adj [B][nv] and
// Z = [zrec | p] [B][nv + np], the inner dimension the batch.  A wave per 16 x 16 tile of C and chunk of SENS_WG_CHUNK instances, the
// operand layout of sens_gemm_mfma: lane l holds adj[b0 + 4 s + l / 16][i0 + l % 16] and Z[b0 + 4 s + l / 16][j0 + l % 16], so the sixteen
// lanes of a quarter read sixteen consecutive doubles of one row.  Rows past nv, columns past nv + np, instances past B, of another
// variant or SKIPPED are zeros in the loads; nothing outside C is stored.  One partial tile per (chunk, tile) in `part`: no atomics.
__global__ __launch_bounds__(64) void sens_wgrad_partial_kernel(const SensWgradArgs a) {
    const int nv = a.nv, np = a.np, N = nv + np, lane = threadIdx.x & 63;
    const int tj = (N + 15) / 16, ntile = ((nv + 15) / 16) * tj;
    const int64_t nwork = static_cast<int64_t>((a.B + SENS_WG_CHUNK - 1) / SENS_WG_CHUNK) * ntile;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t chunk = w / ntile, b0 = chunk * SENS_WG_CHUNK;
        const int t = static_cast<int>(w - chunk * ntile);
        const int i0 = (t / tj) * 16, j0 = (t - (t / tj) * tj) * 16;
        const int ar = i0 + (lane & 15), bc = j0 + (lane & 15), kk = lane >> 4;
        const int steps = static_cast<int>(a.B - b0 < SENS_WG_CHUNK ? a.B - b0 : SENS_WG_CHUNK);      // (uniform)
        sens_v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int s0 = 0; s0 < steps; s0 += 4) {
            const int64_t b = b0 + s0 + kk;
            bool live = s0 + kk < steps;
            if (live) {
                const int var = a.variant ? a.variant[b] : 0;
                live = (var >= a.nvariants ? a.my_variant == 0 : var == a.my_variant) && !(a.flag[b] & TMPC_SENS_SKIPPED);
            }
            double av = 0.0, zv = 0.0;
            if (live && ar < nv) av = a.adj[b * nv + ar];
            if (live && bc < N) {
                const int q = bc - nv;
                zv = q < 0 ? a.zrec[b * nv + bc] : q < a.np0 ? a.P0[b * a.np0 + q] : a.P1[b * (np - a.np0) + (q - a.np0)];
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, zv, acc, 0, 0, 0);
        }
        double *part = a.part + static_cast<size_t>(chunk) * nv * N;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = i0 + (lane >> 4) + 4 * reg, col = j0 + (lane & 15);
            if (row < nv && col < N) part[static_cast<size_t>(row) * N + col] = acc[reg];
        }
    }
}

// Second kernel: a thread per entry of C adds its partials in chunk order.  Hbar(i, j) takes the sums of C(i, j) and C(j, i), whose
// sum is the same number in either order: Hbar is symmetric to the bit.
__global__ __launch_bounds__(SENS_MAX_THREADS) void sens_wgrad_sum_kernel(const SensWgradArgs a) {
    const int nv = a.nv, np = a.np, N = nv + np;
    const size_t nchunk = static_cast<size_t>((a.B + SENS_WG_CHUNK - 1) / SENS_WG_CHUNK), tile = static_cast<size_t>(nv) * N;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nv * N; idx += gridDim.x * blockDim.x) {
        const int i = idx / N, j = idx - i * N;
        double s = 0.0, st = 0.0;
        for (size_t c = 0; c < nchunk; ++c) s += a.part[c * tile + idx];
        if (j < nv) {
            for (size_t c = 0; c < nchunk; ++c) st += a.part[c * tile + static_cast<size_t>(j) * N + i];
            a.Hbar[i * nv + j] = -0.5 * (s + st);
        } else {
            a.Fbar[i * np + (j - nv)] = -s;
        }
    }
}

}  // namespace

int sens_threads(int nv) { return nv <= 32 ? 64 : SENS_MAX_THREADS; }

size_t sens_lds_bytes(int nv, int np) {
    const size_t words = static_cast<size_t>(nv) * (nv | 1) + 10 * static_cast<size_t>(nv + 1) + static_cast<size_t>(np) + 4;
    return words * 8 + (static_cast<size_t>(nv) + 2) * 4;
}

hipError_t launch_sens(const SensArgs &a, unsigned blocks, hipStream_t stream) {
    if (a.nv < 1 || a.nv > SENS_MAX_NV || a.nc < 0 || a.nc > SENS_MAX_NC || a.np < 1 || a.np > SENS_MAX_NP || a.ny < 1 || a.ny > SENS_MAX_NY || a.B < 1 ||
        blocks < 1 || !a.out || !a.flag || !a.n_active || (a.mode == SENS_MODE_JACOBIAN && !a.ws) || (a.mode == SENS_MODE_VJP && !a.ybar))
        return hipErrorInvalidValue;
    return launch_grid(sens_kernel, blocks, static_cast<unsigned>(sens_threads(a.nv)), sens_lds_bytes(a.nv, a.np), stream, a);
}

hipError_t launch_sens_wgrad(const SensWgradArgs &a, unsigned blocks, hipStream_t stream) {
    if (a.nv < 1 || a.nv > SENS_MAX_NV || a.np < 1 || a.np > SENS_MAX_NP || a.np0 < 0 || a.np0 > a.np || a.B < 1 || blocks < 1 || !a.adj || !a.zrec || !a.P0 ||
        (a.np0 < a.np && !a.P1) || !a.flag || !a.part || !a.Hbar || !a.Fbar)
        return hipErrorInvalidValue;
    if (const hipError_t e = launch_grid(sens_wgrad_partial_kernel, blocks, 64u, 0, stream, a); e != hipSuccess) return e;
    const unsigned entries = static_cast<unsigned>(a.nv * (a.nv + a.np));
    return launch_grid(sens_wgrad_sum_kernel, (entries + SENS_MAX_THREADS - 1) / SENS_MAX_THREADS, static_cast<unsigned>(SENS_MAX_THREADS), 0, stream, a);
}

}  // namespace tmpc
