// TEST INFRASTRUCTURE (not product code): a device probe of v_mfma_f64_4x4x4_4b_f64 and of the pass built on it, wv::mfma_blocks and
// wv::gdg_blocks of csrc/tmpc_wave.hpp, behind plain C entry points for ctypes (tests/test_mfma_blocks_gpu.py,
// scripts/gpu_mfma_blocks.py).  csrc/Makefile builds it with the product's flags as lib/libtmpc_mfmablocks.so; nothing of the
// product but tmpc_wave.hpp is included, and the product library links none of this.
//
//   mfmablocks_raw    one instruction per problem on operands the caller lays out lane by lane: the lane maps are read off
//                     index-coded operands on the host
//   mfmablocks_time   s_memtime around 512 matrix instructions of one wave in one workgroup: chains of the block instruction on
//                     two and on four alternating accumulators and on one (dependent), and the same of v_mfma_f64_16x16x4_f64
//   mfmablocks_gdg    [(D.G)'; t'] G through wv::gdg_blocks, staged in LDS as sweep A of tmpc_kernels.hip stages it
//
// Every entry takes HOST pointers, allocates, launches, synchronises, copies back, frees and returns the HIP error code (0 = success),
// -2 for a size that is not compiled, -3 for a count out of range.  Fixed grids, no loop that depends on data, nothing waited on.
#include "tmpc_wave.hpp"

#include <cstddef>
#include <utility>

namespace {

namespace wv = tmpc::wv;
constexpr int L = wv::WAVE;
constexpr int MAX_PROBLEMS = 4096;
constexpr int MAX_KSTEPS = 16;
constexpr int ZERO_ROWS = 4;               // as in tmpc_kernels.hip: the look-ahead of the pass reads one k-step past the last
constexpr double SENTINEL = -7.0e77;
constexpr int odd_up(int v) { return v | 1; }

struct Dev {
    void *p[8];
    int n = 0;
    hipError_t err = hipSuccess;
    void *raw(size_t bytes) {
        void *d = nullptr;
        if (err != hipSuccess || n >= 8) { if (err == hipSuccess) err = hipErrorOutOfMemory; return nullptr; }
        err = hipMalloc(&d, bytes);
        if (err != hipSuccess) return nullptr;
        p[n++] = d;
        return d;
    }
    template <class T>
    const T *in(const T *h, size_t cnt) {
        void *d = raw(cnt * sizeof(T));
        if (d) err = hipMemcpy(d, h, cnt * sizeof(T), hipMemcpyHostToDevice);
        return static_cast<const T *>(d);
    }
    template <class T>
    T *out(size_t cnt) {
        void *d = raw(cnt * sizeof(T));
        if (d) err = hipMemset(d, 0xFF, cnt * sizeof(T));
        return static_cast<T *>(d);
    }
    bool ok() const { return err == hipSuccess; }
    void ran() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    template <class T>
    void back(T *h, const T *d, size_t cnt) {
        if (err == hipSuccess) err = hipMemcpy(h, d, cnt * sizeof(T), hipMemcpyDeviceToHost);
    }
    ~Dev() {
        for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
    }
};

__global__ __launch_bounds__(L) void k_raw(const double *a, const double *b, const double *c, double *d) {
    const size_t at = static_cast<size_t>(blockIdx.x) * L + threadIdx.x;
    d[at] = wv::mfma_blocks(a[at], b[at], c[at]);
}

// ---- timing.  The first time stamp is taken by a statement that also "writes" the operands, the second by one that reads a scalar
// copy of every accumulator: the matrix instructions lie between the two in program order and have delivered their results.
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int T_UNROLL = 16, T_ROUNDS = 32, T_INSTS = T_UNROLL * T_ROUNDS;
__device__ __forceinline__ long long stamp_start(double &a, double &b) {
    long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t), "+v"(a), "+v"(b) : : "memory");
    return t;
}
__device__ __forceinline__ long long stamp_end(int dep) {
    long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "s"(dep) : "memory");
    return t;
}
// KIND 0: blocks, 2 accumulators; 1: tiles, 2 accumulators; 2: blocks, 1 accumulator (dependent); 3: blocks, 4 accumulators; 4: tiles, 1 accumulator
template <int KIND>
__global__ __launch_bounds__(L) void k_time(const double *in, long long *cycles, double *sink) {
    const int lane = static_cast<int>(threadIdx.x);
    double a = in[lane], b = in[L + lane];
    constexpr bool TILE = KIND == 1 || KIND == 4;
    constexpr int NACC = KIND == 0 || KIND == 1 ? 2 : KIND == 3 ? 4 : 1;
    double accb[4] = {0.0, 0.0, 0.0, 0.0};
    v4d acct[2] = {v4d{0.0, 0.0, 0.0, 0.0}, v4d{0.0, 0.0, 0.0, 0.0}};
    const long long t0 = stamp_start(a, b);
#pragma unroll 1
    for (int r = 0; r < T_ROUNDS; ++r) {
#pragma unroll
        for (int u = 0; u < T_UNROLL; ++u) {
            if constexpr (TILE) acct[u % NACC] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acct[u % NACC], 0, 0, 0);
            else accb[u % NACC] = wv::mfma_blocks(a, b, accb[u % NACC]);
        }
    }
    double tot = 0.0;
    if constexpr (TILE) tot = acct[0][0] + acct[0][1] + acct[0][2] + acct[0][3] + acct[1][0] + acct[1][1] + acct[1][2] + acct[1][3];
    else tot = (accb[0] + accb[1]) + (accb[2] + accb[3]);
    const int dep = __builtin_amdgcn_readfirstlane(__double2hiint(tot));
    const long long t1 = stamp_end(dep);
    if (lane == 0) cycles[0] = t1 - t0;
    sink[lane] = tot;
}

// ---- the pass: G[p][4 nks][NV], (D, t)[p][4 nks] -> mf[p][NV][LDM] (pre-filled with the sentinel), gdr[p][NV]
template <int NV>
__global__ __launch_bounds__(L) void k_gdg(const double *G, const double *D, const double *t, int nks, double *mf, double *gdr) {
    constexpr int LDG = 16 * ((NV + 1 + 15) / 16) + 1, LDM = odd_up(NV + 1);      // Shape::LDG, Shape::LDM of tmpc_kernels.hip
    __shared__ double Gt[(4 * MAX_KSTEPS + ZERO_ROWS) * LDG];
    __shared__ double dtw[2 * (4 * MAX_KSTEPS + ZERO_ROWS)];
    __shared__ double mt[NV * LDM];
    __shared__ double gd[NV];
    const int lane = static_cast<int>(threadIdx.x);
    const size_t p = blockIdx.x;
    const int rows = 4 * nks;
    for (int e = lane; e < (rows + ZERO_ROWS) * LDG; e += L) {
        const int f = e / LDG, j = e - f * LDG;
        Gt[e] = (f < rows && j < NV) ? G[(p * rows + f) * NV + j] : (f < rows && j == NV) ? 1.0 : 0.0;      // (column NV: the pass's contract)
    }
    for (int f = lane; f < rows + ZERO_ROWS; f += L) {
        dtw[2 * f] = f < rows ? D[p * rows + f] : 0.0;
        dtw[2 * f + 1] = f < rows ? t[p * rows + f] : 0.0;
    }
    for (int e = lane; e < NV * LDM; e += L) mt[e] = SENTINEL;
    if (lane < NV) gd[lane] = SENTINEL;
    __syncthreads();
    wv::gdg_blocks<NV, LDG, LDM>(Gt, nks, dtw, mt, gd, lane);
    __syncthreads();
    for (int e = lane; e < NV * LDM; e += L) mf[p * NV * LDM + e] = mt[e];
    if (lane < NV) gdr[p * NV + lane] = gd[lane];
}

template <int... V, class F>
bool dispatch(int v, std::integer_sequence<int, V...>, F &&f) {
    return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}
using GdgNV = std::integer_sequence<int, 8, 11, 12, 22>;

}  // namespace

extern "C" {

__attribute__((visibility("default"))) double mfmablocks_sentinel() { return SENTINEL; }
__attribute__((visibility("default"))) int mfmablocks_time_insts() { return T_INSTS; }
__attribute__((visibility("default"))) int mfmablocks_ldm(int nv) { return odd_up(nv + 1); }

// a / b / c / d[np][64]: d = mfma_blocks(a, b, c), lane by lane
__attribute__((visibility("default"))) int mfmablocks_raw(int np, const double *a, const double *b, const double *c, double *d) {
    if (np < 1 || np > MAX_PROBLEMS) return -3;
    const size_t w = static_cast<size_t>(np) * L;
    Dev dv;
    const double *da = dv.in(a, w), *db = dv.in(b, w), *dc = dv.in(c, w);
    double *dd = dv.out<double>(w);
    if (dv.ok()) {
        k_raw<<<np, L>>>(da, db, dc, dd);
        dv.ran();
    }
    dv.back(d, dd, w);
    return static_cast<int>(dv.err);
}

// cycles[reps]: s_memtime ticks of mfmablocks_time_insts() instructions of chain `kind`, one launch per repetition
__attribute__((visibility("default"))) int mfmablocks_time(int kind, int reps, long long *cycles) {
    if (reps < 1 || reps > 64) return -3;
    if (kind < 0 || kind > 4) return -2;
    double ab[2 * L];
    for (int i = 0; i < 2 * L; ++i) ab[i] = 1.0 + 0.001 * i;
    Dev dv;
    const double *din = dv.in(ab, 2 * L);
    long long *dc = dv.out<long long>(1);
    double *sink = dv.out<double>(L);
    for (int r = 0; r < reps && dv.ok(); ++r) {
        if (kind == 0) k_time<0><<<1, L>>>(din, dc, sink);
        else if (kind == 1) k_time<1><<<1, L>>>(din, dc, sink);
        else if (kind == 2) k_time<2><<<1, L>>>(din, dc, sink);
        else if (kind == 3) k_time<3><<<1, L>>>(din, dc, sink);
        else k_time<4><<<1, L>>>(din, dc, sink);
        dv.ran();
        dv.back(cycles + r, dc, 1);
    }
    return static_cast<int>(dv.err);
}

// G[np][4 nks][nv], D / t[np][4 nks] -> mf[np][nv][mfmablocks_ldm(nv)], gdr[np][nv]
__attribute__((visibility("default"))) int mfmablocks_gdg(int nv, int nks, int np, const double *G, const double *D, const double *t, double *mf,
                                                          double *gdr) {
    if (np < 1 || np > MAX_PROBLEMS || nks < 1 || nks > MAX_KSTEPS) return -3;
    int rc = 0;
    const bool known = dispatch(nv, GdgNV{}, [&](auto nv_) {
        constexpr int NV = decltype(nv_)::value;
        const size_t rows = static_cast<size_t>(np) * 4 * nks;
        Dev dv;
        const double *dG = dv.in(G, rows * NV), *dD = dv.in(D, rows), *dt = dv.in(t, rows);
        double *dmf = dv.out<double>(static_cast<size_t>(np) * NV * odd_up(NV + 1)), *dg = dv.out<double>(static_cast<size_t>(np) * NV);
        if (dv.ok()) {
            k_gdg<NV><<<np, L>>>(dG, dD, dt, nks, dmf, dg);
            dv.ran();
        }
        dv.back(mf, dmf, static_cast<size_t>(np) * NV * odd_up(NV + 1));
        dv.back(gdr, dg, static_cast<size_t>(np) * NV);
        rc = static_cast<int>(dv.err);
    });
    return known ? rc : -2;
}

}  // extern "C"
