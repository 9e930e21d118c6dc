// TEST INFRASTRUCTURE (not product code): the wave helpers of csrc/tmpc_wave.hpp as shipped -- inline-assembly DPP forms, the real
// v_permlane32_swap / v_permlane16_swap, v_rcp_f64, the bare v_max_f64 / v_min_f64 -- on the device, one 64-lane wave per problem
// and one block per problem, behind plain C entry points for ctypes (tests/test_wave_primitives_gpu.py).  csrc/Makefile builds it
// twice: lib/libtmpc_wavecheck.so with the product's flags and lib/libtmpc_wavecheck_nofmac.so with -DTMPC_NO_DPP_FMAC (the
// compiler's two-instruction form of the DPP multiply-add).  Nothing of the product but tmpc_wave.hpp is included, and the
// product library links none of this.
//
// Every entry takes HOST pointers: it checks the sizes, allocates device memory, launches, synchronises, copies back, frees and
// returns the HIP error code (0 = success), -2 for a size that is not compiled, -3 for a problem count outside [1, MAX_PROBLEMS].
// The kernels have a fixed grid and fully unrolled bodies: no loop depends on data and nothing is waited on.
#include "tmpc_wave.hpp"

#include <cstddef>
#include <utility>

namespace {

namespace wv = tmpc::wv;
constexpr int L = wv::WAVE;
constexpr int MAXC = 52;                  // values per lane of a data set of the sums (tests/wavesim/swapsum_main.cpp)
constexpr int MAX_PROBLEMS = 4096;
constexpr int MAX_ELEMS = 1 << 20;
constexpr double SENTINEL = -7.0e77;      // what the kernels put where a routine is expected to write (or to leave alone)
constexpr int odd_up(int v) { return v | 1; }      // Shape::odd_up of tmpc_kernels.hip

// device buffers of one call: everything is freed when the entry returns, the first error sticks
struct Dev {
    void *p[16];
    int n = 0;
    hipError_t err = hipSuccess;
    void *raw(size_t bytes) {
        void *d = nullptr;
        if (err != hipSuccess || n >= 16) { if (err == hipSuccess) err = hipErrorOutOfMemory; return nullptr; }
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
        if (d) err = hipMemset(d, 0xFF, cnt * sizeof(T));      // (all ones: a NaN / -1 where a kernel failed to write)
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

// calls f(integral_constant<int, V>) for the V of the list that equals v; false if there is none
template <int... V, class F>
bool dispatch(int v, std::integer_sequence<int, V...>, F &&f) {
    return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}
template <int OFF, int... I>
constexpr auto shifted(std::integer_sequence<int, I...>) { return std::integer_sequence<int, (OFF + I)...>{}; }

// ---- lanes_factor / lanes_backsub_lane with the carried right-hand side, lanes_forward + lanes_backsub_lane with a second one.
// The caller lays the wave out: rows[p][lane][N] is the matrix row that lane `lane` of problem p holds (N <= 16: every 16-lane
// row of the wave its own matrix), b1 / b2[p][lane] its right-hand-side entries.  All 64 lanes report.
template <int N>
__global__ __launch_bounds__(L) void k_lanes(const double *rows, const double *b1, const double *b2, double *frows, double *dinv,
                                              double *x, double *x2, int *ok) {
    const int lane = static_cast<int>(threadIdx.x);
    const size_t at = static_cast<size_t>(blockIdx.x) * L + lane;
    double row[N];
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = rows[at * N + j];
    double b = b1[at], d = 1.0;
    const bool o = wv::lanes_factor<N>(row, b, d, lane);
    const double xl = wv::lanes_backsub_lane<N>(row, b, d, lane);
    double bb = b2[at];
    wv::lanes_forward<N>(row, bb, lane);
    const double xl2 = wv::lanes_backsub_lane<N>(row, bb, d, lane);
#pragma unroll
    for (int j = 0; j < N; ++j) frows[at * N + j] = row[j];
    dinv[at] = d;
    x[at] = xl;
    x2[at] = xl2;
    ok[at] = o ? 1 : 0;
}

// ---- rows32_factor_solve, then rows32_resolve with a second right-hand side.  M[p][N][N], b1 / b2[p][N]; returns x[p][N], the LDS
// matrix after the call fac[p][N][LDM] (factor, 1 / d_i in column N; the kernel pre-fills column N and the padding behind it,
// x and x2 with the sentinel), x2[p][N] (the sentinel where the factor failed: the kernels do not resolve then) and ok[p][64].
template <int N>
__global__ __launch_bounds__(L) void k_rows32(const double *M, const double *b1, const double *b2, double *x, double *fac, double *x2,
                                               int *ok) {
    constexpr int LDM = odd_up(N + 1);
    __shared__ double Mf[N * LDM];
    __shared__ double rhs[N], xs[N];
    const int lane = static_cast<int>(threadIdx.x);
    const size_t p = blockIdx.x;
    for (int e = lane; e < N * LDM; e += L) {
        const int i = e / LDM, j = e - i * LDM;
        Mf[e] = j < N ? M[(p * N + i) * N + j] : SENTINEL;
    }
    if (lane < N) { rhs[lane] = b1[p * N + lane]; xs[lane] = SENTINEL; }
    __syncthreads();
    const bool o = wv::rows32_factor_solve<N, LDM>(Mf, rhs, xs, lane);
    __syncthreads();
    for (int e = lane; e < N * LDM; e += L) fac[p * N * LDM + e] = Mf[e];
    if (lane < N) x[p * N + lane] = xs[lane];
    ok[p * L + lane] = o ? 1 : 0;
    __syncthreads();
    if (lane < N) { rhs[lane] = b2[p * N + lane]; xs[lane] = SENTINEL; }
    __syncthreads();
    if (o) wv::rows32_resolve<N, LDM>(Mf, rhs, xs, lane);      // (wave-uniform: readfirstlane inside the factor)
    __syncthreads();
    if (lane < N) x2[p * N + lane] = xs[lane];
}

// ---- the sums: in[s][MAXC][64] (value c of lane l of data set s at c * 64 + l, the layout of swapsum_main.cpp), res[s][64][CNT]:
// what every lane reads back from the CNT totals
template <int CNT>
__device__ __forceinline__ void load_acc(double (&acc)[CNT], const double *in, int lane) {
#pragma unroll
    for (int c = 0; c < CNT; ++c) acc[c] = in[static_cast<size_t>(blockIdx.x) * MAXC * L + c * L + lane];
}
template <int CNT>
__device__ __forceinline__ void store_totals(const double *out, double *res, int lane) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CNT; ++c) res[(static_cast<size_t>(blockIdx.x) * L + lane) * CNT + c] = out[c];
}
template <int CNT>
__device__ __forceinline__ void poison(double *out, int lane) {
    for (int c = lane; c < CNT; c += L) out[c] = SENTINEL;
    __syncthreads();
}
template <int CNT, int RR>
__global__ __launch_bounds__(L) void k_swap(const double *in, double *res) {
    __shared__ double red[RR * wv::RED_STRIDE];
    __shared__ double out[CNT];
    const int lane = static_cast<int>(threadIdx.x);
    double acc[CNT];
    load_acc(acc, in, lane);
    poison<CNT>(out, lane);
    wv::swap_reduce_to_lds<CNT, RR>(acc, red, out, lane);
    store_totals<CNT>(out, res, lane);
}
// one round for totals that live in two LDS arrays (tmpc_kernels.hip: wave_sums_to_lds2): entries below SPLIT to out0, the others to out1
template <int CNT, int RR, int SPLIT>
__global__ __launch_bounds__(L) void k_swap_at(const double *in, double *res) {
    __shared__ double red[RR * wv::RED_STRIDE];
    __shared__ double out[CNT + 8];          // out0 = out, out1 = out + SPLIT + 8: a gap that must stay untouched
    const int lane = static_cast<int>(threadIdx.x);
    double acc[CNT];
    load_acc(acc, in, lane);
    poison<CNT + 8>(out, lane);
    double *out0 = out, *out1 = out + SPLIT + 8;
    wv::swap_reduce_to_lds_at<CNT, RR>(acc, red, [out0, out1](int e) { return e < SPLIT ? out0 + e : out1 + (e - SPLIT); }, lane);
    store_totals<CNT + 8>(out, res, lane);
}
template <int CNT>
__global__ __launch_bounds__(L) void k_reduce(const double *in, double *res) {
    __shared__ double red[16 * wv::RED_STRIDE];
    __shared__ double out[CNT];
    const int lane = static_cast<int>(threadIdx.x);
    double acc[CNT];
    load_acc(acc, in, lane);
    poison<CNT>(out, lane);
    wv::reduce_to_lds<CNT>(acc, red, out, lane);
    store_totals<CNT>(out, res, lane);
}
// wave_sum2 of values 0 and 1: res[s][64][2]
__global__ __launch_bounds__(L) void k_sum2(const double *in, double *res) {
    const int lane = static_cast<int>(threadIdx.x);
    double acc[2];
    load_acc(acc, in, lane);
    wv::wave_sum2(acc[0], acc[1], lane);
    res[(static_cast<size_t>(blockIdx.x) * L + lane) * 2] = acc[0];
    res[(static_cast<size_t>(blockIdx.x) * L + lane) * 2 + 1] = acc[1];
}
// wave_reduce of value 0: res[s][64]
template <class Op>
__global__ __launch_bounds__(L) void k_wave_reduce(const double *in, double *res) {
    const int lane = static_cast<int>(threadIdx.x);
    double acc[1];
    load_acc(acc, in, lane);
    res[static_cast<size_t>(blockIdx.x) * L + lane] = wv::wave_reduce<Op>(acc[0]);
}

// ---- elementwise: fast_rcp(a), vmax(a, b), vmin(a, b), vmax_abs(a, b)
template <int OP>
__global__ __launch_bounds__(L) void k_elem(const double *a, const double *b, double *r, int n) {
    const int i = static_cast<int>(blockIdx.x) * L + static_cast<int>(threadIdx.x);
    if (i >= n) return;
    if constexpr (OP == 0) r[i] = wv::fast_rcp(a[i]);
    else if constexpr (OP == 1) r[i] = wv::vmax(a[i], b[i]);
    else if constexpr (OP == 2) r[i] = wv::vmin(a[i], b[i]);
    else r[i] = wv::vmax_abs(a[i], b[i]);
}

template <class K>
int run_sums(K kernel, int cnt, const double *in, int nsets, double *res) {
    Dev dv;
    const double *din = dv.in(in, static_cast<size_t>(nsets) * MAXC * L);
    double *dres = dv.out<double>(static_cast<size_t>(nsets) * L * cnt);
    if (dv.ok()) {
        kernel<<<nsets, L>>>(din, dres);
        dv.ran();
    }
    dv.back(res, dres, static_cast<size_t>(nsets) * L * cnt);
    return static_cast<int>(dv.err);
}

using LanesN = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 28>;
using Rows32N = std::integer_sequence<int, 17, 22, 24, 26, 31, 32>;
using ReduceN = std::integer_sequence<int, 1, 15, 16, 17, 33>;
using Count32 = decltype(shifted<1>(std::make_integer_sequence<int, 32>{}));
using CountB = std::integer_sequence<int, 44, 52>;

}  // namespace

extern "C" {

__attribute__((visibility("default"))) double wavecheck_sentinel() { return SENTINEL; }

// 1 if this library was built with the compiler's form of the DPP multiply-add (-DTMPC_NO_DPP_FMAC)
__attribute__((visibility("default"))) int wavecheck_nofmac() {
#ifdef TMPC_NO_DPP_FMAC
    return 1;
#else
    return 0;
#endif
}

// rows[np][64][n], b1 / b2[np][64] -> frows[np][64][n], dinv / x / x2[np][64], ok[np][64]
__attribute__((visibility("default"))) int wavecheck_lanes(int n, int np, const double *rows, const double *b1, const double *b2,
                                                           double *frows, double *dinv, double *x, double *x2, int *ok) {
    if (np < 1 || np > MAX_PROBLEMS) return -3;
    int rc = 0;
    const bool known = dispatch(n, LanesN{}, [&](auto n_) {
        constexpr int N = decltype(n_)::value;
        const size_t w = static_cast<size_t>(np) * L;
        Dev dv;
        const double *drows = dv.in(rows, w * N), *db1 = dv.in(b1, w), *db2 = dv.in(b2, w);
        double *dfr = dv.out<double>(w * N), *ddi = dv.out<double>(w), *dx = dv.out<double>(w), *dx2 = dv.out<double>(w);
        int *dok = dv.out<int>(w);
        if (dv.ok()) {
            k_lanes<N><<<np, L>>>(drows, db1, db2, dfr, ddi, dx, dx2, dok);
            dv.ran();
        }
        dv.back(frows, dfr, w * N);
        dv.back(dinv, ddi, w);
        dv.back(x, dx, w);
        dv.back(x2, dx2, w);
        dv.back(ok, dok, w);
        rc = static_cast<int>(dv.err);
    });
    return known ? rc : -2;
}

// M[np][n][n], b1 / b2[np][n] -> x[np][n], fac[np][n][ldm], x2[np][n], ok[np][64]; ldm = wavecheck_rows32_ldm(n)
__attribute__((visibility("default"))) int wavecheck_rows32_ldm(int n) { return n > 16 && n <= 32 ? odd_up(n + 1) : -2; }
__attribute__((visibility("default"))) int wavecheck_rows32(int n, int np, const double *M, const double *b1, const double *b2, double *x,
                                                            double *fac, double *x2, int *ok) {
    if (np < 1 || np > MAX_PROBLEMS) return -3;
    int rc = 0;
    const bool known = dispatch(n, Rows32N{}, [&](auto n_) {
        constexpr int N = decltype(n_)::value;
        constexpr int LDM = odd_up(N + 1);
        const size_t q = static_cast<size_t>(np);
        Dev dv;
        const double *dM = dv.in(M, q * N * N), *db1 = dv.in(b1, q * N), *db2 = dv.in(b2, q * N);
        double *dx = dv.out<double>(q * N), *dfac = dv.out<double>(q * N * LDM), *dx2 = dv.out<double>(q * N);
        int *dok = dv.out<int>(q * L);
        if (dv.ok()) {
            k_rows32<N><<<np, L>>>(dM, db1, db2, dx, dfac, dx2, dok);
            dv.ran();
        }
        dv.back(x, dx, q * N);
        dv.back(fac, dfac, q * N * LDM);
        dv.back(x2, dx2, q * N);
        dv.back(ok, dok, q * L);
        rc = static_cast<int>(dv.err);
    });
    return known ? rc : -2;
}

// swap_reduce_to_lds<cnt, rr>: in[nsets][52][64] -> res[nsets][64][cnt]
__attribute__((visibility("default"))) int wavecheck_swap_reduce(int cnt, int rr, const double *in, int nsets, double *res) {
    if (nsets < 1 || nsets > MAX_PROBLEMS) return -3;
    int rc = 0;
    bool known = false;
    if (rr == 12) {
        known = dispatch(cnt, Count32{}, [&](auto c) { rc = run_sums(k_swap<decltype(c)::value, 12>, cnt, in, nsets, res); }) ||
                dispatch(cnt, CountB{}, [&](auto c) { rc = run_sums(k_swap<decltype(c)::value, 12>, cnt, in, nsets, res); });
    } else if (rr == 16) {
        known = dispatch(cnt, Count32{}, [&](auto c) { rc = run_sums(k_swap<decltype(c)::value, 16>, cnt, in, nsets, res); });
    }
    return known ? rc : -2;
}
// swap_reduce_to_lds_at<34, 12> with the split output of the bench shape's sweep B (2 NV = 22 totals to one array, 2 KC + 2 = 12 to
// another): res[nsets][64][42]: out0 at 0 .. 21, eight untouched sentinels, out1 at 30 .. 41
__attribute__((visibility("default"))) int wavecheck_swap_reduce_split(const double *in, int nsets, double *res) {
    if (nsets < 1 || nsets > MAX_PROBLEMS) return -3;
    return run_sums(k_swap_at<34, 12, 22>, 42, in, nsets, res);
}
// reduce_to_lds<cnt>: in[nsets][52][64] -> res[nsets][64][cnt]
__attribute__((visibility("default"))) int wavecheck_reduce(int cnt, const double *in, int nsets, double *res) {
    if (nsets < 1 || nsets > MAX_PROBLEMS) return -3;
    int rc = 0;
    const bool known = dispatch(cnt, ReduceN{}, [&](auto c) { rc = run_sums(k_reduce<decltype(c)::value>, cnt, in, nsets, res); });
    return known ? rc : -2;
}
// wave_sum2 of values 0 and 1: res[nsets][64][2]
__attribute__((visibility("default"))) int wavecheck_sum2(const double *in, int nsets, double *res) {
    if (nsets < 1 || nsets > MAX_PROBLEMS) return -3;
    return run_sums(k_sum2, 2, in, nsets, res);
}
// wave_reduce<OpSum (0) / OpMin (1) / OpMax (2)> of value 0: res[nsets][64]
__attribute__((visibility("default"))) int wavecheck_wave_reduce(int op, const double *in, int nsets, double *res) {
    if (nsets < 1 || nsets > MAX_PROBLEMS) return -3;
    if (op == 0) return run_sums(k_wave_reduce<wv::OpSum>, 1, in, nsets, res);
    if (op == 1) return run_sums(k_wave_reduce<wv::OpMin>, 1, in, nsets, res);
    if (op == 2) return run_sums(k_wave_reduce<wv::OpMax>, 1, in, nsets, res);
    return -2;
}
// op 0: fast_rcp(a) (b unused, may be null), 1: vmax(a, b), 2: vmin(a, b), 3: vmax_abs(a, b); n elements
__attribute__((visibility("default"))) int wavecheck_elementwise(int op, const double *a, const double *b, int n, double *r) {
    if (n < 1 || n > MAX_ELEMS) return -3;
    if (op < 0 || op > 3) return -2;
    Dev dv;
    const double *da = dv.in(a, static_cast<size_t>(n));
    const double *db = op == 0 ? da : dv.in(b, static_cast<size_t>(n));
    double *dr = dv.out<double>(static_cast<size_t>(n));
    if (dv.ok()) {
        const int blocks = (n + L - 1) / L;
        if (op == 0) k_elem<0><<<blocks, L>>>(da, db, dr, n);
        else if (op == 1) k_elem<1><<<blocks, L>>>(da, db, dr, n);
        else if (op == 2) k_elem<2><<<blocks, L>>>(da, db, dr, n);
        else k_elem<3><<<blocks, L>>>(da, db, dr, n);
        dv.ran();
    }
    dv.back(r, dr, static_cast<size_t>(n));
    return static_cast<int>(dv.err);
}

}  // extern "C"
