// Estimation of the disturbance set W of a linear model from closed loops on the plant it was derived from (gfx950) -- the reference's
// Results/estimate_W_for_Cartpole.py on the RK4 cart-pole of the device closed loop (mcstep::cartpole_rhs):
//
//   x_{k+1} = plant(x_k, u_k = -K x_k)   (force held over one sampling period),      w_k = x_k - (A - B K) x_{k-1},  k = 1 .. T - 1
//
// for many initial states (estimate_W_for_Cartpole.py:78-107), then order statistics of each component of w over all trajectories and
// periods (:117-120: the 1.25 % / 98.75 % quantiles).
//
//   west_rollout_kernel   one LANE per trajectory: the four states and the RK4 stages in registers, 4 (T - 1) doubles written per lane,
//                         component-major so that the lanes of a wave write adjacent words.  Minimum and maximum per component: in
//                         registers, over the wave at the end, then integer atomics on the order-preserving key (below) -- the result
//                         does not depend on the order in which the waves arrive.
//   west_hist_kernel /    exact selection by most-significant-digit radix: a double maps to a 64-bit key whose unsigned order is the
//   west_narrow_kernel    order of the values (negative: all bits flipped, otherwise: sign bit flipped; -0 < +0 are neighbours).  Six
//                         passes of 11, 11, 11, 11, 11 and 9 bits.  A pass counts, per requested rank, the digit of every key that
//                         matches the rank's prefix so far: per workgroup in LDS (32-bit counts), the non-empty bins then go to the
//                         global histogram with one 64-bit integer add each.  One wave per column narrows: the bin that holds the
//                         rank extends the prefix, the rank becomes the rank inside that bin.  Ranks that (still) share a prefix
//                         share a histogram -- all of them in the first pass.  After the last pass the prefix IS the key of the
//                         answer: ties need no care.  NaN have no order: they are counted and left out; +-inf keep their place.
#ifdef TMPC_HOST_SIM
#include "west_sim.hpp"     // tests/wavesim: this very source compiled for the CPU under sanitizers (never in the product)
#else
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "tmpc_device.hpp"
#include "tmpc_launch.hpp"
#include "tmpc_mc_step.hpp"
#include "tmpc_wave.hpp"
#include "tmpc_west.hpp"

namespace tmpc {

namespace {

using ull = unsigned long long;

constexpr int WEST_ROLL_THREADS = 64;        // one wave per workgroup: 65 536 trajectories are one wave per SIMD of the device
constexpr int WEST_HIST_THREADS = 256;
constexpr ull WEST_NO_SLOT = ~0ull;
constexpr ull WEST_ABS = 0x7fffffffffffffffull, WEST_INF = 0x7ff0000000000000ull;

// the grid of a launch: every workgroup on the host execution model (launch_grid runs workgroup 0 alone there)
template <class... P, class... A>
hipError_t west_launch(void (*kernel)(P...), unsigned blocks, unsigned threads, size_t lds, hipStream_t stream, A &&...args) {
#ifdef TMPC_HOST_SIM
    (void)stream;
    for (unsigned b = 0; b < blocks; ++b) {
        sim::Dim3 bi, gd;
        bi.x = b;
        gd.x = blocks;
        sim_rendezvous_total += sim::run_block(static_cast<int>(threads), lds, bi, gd, [&]() { kernel(static_cast<P>(args)...); });
    }
    return hipSuccess;
#else
    return launch_grid(kernel, blocks, threads, lds, stream, static_cast<A &&>(args)...);
#endif
}

__device__ __forceinline__ ull west_bits(double v) { return __builtin_bit_cast(ull, v); }

// lo + (hi - lo) u in two roundings, as numpy evaluates it (a fused multiply-add would round once)
__device__ __forceinline__ double west_in_box(double lo, double hi, double u) {
#pragma clang fp contract(off)
    const double span = hi - lo;
    const double prod = span * u;
    return lo + prod;
}

__global__ __launch_bounds__(WEST_ROLL_THREADS) void west_rollout_kernel(WestRollout a) {
    const int lane = threadIdx.x & 63;
    const int64_t b = static_cast<int64_t>(blockIdx.x) * WEST_ROLL_THREADS + threadIdx.x;
    const bool live = b < a.n_traj;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        if (a.draw) {
            ull r[4];
            mcstep::philox4x64(0ull, 0ull, a.seed, static_cast<ull>(a.first + b), r);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = west_in_box(a.lo[i], a.hi[i], mcstep::u01(r[i]));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = a.x0[b * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) a.x0_used[b * 4 + i] = x[i];
    }
    double mn[4], mx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; }
    // the plant of the lane's trajectory: the call's, or the lane's own seven numbers (tmpc_estimate_w_models); Acl and K stay the model's
    double par[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) par[i] = a.par[i];
    if (a.par_traj != nullptr && live) {
#pragma unroll
        for (int i = 0; i < 7; ++i) par[i] = a.par_traj[b * 7 + i];
    }
    const double dt = par[6] / a.substeps;
    const int64_t per_comp = static_cast<int64_t>(a.T - 1) * a.n_traj;
    if (live) {
        for (int k = 0; k < a.T; ++k) {
            double xp[4] = {x[0], x[1], x[2], x[3]};
            double u0 = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) u0 -= a.K[i] * x[i];
            // zero-order hold of u over the sampling period, RK4 at the physics rate: the hold of mcstep::mc_step_wave, operation for operation
            for (int sstep = 0; sstep < a.substeps; ++sstep) {
                double k1[4], k2[4], k3[4], k4[4], yt[4];
                mcstep::cartpole_rhs(par, x, u0, k1);
                for (int i = 0; i < 4; ++i) yt[i] = x[i] + 0.5 * dt * k1[i];
                mcstep::cartpole_rhs(par, yt, u0, k2);
                for (int i = 0; i < 4; ++i) yt[i] = x[i] + 0.5 * dt * k2[i];
                mcstep::cartpole_rhs(par, yt, u0, k3);
                for (int i = 0; i < 4; ++i) yt[i] = x[i] + dt * k3[i];
                mcstep::cartpole_rhs(par, yt, u0, k4);
                for (int i = 0; i < 4; ++i) x[i] += dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
            }
            // the state after the last period is not sampled (estimate_W_for_Cartpole.py:94-107: w is formed when the NEXT input is)
            if (k + 1 < a.T) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double s = a.Acl[c * 4] * xp[0];
#pragma unroll
                    for (int i = 1; i < 4; ++i) s += a.Acl[c * 4 + i] * xp[i];
                    const double w = x[c] - s;
                    a.samples[c * per_comp + static_cast<int64_t>(k) * a.n_traj + b] = w;
                    if (fabs(w) < INFINITY) { mn[c] = fmin(mn[c], w); mx[c] = fmax(mx[c], w); }
                }
            }
        }
        a.xnorm[b] = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
    }
    // every lane of the wave is here (the ones beyond n_traj carry +-inf)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double lo = wv::wave_reduce<wv::OpMin>(mn[c]), hi = wv::wave_reduce<wv::OpMax>(mx[c]);
        if (lane == 0) {
            atomicMin(&a.minmax[c], west_key(west_bits(lo)));
            atomicMax(&a.minmax[4 + c], west_key(west_bits(hi)));
        }
    }
}

// ---------------------------------------------------------------- selection
__device__ __forceinline__ int west_shift(int pass) { return pass < WEST_PASSES - 1 ? 64 - WEST_DIGIT_BITS * (pass + 1) : 0; }
__device__ __forceinline__ int west_width(int pass) { return pass < WEST_PASSES - 1 ? WEST_DIGIT_BITS : 64 - WEST_DIGIT_BITS * (WEST_PASSES - 1); }

// the state of a group of ranks, per column c and rank r of the group, at [c * WEST_MAX_RANKS + r]:
//   prefix  the digits found so far (the low bits zero)     rem   the rank among the keys with that prefix
//   slot    the histogram this rank reads: the first rank of the group with the same prefix (WEST_NO_SLOT: beyond the column's values)
__global__ __launch_bounds__(64) void west_select_init_kernel(const ull *__restrict__ ranks, int g0, int R, int ncol, ull *__restrict__ prefix,
                                                              ull *__restrict__ rem, ull *__restrict__ slot) {
    for (int t = threadIdx.x; t < ncol * WEST_MAX_RANKS; t += 64) {
        const int r = t % WEST_MAX_RANKS;
        prefix[t] = 0ull;
        rem[t] = r < R ? ranks[g0 + r] : 0ull;
        slot[t] = r < R ? 0ull : WEST_NO_SLOT;
    }
}

// workgroups [c * nblk, (c + 1) * nblk) share column c.  LDS: the prefixes (8 x 64 bit), which ranks own a histogram (8 x 32 bit), the
// workgroup's count of non-finite values, R histograms of 2048 x 32 bit (a workgroup sees fewer than 2^32 keys: n < 2^32 * nblk is
// the launcher's business).
__global__ __launch_bounds__(WEST_HIST_THREADS) void west_hist_kernel(const double *__restrict__ data, int64_t n, int64_t col_stride, int nblk, int R,
                                                                       int pass, const ull *__restrict__ prefix, const ull *__restrict__ slot,
                                                                       ull *__restrict__ hist, ull *__restrict__ nonfinite) {
#ifdef TMPC_HOST_SIM
    ull *smem = sim::lds<ull>();
#else
    extern __shared__ __attribute__((aligned(16))) ull smem[];
#endif
    ull *spre = smem;
    unsigned *sact = reinterpret_cast<unsigned *>(smem + WEST_MAX_RANKS), *cnt = sact + WEST_MAX_RANKS, *h = sact + 2 * WEST_MAX_RANKS;
    const int tid = threadIdx.x;
    const int c = static_cast<int>(blockIdx.x) / nblk, j = static_cast<int>(blockIdx.x) % nblk;
    for (int i = tid; i < R * WEST_BINS; i += WEST_HIST_THREADS) h[i] = 0u;
    if (tid < WEST_MAX_RANKS) {
        spre[tid] = prefix[c * WEST_MAX_RANKS + tid];
        sact[tid] = (tid < R && slot[c * WEST_MAX_RANKS + tid] == static_cast<ull>(tid)) ? 1u : 0u;
    }
    if (tid == 0) cnt[0] = 0u;
    __syncthreads();
    const int shift = west_shift(pass), hs = shift + west_width(pass);
    const ull mask = (1ull << west_width(pass)) - 1ull;
    const double *__restrict__ col = data + static_cast<int64_t>(c) * col_stride;
    unsigned nf = 0u;
    for (int64_t i = static_cast<int64_t>(j) * WEST_HIST_THREADS + tid; i < n; i += static_cast<int64_t>(nblk) * WEST_HIST_THREADS) {
        const ull u = west_bits(col[i]), mag = u & WEST_ABS;
        if (mag >= WEST_INF) {
            ++nf;
            if (mag > WEST_INF) continue;                 // NaN: no order, no rank
        }
        const ull key = west_key(u);
        const unsigned digit = static_cast<unsigned>((key >> shift) & mask);
        if (pass == 0) {
            atomicAdd(&h[digit], 1u);
        } else {
            for (int r = 0; r < R; ++r)
                if (sact[r] && (key >> hs) == (spre[r] >> hs)) atomicAdd(&h[r * WEST_BINS + digit], 1u);
        }
    }
    if (nonfinite && nf) atomicAdd(&cnt[0], nf);
    __syncthreads();
    for (int i = tid; i < R * WEST_BINS; i += WEST_HIST_THREADS) {
        const unsigned v = h[i];
        if (v) atomicAdd(&hist[(static_cast<size_t>(c) * WEST_MAX_RANKS + i / WEST_BINS) * WEST_BINS + i % WEST_BINS], static_cast<ull>(v));
    }
    if (nonfinite && tid == 0 && cnt[0]) atomicAdd(&nonfinite[c], static_cast<ull>(cnt[0]));
}

// One wave per column: for every rank of the group the bin of its histogram that holds it.  LDS (64 bit): the 64 lanes' partial sums,
// then the group's prefixes, ranks and slots.
__global__ __launch_bounds__(64) void west_narrow_kernel(int R, int pass, int n_rank, int g0, ull *__restrict__ prefix, ull *__restrict__ rem,
                                                         ull *__restrict__ slot, const ull *__restrict__ hist, double *__restrict__ out) {
#ifdef TMPC_HOST_SIM
    ull *smem = sim::lds<ull>();
#else
    extern __shared__ __attribute__((aligned(16))) ull smem[];
#endif
    ull *part = smem, *spre = smem + 64, *srem = spre + WEST_MAX_RANKS, *sslot = srem + WEST_MAX_RANKS;
    const int lane = threadIdx.x, c = blockIdx.x;
    const int shift = west_shift(pass), per = (1 << west_width(pass)) / 64;
    if (lane < WEST_MAX_RANKS) {
        spre[lane] = prefix[c * WEST_MAX_RANKS + lane];
        srem[lane] = rem[c * WEST_MAX_RANKS + lane];
        sslot[lane] = slot[c * WEST_MAX_RANKS + lane];
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const ull sl = sslot[r];                           // (the same on every lane: the branch is uniform)
        if (sl == WEST_NO_SLOT) continue;
        const ull *H = hist + (static_cast<size_t>(c) * WEST_MAX_RANKS + sl) * WEST_BINS;
        ull sum = 0ull;
        for (int q = 0; q < per; ++q) sum += H[lane * per + q];
        part[lane] = sum;
        __syncthreads();
        const ull k = srem[r];
        int L = -1;
        ull base = 0ull, cum = 0ull;
        for (int l = 0; l < 64; ++l) {
            const ull v = part[l];
            if (L < 0 && k < cum + v) { L = l; base = cum; }
            cum += v;
        }
        __syncthreads();
        if (lane == 0) {
            if (L < 0) {
                sslot[r] = WEST_NO_SLOT;                   // fewer values than this rank asks for
            } else {
                ull below = base;
                int bin = L * per;
                for (int q = 0; q < per - 1; ++q) {
                    const ull v = H[L * per + q];
                    if (k < below + v) break;
                    below += v;
                    ++bin;
                }
                spre[r] |= static_cast<ull>(bin) << shift;
                srem[r] = k - below;
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        for (int r = 0; r < R; ++r) {
            if (sslot[r] == WEST_NO_SLOT) continue;
            int s = r;
            for (int q = r - 1; q >= 0; --q)
                if (sslot[q] != WEST_NO_SLOT && spre[q] == spre[r]) s = q;
            sslot[r] = static_cast<ull>(s);
        }
    }
    __syncthreads();
    if (lane < WEST_MAX_RANKS) {
        prefix[c * WEST_MAX_RANKS + lane] = spre[lane];
        rem[c * WEST_MAX_RANKS + lane] = srem[lane];
        slot[c * WEST_MAX_RANKS + lane] = sslot[lane];
        if (pass == WEST_PASSES - 1 && lane < R)
            out[static_cast<size_t>(c) * n_rank + g0 + lane] =
                sslot[lane] == WEST_NO_SLOT ? __longlong_as_double(0x7ff8000000000000ll) : __builtin_bit_cast(double, west_unkey(spre[lane]));
    }
}

}  // namespace

hipError_t launch_west_rollout(const WestRollout &a, hipStream_t stream) {
    if (a.n_traj < 1 || a.T < 2 || a.substeps < 1) return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>((a.n_traj + WEST_ROLL_THREADS - 1) / WEST_ROLL_THREADS);
    return west_launch(west_rollout_kernel, blocks, WEST_ROLL_THREADS, 0, stream, a);
}

size_t west_select_ws_words(int ncol) { return static_cast<size_t>(ncol) * WEST_MAX_RANKS * (WEST_BINS + 3); }

hipError_t launch_west_select(const double *data, int64_t n, int64_t col_stride, int ncol, int n_rank, const unsigned long long *ranks,
                              unsigned long long *ws, double *out, unsigned long long *nonfinite, hipStream_t stream) {
    if (n < 1 || ncol < 1 || n_rank < 0 || (n_rank > 0 && (!ranks || !out))) return hipErrorInvalidValue;
    const size_t per = static_cast<size_t>(ncol) * WEST_MAX_RANKS;
    ull *hist = ws, *prefix = ws + per * WEST_BINS, *rem = prefix + per, *slot = rem + per;
    const int nblk = static_cast<int>(n / 4096 < 1 ? 1 : (n / 4096 > 512 ? 512 : n / 4096));
    if (nonfinite)
        if (const hipError_t e = hipMemsetAsync(nonfinite, 0, sizeof(ull) * ncol, stream); e != hipSuccess) return e;
    // (without ranks: one counting pass for `nonfinite`)
    for (int g0 = 0; g0 < (n_rank > 0 ? n_rank : 1); g0 += WEST_MAX_RANKS) {
        const int R = n_rank > 0 ? (n_rank - g0 < WEST_MAX_RANKS ? n_rank - g0 : WEST_MAX_RANKS) : 1;
        if (n_rank > 0) {
            if (const hipError_t e = west_launch(west_select_init_kernel, 1, 64, 0, stream, ranks, g0, R, ncol, prefix, rem, slot); e != hipSuccess) return e;
        } else {
            if (const hipError_t e = hipMemsetAsync(prefix, 0, sizeof(ull) * 3 * per, stream); e != hipSuccess) return e;
        }
        const size_t lds_hist = sizeof(ull) * WEST_MAX_RANKS + sizeof(unsigned) * (2 * WEST_MAX_RANKS + static_cast<size_t>(R) * WEST_BINS);
        for (int pass = 0; pass < (n_rank > 0 ? WEST_PASSES : 1); ++pass) {
            if (const hipError_t e = hipMemsetAsync(hist, 0, sizeof(ull) * per * WEST_BINS, stream); e != hipSuccess) return e;
            if (const hipError_t e = west_launch(west_hist_kernel, static_cast<unsigned>(ncol * nblk), WEST_HIST_THREADS, lds_hist, stream, data, n, col_stride,
                                                 nblk, R, pass, prefix, slot, hist, (g0 == 0 && pass == 0) ? nonfinite : nullptr);
                e != hipSuccess)
                return e;
            if (n_rank == 0) break;
            if (const hipError_t e = west_launch(west_narrow_kernel, static_cast<unsigned>(ncol), 64, sizeof(ull) * (64 + 3 * WEST_MAX_RANKS), stream, R, pass,
                                                 n_rank, g0, prefix, rem, slot, hist, out);
                e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

}  // namespace tmpc
