// Ensemble statistics of the closed loops' per-step record (gfx950; include/tmpc.h: tmpc_mc_series_stats, tmpc_series_stats).
//
// The record is time-major, e[T][B] and word[T][B] (tmpc_mc_step.hpp writes it); a COLUMN is the entries [t][b] of the members b of one
// group g -- a thousand values or so, T x G columns.  One workgroup per column, one launch:
//
//   phase 1   every thread walks the column with stride SERIES_THREADS: the counts of the word's bits, maxima and sums of its two fields,
//             and of the values that take part (ALIVE set, e not NaN) a partial sum and the largest order-preserving key.  The 256 partial
//             results meet in a tree through LDS -- integers, so exact in any order; the sum of e in the tree's fixed order: no atomics on
//             doubles, the same bytes from call to call.
//   phase 2   exact order statistics by a most-significant-digit radix select on the keys: eight passes of 8 bits, the histograms in LDS, the
//             column read again from L2 in every pass -- a column is not limited by LDS.  All quantiles go through a pass together; those whose
//             prefixes (still) coincide share a histogram, all of them in the first pass.  A pass: LDS atomic adds into 256 bins, sixteen
//             threads per quantile sum sixteen bins each, one thread per quantile finds the chunk and the bin that holds its rank.  After the
//             last pass the prefix IS the key of the answer: ties need no care; +-inf keep their place.
//
// LDS: a histogram row is 256 bins + 16 words, so that the rows of the four quantiles a wave sums lie 16 banks apart, and a thread starts
// its sixteen bins at its own offset: the sixty-four lanes of the summing wave read sixty-four banks.  The atomic adds of a pass go where the
// data sends them; equal values meet in one bin and serialise there (64 lanes: 64 LDS cycles per instruction, a few instructions per pass).
// No private arrays, no scratch; members beyond the column are never loaded.
#ifdef TMPC_HOST_SIM
#include "west_sim.hpp"     // tests/wavesim: this very source compiled for the CPU under sanitizers (never in the product)
#else
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "tmpc_device.hpp"
#include "tmpc_launch.hpp"
#include "tmpc_series.hpp"
#include "tmpc_west.hpp"

namespace tmpc {

namespace {

using ull = unsigned long long;

constexpr int SERIES_THREADS = 256;
constexpr int SERIES_BINS = 256, SERIES_DIGIT_BITS = 8, SERIES_PASSES = 8;
constexpr int SERIES_ROW = SERIES_BINS + 16;       // words between two histograms
constexpr int SERIES_CHUNKS = 16;                  // threads that sum a histogram; SERIES_BINS / SERIES_CHUNKS bins each
constexpr int SERIES_PART_ROW = SERIES_CHUNKS + 1;
constexpr int SERIES_NI = 11;                      // per-thread 32-bit results: the eight counts, age_max, iters_max, values that take part
constexpr int SERIES_NL = 3;                       // 64-bit ones: age_sum, iters_sum, the largest key
static_assert(SERIES_MAX_Q * SERIES_CHUNKS == SERIES_THREADS && SERIES_MAX_Q == TMPC_SER_MAX_Q, "one thread per (quantile, chunk)");

// LDS in 8-byte words: the tree's arrays, reused by the histograms once the totals are read; then the selection's state
constexpr size_t SERIES_TREE_WORDS = static_cast<size_t>(SERIES_NL + 1) * SERIES_THREADS + static_cast<size_t>(SERIES_NI) * SERIES_THREADS / 2 + SERIES_THREADS / 2;
constexpr size_t SERIES_HIST_WORDS = static_cast<size_t>(SERIES_MAX_Q) * SERIES_ROW / 2;
constexpr size_t SERIES_UNION_WORDS = SERIES_TREE_WORDS > SERIES_HIST_WORDS ? SERIES_TREE_WORDS : SERIES_HIST_WORDS;
constexpr size_t SERIES_STATE_WORDS = SERIES_MAX_Q + SERIES_MAX_Q + static_cast<size_t>(SERIES_MAX_Q) * SERIES_PART_ROW / 2 + 1;      // prefix; rank | slot; partial sums; n
constexpr size_t SERIES_LDS_BYTES = (SERIES_UNION_WORDS + SERIES_STATE_WORDS) * 8;

// the grid of a launch: every workgroup on the host execution model (launch_grid runs workgroup 0 alone there)
template <class... P, class... A>
hipError_t series_launch(void (*kernel)(P...), unsigned blocks, unsigned threads, size_t lds, hipStream_t stream, A &&...args) {
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

__global__ __launch_bounds__(SERIES_THREADS) void series_stats_kernel(const SeriesStats a) {
#ifdef TMPC_HOST_SIM
    ull *smem = sim::lds<ull>();
#else
    extern __shared__ __attribute__((aligned(16))) ull smem[];
#endif
    // the tree: [SERIES_NL][256] 64-bit, [256] double, [SERIES_NI][256] 32-bit
    ull *sl = smem;
    double *sd = reinterpret_cast<double *>(smem + SERIES_NL * SERIES_THREADS);
    unsigned *si = reinterpret_cast<unsigned *>(smem + (SERIES_NL + 1) * SERIES_THREADS);
    unsigned *hist = reinterpret_cast<unsigned *>(smem);                                   // [n_q][SERIES_ROW], after the tree
    ull *spre = smem + SERIES_UNION_WORDS;                                                 // [16] digits found so far
    unsigned *srank = reinterpret_cast<unsigned *>(spre + SERIES_MAX_Q);                   // [16] rank among the keys with that prefix
    unsigned *sslot = srank + SERIES_MAX_Q;                                                // [16] first quantile with the same prefix: whose histogram to read
    unsigned *part = sslot + SERIES_MAX_Q;                                                 // [16][SERIES_PART_ROW]
    unsigned *sn = part + SERIES_MAX_Q * SERIES_PART_ROW;                                  // [1] values that take part

    const int tid = threadIdx.x;
    const int64_t col = blockIdx.x, ncol = static_cast<int64_t>(a.T) * a.G;
    const int t = static_cast<int>(col / a.G), g = static_cast<int>(col - static_cast<int64_t>(t) * a.G);
    const int64_t i0 = a.start[g], i1 = a.start[g + 1];
    const double *__restrict__ e_row = a.e + static_cast<int64_t>(t) * a.B;
    const uint32_t *__restrict__ w_row = a.word + static_cast<int64_t>(t) * a.B;

    // ---- phase 1
    unsigned c_alive = 0, c_nan = 0, c_up = 0, c_down = 0, c_adopt = 0, c_tube = 0, c_nopt = 0, c_over = 0, c_part = 0, age_mx = 0, it_mx = 0;
    ull age_sum = 0, it_sum = 0, kmax = 0;
    double esum = 0.0;
    for (int64_t i = i0 + tid; i < i1; i += SERIES_THREADS) {
        const int64_t b = a.member[i];
        const uint32_t w = w_row[b];
        if (!(w & TMPC_SER_ALIVE)) continue;
        ++c_alive;
        c_up += (w >> 1) & 1u; c_down += (w >> 2) & 1u; c_adopt += (w >> 3) & 1u; c_tube += (w >> 4) & 1u; c_nopt += (w >> 5) & 1u; c_over += (w >> 6) & 1u;
        const unsigned it = (w >> TMPC_SER_ITERS_SHIFT) & TMPC_SER_SATURATE, age = w >> TMPC_SER_AGE_SHIFT;
        it_mx = it > it_mx ? it : it_mx;
        age_mx = age > age_mx ? age : age_mx;
        it_sum += it;
        age_sum += age;
        const double v = e_row[b];
        if (v != v) { ++c_nan; continue; }
        ++c_part;
        esum += v;
        const ull key = west_key(__builtin_bit_cast(ull, v));
        kmax = key > kmax ? key : kmax;
    }
    si[0 * SERIES_THREADS + tid] = c_alive; si[1 * SERIES_THREADS + tid] = c_nan; si[2 * SERIES_THREADS + tid] = c_up; si[3 * SERIES_THREADS + tid] = c_down;
    si[4 * SERIES_THREADS + tid] = c_adopt; si[5 * SERIES_THREADS + tid] = c_tube; si[6 * SERIES_THREADS + tid] = c_nopt; si[7 * SERIES_THREADS + tid] = c_over;
    si[8 * SERIES_THREADS + tid] = age_mx; si[9 * SERIES_THREADS + tid] = it_mx; si[10 * SERIES_THREADS + tid] = c_part;
    sl[0 * SERIES_THREADS + tid] = age_sum; sl[1 * SERIES_THREADS + tid] = it_sum; sl[2 * SERIES_THREADS + tid] = kmax;
    sd[tid] = esum;
    for (int off = SERIES_THREADS / 2; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) {
#pragma unroll
            for (int k = 0; k < SERIES_NI; ++k) {
                const unsigned x = si[k * SERIES_THREADS + tid], y = si[k * SERIES_THREADS + tid + off];
                si[k * SERIES_THREADS + tid] = (k == 8 || k == 9) ? (x > y ? x : y) : x + y;
            }
#pragma unroll
            for (int k = 0; k < SERIES_NL; ++k) {
                const ull x = sl[k * SERIES_THREADS + tid], y = sl[k * SERIES_THREADS + tid + off];
                sl[k * SERIES_THREADS + tid] = k == 2 ? (x > y ? x : y) : x + y;
            }
            sd[tid] = sd[tid] + sd[tid + off];
        }
    }
    const int nq = a.n_q;
    if (tid == 0) {
        const unsigned n = si[10 * SERIES_THREADS];
#pragma unroll
        for (int k = 0; k < SERIES_INT_TABLES; ++k) a.out_i[k * ncol + col] = static_cast<int32_t>(si[k * SERIES_THREADS]);
        a.out_l[col] = static_cast<int64_t>(sl[0]);
        a.out_l[ncol + col] = static_cast<int64_t>(sl[SERIES_THREADS]);
        a.out_d[col] = n ? sd[0] : 0.0;
        a.out_d[ncol + col] = n ? __builtin_bit_cast(double, west_unkey(sl[2 * SERIES_THREADS])) : __longlong_as_double(0x7ff8000000000000ll);
        sn[0] = n;
    }
    __syncthreads();                      // the totals are read: the tree's arrays become the histograms
    const unsigned n = sn[0];
    if (nq == 0) return;
    if (n == 0) {
        if (tid < nq) a.out_q[col * nq + tid] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }

    // ---- phase 2: rank floor(q (n - 1)) of every quantile, one multiplication and one floor (the host twins compute the same)
    if (tid < nq) {
        const double pos = a.q[tid] * static_cast<double>(n - 1u);
        spre[tid] = 0ull;
        srank[tid] = static_cast<unsigned>(floor(pos));
        sslot[tid] = 0u;
    }
    for (int pass = 0; pass < SERIES_PASSES; ++pass) {
        const int shift = 64 - SERIES_DIGIT_BITS * (pass + 1);
        for (int i = tid; i < nq * SERIES_ROW; i += SERIES_THREADS) hist[i] = 0u;
        __syncthreads();
        for (int64_t i = i0 + tid; i < i1; i += SERIES_THREADS) {
            const int64_t b = a.member[i];
            if (!(w_row[b] & TMPC_SER_ALIVE)) continue;
            const double v = e_row[b];
            if (v != v) continue;
            const ull key = west_key(__builtin_bit_cast(ull, v));
            const unsigned digit = static_cast<unsigned>(key >> shift) & (SERIES_BINS - 1);
            for (int r = 0; r < nq; ++r)
                if (sslot[r] == static_cast<unsigned>(r) && (pass == 0 || ((key ^ spre[r]) >> (shift + SERIES_DIGIT_BITS)) == 0ull))
                    atomicAdd(&hist[r * SERIES_ROW + digit], 1u);
        }
        __syncthreads();
        {
            // thread (r, ch) sums the bins [16 ch, 16 ch + 16) of quantile r's histogram, starting at bin 16 ch + ch
            const int r = tid / SERIES_CHUNKS, ch = tid % SERIES_CHUNKS;
            if (r < nq) {
                const unsigned *H = hist + sslot[r] * SERIES_ROW + ch * (SERIES_BINS / SERIES_CHUNKS);
                unsigned s = 0u;
                for (int k = 0; k < SERIES_BINS / SERIES_CHUNKS; ++k) s += H[(k + ch) & (SERIES_BINS / SERIES_CHUNKS - 1)];
                part[r * SERIES_PART_ROW + ch] = s;
            }
        }
        __syncthreads();
        if (tid < nq) {
            // the rank lies in the column (rank < n = the sum of the histogram): the last chunk and the last bin need no test
            const unsigned *H = hist + sslot[tid] * SERIES_ROW;
            const unsigned k = srank[tid];
            unsigned below = 0u;
            int ch = 0;
            for (; ch < SERIES_CHUNKS - 1; ++ch) {
                const unsigned v = part[tid * SERIES_PART_ROW + ch];
                if (k < below + v) break;
                below += v;
            }
            int bin = ch * (SERIES_BINS / SERIES_CHUNKS);
            for (int j = 0; j < SERIES_BINS / SERIES_CHUNKS - 1; ++j) {
                const unsigned v = H[bin];
                if (k < below + v) break;
                below += v;
                ++bin;
            }
            spre[tid] |= static_cast<ull>(bin) << shift;
            srank[tid] = k - below;
        }
        __syncthreads();
        if (tid < nq) {
            unsigned s = static_cast<unsigned>(tid);
            for (int j = tid - 1; j >= 0; --j)
                if (spre[j] == spre[tid]) s = static_cast<unsigned>(j);
            sslot[tid] = s;
        }
        __syncthreads();
    }
    if (tid < nq) a.out_q[col * nq + tid] = __builtin_bit_cast(double, west_unkey(spre[tid]));
}

}  // namespace

hipError_t launch_series_stats(const SeriesStats &s, hipStream_t stream) {
    if (s.B < 1 || s.T < 1 || s.G < 1 || s.n_q < 0 || s.n_q > SERIES_MAX_Q || !s.e || !s.word || !s.member || !s.start || !s.out_i || !s.out_l || !s.out_d ||
        (s.n_q > 0 && (!s.out_q || !s.q)))
        return hipErrorInvalidValue;
    const int64_t ncol = static_cast<int64_t>(s.T) * s.G;
    if (ncol > 0x7fffffffll) return hipErrorInvalidValue;
    return series_launch(series_stats_kernel, static_cast<unsigned>(ncol), SERIES_THREADS, SERIES_LDS_BYTES, stream, s);
}

}  // namespace tmpc
