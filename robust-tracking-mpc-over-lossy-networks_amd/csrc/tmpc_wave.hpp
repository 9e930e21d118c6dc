// Wave-level device helpers shared by the kernels (tmpc_kernels.hip, tmpc_block.hip, tmpc_lp.hip): DPP / permlane / readlane
// reductions over the 64 lanes of a gfx950 wavefront and a division-free reciprocal.
#pragma once
#ifdef TMPC_HOST_SIM
#include "hip_sim.hpp"      // tests/wavesim: the same source compiled for the CPU (sanitizer runs), never in the product
#else
#include <hip/hip_runtime.h>
#endif

#include <cstdint>
#include <utility>

namespace tmpc {
namespace wv {

constexpr int WAVE = 64;

// 1/x to full double precision for normal, finite x: v_rcp_f64 + two Newton steps
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
// max / min as the bare instruction.  `fmax` compiles to v_max_f64 preceded by a canonicalising v_max_f64 x, x of every
// operand the compiler cannot prove quiet (2-3 instructions per call in the row sweeps); the instruction itself already
// returns the other operand when one is a NaN, which is all these reductions need.
#ifdef TMPC_HOST_SIM
__device__ __forceinline__ double vmax(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double vmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double vmax_abs(double a, double b) { return fmax(a, fabs(b)); }
#else
__device__ __forceinline__ double vmax(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmin(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmax_abs(double a, double b) {      // max(a, |b|)
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
#endif
struct OpSum { __device__ __forceinline__ static double f(double a, double b) { return a + b; } };
struct OpMin { __device__ __forceinline__ static double f(double a, double b) { return vmin(a, b); } };
struct OpMax { __device__ __forceinline__ static double f(double a, double b) { return vmax(a, b); } };

// all-reduce over the wave: every lane returns the total
template <class Op>
__device__ __forceinline__ double wave_reduce(double v) {
    v = Op::f(v, dpp_mov_d<0xB1>(v));    // quad_perm [1,0,3,2]
    v = Op::f(v, dpp_mov_d<0x4E>(v));    // quad_perm [2,3,0,1]
    v = Op::f(v, dpp_mov_d<0x141>(v));   // row_half_mirror
    v = Op::f(v, dpp_mov_d<0x140>(v));   // row_mirror
    const double r0 = readlane_d(v, 0), r1 = readlane_d(v, 16), r2 = readlane_d(v, 32), r3 = readlane_d(v, 48);
    return Op::f(Op::f(r0, r1), Op::f(r2, r3));
}

// Orders one wave's LDS traffic for the compiler (the hardware runs the DS instructions of a wave in issue order).
#ifdef TMPC_HOST_SIM
__device__ __forceinline__ void lds_fence() { sim::wave_fence(); }
#else
__device__ __forceinline__ void lds_fence() { asm volatile("" ::: "memory"); }
#endif

// Sum each of acc[0..CNT) over the 64 lanes, totals to out[0..CNT) (LDS).  `red` is a [16][68] tile: 16 entries per round
// are written as rows (lane l at column l + l/16), lane l then adds the 16-lane quarter (l & 3) of entry (l >> 2) and
// the four quarters of a quad meet through two DPP quad permutes.
constexpr int RED_STRIDE = 68;
template <int CNT>
__device__ __forceinline__ void reduce_to_lds(const double (&acc)[CNT], double *red, double *out, int lane) {
    const int e = lane >> 2, qd = lane & 3;
    const int wcol = lane + (lane >> 4);
#pragma unroll
    for (int c0 = 0; c0 < CNT; c0 += 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (c0 + k < CNT) red[k * RED_STRIDE + wcol] = acc[c0 + k];
        lds_fence();
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) t += red[e * RED_STRIDE + qd * 17 + j];
        t += dpp_mov_d<0xB1>(t);
        t += dpp_mov_d<0x4E>(t);
        if (qd == 0 && c0 + e < CNT) out[c0 + e] = t;
        lds_fence();
    }
}

// ---- wave sums in registers with the cross-half swaps of gfx950.  v_permlane32_swap_b32 x, y exchanges the upper 32 lanes of x
// with the lower 32 lanes of y, v_permlane16_swap_b32 x, y the odd 16-lane rows of x with the even rows of y.  Followed by one
// v_add_f64, a swap of two 64-bit values (two swaps: low and high dwords) leaves on the lanes WITHOUT bit HALF the sum of `a`
// over lanes l and l ^ HALF, and on the lanes WITH it the same sum of `b`: two partial sums halve into one register, with no
// LDS and no fence.  (The compiler inserts the wait states in front of a swap whose operand was just written.)
template <int HALF>
__device__ __forceinline__ void permlane_swap(int &x, int &y, int lane) {
    static_assert(HALF == 32 || HALF == 16, "v_permlane32_swap / v_permlane16_swap");
#ifdef TMPC_HOST_SIM
    const int xo = __builtin_amdgcn_readlane(x, lane ^ HALF), yo = __builtin_amdgcn_readlane(y, lane ^ HALF);
    const bool up = (lane & HALF) != 0;
    x = up ? yo : x;
    y = up ? y : xo;
#else
    (void)lane;
    if constexpr (HALF == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
        x = static_cast<int>(r[0]);
        y = static_cast<int>(r[1]);
    } else {
        const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
        x = static_cast<int>(r[0]);
        y = static_cast<int>(r[1]);
    }
#endif
}
template <int HALF>
__device__ __forceinline__ double swap_add(double a, double b, int lane) {
    int alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
    permlane_swap<HALF>(alo, blo, lane);
    permlane_swap<HALF>(ahi, bhi, lane);
    return __hiloint2double(ahi, alo) + __hiloint2double(bhi, blo);
}

// Totals of a and b over the wave, on every lane: one swap puts a on the lower and b on the upper 32 lanes, the rest is
// wave_reduce's butterfly and four v_readlane -- two sums for the price of one.
__device__ __forceinline__ void wave_sum2(double &a, double &b, int lane) {
    double v = swap_add<32>(a, b, lane);
    v += dpp_mov_d<0xB1>(v);
    v += dpp_mov_d<0x4E>(v);
    v += dpp_mov_d<0x141>(v);
    v += dpp_mov_d<0x140>(v);
    a = readlane_d(v, 0) + readlane_d(v, 16);
    b = readlane_d(v, 32) + readlane_d(v, 48);
}

// Sum each of acc[0..CNT) over the 64 lanes, totals to out[0..CNT) (LDS): the contract of the transposition tile's reduction
// with a quarter of its LDS traffic.  Level 1: entry c and entry c + H1 (H1 = ceil(CNT / 2)) share a register after a
// v_permlane32_swap (c on lanes 0-31, c + H1 on lanes 32-63, each summed over lanes l and l ^ 32).  Level 2: register d and
// register d + H2 (H2 = ceil(H1 / 2)) the same with v_permlane16_swap: register d then holds on its 16-lane row r the entry
// d + (r & 1) H2 + (r >> 1) H1 as sixteen partial sums (a register without a partner pairs with zero).  Finish: the H2
// registers go to rows of the [RR][RED_STRIDE] tile (lane l at column l + l / 16) -- H2 <= RR stores per lane where the
// tile form needs CNT --, and lane l adds the sixteen partial sums of row (l >> 2), quarter (l & 3): a complete total, no
// DPP step.  More than RR rows: rounds of RR.  The general form takes the place of total e from `out_at(e)`, so that one
// round can serve totals that live in different LDS arrays.
template <int CNT, int RR, class OutAt>
__device__ __forceinline__ void swap_reduce_to_lds_at(const double (&acc)[CNT], double *red, OutAt &&out_at, int lane) {
    constexpr int H1 = (CNT + 1) / 2, H2 = (H1 + 1) / 2;
    double r1[H1];
#pragma unroll
    for (int c = 0; c < H1; ++c) r1[c] = swap_add<32>(acc[c], c + H1 < CNT ? acc[c + H1] : 0.0, lane);
    double r2[H2];
#pragma unroll
    for (int d = 0; d < H2; ++d) r2[d] = swap_add<16>(r1[d], d + H2 < H1 ? r1[d + H2] : 0.0, lane);
    // entry of register d on 16-lane row r; -1 where that place holds the zero partner's sums
    auto entry = [](int d, int r) {
        const int e = d + (r & 1) * H2 + (r >> 1) * H1;
        return ((r & 1) && d + H2 >= H1) || e >= CNT ? -1 : e;
    };
    const int wcol = lane + (lane >> 4);
    const int k = lane >> 2, qd = lane & 3;
#pragma unroll
    for (int d0 = 0; d0 < H2; d0 += RR) {
#pragma unroll
        for (int d = 0; d < RR; ++d)
            if (d0 + d < H2) red[d * RED_STRIDE + wcol] = r2[d0 + d];
        lds_fence();
        constexpr int NR = RR < 16 ? RR : 16;
        const int kr = k < NR && d0 + k < H2 ? k : 0;      // (lanes beyond the stored rows read row 0 and store nothing)
        double t4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 16; ++j) t4[j & 3] += red[kr * RED_STRIDE + qd * 17 + j];
        const double t = (t4[0] + t4[1]) + (t4[2] + t4[3]);
        const int e = (k < NR && d0 + k < H2) ? entry(d0 + k, qd) : -1;
        if (e >= 0) *out_at(e) = t;
        lds_fence();
    }
}
template <int CNT, int RR>
__device__ __forceinline__ void swap_reduce_to_lds(const double (&acc)[CNT], double *red, double *out, int lane) {
    swap_reduce_to_lds_at<CNT, RR>(acc, red, [out](int e) { return out + e; }, lane);
}

// n x n symmetric positive definite solve with the rows on the lanes: lane i (< N) holds row i in registers; LDL' by
// Gaussian elimination without pivoting, the pivot row broadcast with v_readlane.  `b` is carried as an extra column.
template <int N>
__device__ __forceinline__ bool rows_factor(double (&row)[N], double &b, double &dinv, int lane) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double pkk = readlane_d(row[k], k);
        ok = ok && (pkk > 0.0);
        const double pinv = fast_rcp(pkk);
        const double f = (lane > k) ? row[k] * pinv : 0.0;
#pragma unroll
        for (int j = k + 1; j < N; ++j) row[j] = fma(-f, readlane_d(row[j], k), row[j]);
        b = fma(-f, readlane_d(b, k), b);
        if (lane > k) row[k] = f;
        if (lane == k) dinv = pinv;
    }
    return ok;
}
template <int N>
__device__ __forceinline__ void rows_forward(const double (&row)[N], double &b, int lane) {
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
        const double f = (lane > k) ? row[k] : 0.0;
        b = fma(-f, readlane_d(b, k), b);
    }
}
// back substitution; x_i is returned on lane i
template <int N>
__device__ __forceinline__ double rows_backsub_lane(const double (&row)[N], double b, double dinv, int lane) {
    double xl = 0.0;
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        const double bi = b * dinv;
        const double xi = readlane_d(bi, i);
        xl = (lane == i) ? bi : xl;
        b = fma(-row[i], xi, b);
    }
    return xl;
}

// ---- the same three routines for N <= 16 with the pivot row handed round by ONE 64-bit DPP move instead of two
// v_readlane_b32: `v_mov_b64_dpp ... row_newbcast:k` (gfx90a and later; the only DPP control the double-precision ALU
// takes) copies lane k of every 16-lane row to the whole row.  Two instructions per multiply-add of the elimination
// instead of three, and no SGPR round trip.  Every 16-lane row of the wave works on the matrix whose row i sits on its
// lane i: the callers keep theirs on lanes 0 .. N-1 and ignore what the other three rows compute.
template <int K>
__device__ __forceinline__ double row_bcast_d(double v) {
    return __builtin_amdgcn_mov_dpp(v, 0x150 + K, 0xF, 0xF, false);      // row_newbcast:K
}
template <int N, class F>
__device__ __forceinline__ void static_for_n(F &&f) {
    [&]<int... I>(std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, N>{});
}
// acc + (lane K of v's 16-lane row) * m in ONE instruction: v_fmac_f64 is a two-operand (VOP2) instruction on gfx90a and later
// and takes the DPP operand itself (`v_fmac_f64_dpp dst, src0, src1 row_newbcast:K`: dst += dpp(src0) * src1).  The compiler
// does not fuse a 64-bit DPP move into the multiply-add that consumes it (round 3 shipped v_mov_b64_dpp + v_fma_f64: two
// instructions and one more link in every dependent chain of the eliminations), hence inline assembly.
// Hazard (gfx9 family, software managed): a vector-ALU write of a VGPR needs two wait states before a DPP read of it, and the
// compiler's hazard recognizer does not look into inline assembly.  The statements are `asm volatile`, i.e. they stay in
// program order among themselves; NOPS > 0 puts `s_nop NOPS-1` in front where the DPP operand may have been written by the
// statement just before (the dependent chains of the substitutions), and the callers order their statements so that the
// other operands were written at least two instructions earlier (each routine says how).
// (-DTMPC_NO_DPP_FMAC: diagnostic builds with the compiler's two-instruction form)
template <int K, int NOPS>
__device__ __forceinline__ void fmac_bcast(double &acc, double v, double m) {
#if defined(TMPC_HOST_SIM) || defined(TMPC_NO_DPP_FMAC)
    acc = fma(row_bcast_d<K>(v), m, acc);
#else
    if constexpr (NOPS > 0)
        asm volatile("s_nop %3\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%4 row_mask:0xf bank_mask:0xf"
                     : "+v"(acc) : "v"(v), "v"(m), "n"(NOPS - 1), "n"(K));
    else
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(v), "v"(m), "n"(K));
#endif
}
// the pivot broadcast in the same (volatile) instruction order as the updates: `v` may have been written by the update two
// statements back (last elimination steps), which the compiler cannot see
template <int K, int NOPS>
__device__ __forceinline__ double row_bcast_ordered(double v) {
#if defined(TMPC_HOST_SIM) || defined(TMPC_NO_DPP_FMAC)
    return row_bcast_d<K>(v);
#else
    double r;
    if constexpr (NOPS > 0)
        asm volatile("s_nop %2\n\tv_mov_b64_dpp %0, %1 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(NOPS - 1), "n"(K));
    else
        asm volatile("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(K));
    return r;
#endif
}
// pins a value: everything that produces `v` is issued before the (empty, volatile) statement, which in turn stays in front
// of the volatile statements that follow
__device__ __forceinline__ void pin(double &v) {
#if !defined(TMPC_HOST_SIM) && !defined(TMPC_NO_DPP_FMAC)
    asm volatile("" : "+v"(v));
#endif
}
// returns whether the matrix of lanes 0 .. N-1 had positive pivots (wave-uniform)
// Software pipelined: the update of column k+1 comes FIRST in step k, the next pivot is broadcast two updates later (the two
// wait states of the DPP read) and its reciprocal -- rcp and four dependent multiply-adds, the longest chain of a step -- runs
// while the remaining updates of step k issue.  Order of the other DPP reads: an update of step k reads a register written in
// step k-1, with at least the pivot broadcast and the multiplier's instructions in between.  The inputs of step 0 come from
// LDS loads (guarded by s_waitcnt) and, b, from the caller through pin().
// (this form, with a select per use of the triangular structure, defines the values: it is what the host execution model and
// the -DTMPC_NO_DPP_FMAC builds run; the product runs rows16_factor_masked below)
template <int N>
__device__ __forceinline__ bool rows16_factor_select(double (&row)[N], double &b, double &dinv, int lane) {
    static_assert(N <= 16, "one matrix row per lane of a 16-lane DPP row");
    const int l16 = lane & 15;
    bool ok = true;
    pin(b);
    double pkk = row_bcast_ordered<0, 0>(row[0]);
    double pinv = fast_rcp(pkk);
    static_for_n<N>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        ok = ok && (pkk > 0.0);
        const double pinv_k = pinv;
        const double f = (l16 > k) ? row[k] * pinv_k : 0.0;
        const double nf = -f;
        constexpr int NU = N - 1 - k;              // columns still to update
        // columns k+1, k+2, k+3 (b takes a place when fewer are left), then the next pivot, then the rest
        static_for_n<(NU < 3 ? NU : 3)>([&](auto j_) {
            constexpr int j = k + 1 + decltype(j_)::value;
            fmac_bcast<k, 0>(row[j], row[j], nf);
        });
        if constexpr (NU < 3) fmac_bcast<k, 0>(b, b, nf);
        if constexpr (k + 1 < N) {
            // (two statements lie between the write of row[k+1] and this read of it -- the DPP hazard's two wait states -- except
            // in the last step but one, where only the update of b does: NU = 1 waits)
            pkk = row_bcast_ordered<k + 1, (NU == 1 ? 2 : 0)>(row[k + 1]);
            pinv = fast_rcp(pkk);
        }
        if constexpr (NU >= 3) {
            static_for_n<NU - 3>([&](auto j_) {
                constexpr int j = k + 4 + decltype(j_)::value;
                fmac_bcast<k, 0>(row[j], row[j], nf);
            });
            fmac_bcast<k, 0>(b, b, nf);
        }
        if (l16 > k) row[k] = f;
        if (l16 == k) dinv = pinv_k;
    });
    return __builtin_amdgcn_readfirstlane(static_cast<int>(ok)) != 0;
}
// The substitutions are ONE dependent chain on b -- every step reads through DPP what the step before wrote, which costs the
// two wait states whatever the instruction --: the fused form gains nothing there, and the compiler fills the wait states of
// its own two-instruction form (v_mov_b64_dpp + v_fma_f64) with the selects of the neighbouring steps.
template <int N>
__device__ __forceinline__ void rows16_forward(const double (&row)[N], double &b, int lane) {
    const int l16 = lane & 15;
    static_for_n<N - 1>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        const double f = (l16 > k) ? row[k] : 0.0;
        b = fma(-f, row_bcast_d<k>(b), b);
    });
}
template <int N>
__device__ __forceinline__ double rows16_backsub_lane_select(const double (&row)[N], double b, double dinv, int lane) {
    const int l16 = lane & 15;
    double xl = 0.0;
    static_for_n<N>([&](auto r_) {
        constexpr int i = N - 1 - decltype(r_)::value;
        const double bi = b * dinv;
        const double xi = row_bcast_d<i>(bi);
        xl = (l16 == i) ? bi : xl;
        b = fma(-row[i], xi, b);
    });
    return xl;
}

// ---- the factorisation and the back substitution without the selects.  `l16 > k`, `l16 == k` and `l16 <= i` are lane patterns
// known at compile time: instead of a compare and two v_cndmask_b32 per 64-bit select, the few instructions that belong to a
// pattern run with EXEC set to it (two s_mov_b32 of a literal; the scalar unit, not the vector pipe the wave shares).  The values
// are those of the select forms above, on every lane and in every 16-lane row:
//   - a multiplier that the select form sets to zero IS zero here too (the updates multiply by it under full EXEC: an infinity
//     in an excluded lane still makes a NaN, and -0 + 0 still gives +0) -- only HOW the zero gets there changes;
//   - the back substitution masks the update itself, which the select form applies to every lane, because the lanes it
//     excludes hold values that nothing reads afterwards (lane i is done once step i has taken its x_i = b_i / d_i).
// All 64 lanes must be active at the call (the DPP broadcasts of the select forms need that as well): every statement restores
// EXEC to -1, so that nothing the compiler places between two statements runs under a pattern.
// A DPP read of a lane that EXEC disables does not deliver its value: the factorisation keeps its DPP instructions outside the
// masked stretches, the back substitution's pattern includes the lane it broadcasts.  A scalar write of EXEC needs no wait
// state in front of a DPP instruction (the five wait states are for a VECTOR write of EXEC).
// (-DTMPC_DEBUG_EXEC: diagnostic builds trap where a masked routine is entered with a lane switched off -- a caller under a divergent
// branch would otherwise get its idle lanes switched on by the restore)
__device__ __forceinline__ void expect_full_exec() {
#if defined(TMPC_DEBUG_EXEC) && !defined(TMPC_HOST_SIM)
    if (__builtin_amdgcn_read_exec() != ~0ull) __builtin_trap();
#endif
}
constexpr unsigned lanes4x16(unsigned m16) { return (m16 & 0xFFFFu) * 0x10001u; }      // the same 16-lane pattern in all four rows, per EXEC half
constexpr unsigned m16_gt(int k) { return (0xFFFFu << (k + 1)) & 0xFFFFu; }
constexpr unsigned m16_eq(int k) { return 1u << k; }
constexpr unsigned m16_le(int i) { return (2u << i) - 1u; }

// step K of the factorisation, everything that depends on the lane's place:  lanes above K: f = rk * pinv, rk = f, nf = -f;
// lane K: dinv = pinv, nf = -0.  Lanes below K keep the -0 they got as lane K of their own step: nf is ONE register through
// all steps (step 0 writes every lane of it).
template <int K>
__device__ __forceinline__ void factor_scale(double &nf, double &rk, double &dinv, double pinv, int l16) {
#if defined(TMPC_HOST_SIM) || defined(TMPC_NO_DPP_FMAC)
    if (l16 > K) {
        const double f = rk * pinv;
        nf = -f;
        rk = f;
    }
    if (l16 == K) {
        dinv = pinv;
        nf = -0.0;
    }
#else
    (void)l16;
    constexpr int GT = static_cast<int>(lanes4x16(m16_gt(K))), EQ = static_cast<int>(lanes4x16(m16_eq(K)));
    if constexpr (K == 0)
        asm volatile("s_mov_b32 exec_lo, %4\n\ts_mov_b32 exec_hi, %4\n\t"
                     "v_mul_f64 %0, -%1, %3\n\tv_mul_f64 %1, %1, %3\n\t"
                     "s_mov_b32 exec_lo, %5\n\ts_mov_b32 exec_hi, %5\n\t"
                     "v_mov_b64 %2, %3\n\tv_lshlrev_b64 %0, 63, 1\n\t"
                     "s_mov_b64 exec, -1"
                     : "=&v"(nf), "+v"(rk), "+v"(dinv) : "v"(pinv), "n"(GT), "n"(EQ));
    else if constexpr (K < 15)
        asm volatile("s_mov_b32 exec_lo, %4\n\ts_mov_b32 exec_hi, %4\n\t"
                     "v_mul_f64 %0, -%1, %3\n\tv_mul_f64 %1, %1, %3\n\t"
                     "s_mov_b32 exec_lo, %5\n\ts_mov_b32 exec_hi, %5\n\t"
                     "v_mov_b64 %2, %3\n\tv_lshlrev_b64 %0, 63, 1\n\t"
                     "s_mov_b64 exec, -1"
                     : "+v"(nf), "+v"(rk), "+v"(dinv) : "v"(pinv), "n"(GT), "n"(EQ));
    else      // (no lane above 15)
        asm volatile("s_mov_b32 exec_lo, %3\n\ts_mov_b32 exec_hi, %3\n\t"
                     "v_mov_b64 %1, %2\n\tv_lshlrev_b64 %0, 63, 1\n\t"
                     "s_mov_b64 exec, -1"
                     : "+v"(nf), "+v"(dinv) : "v"(pinv), "n"(EQ));
#endif
}
// step I of the back substitution on the lanes up to I:  x = b * dinv (lane I's is x_I and stays: the later steps run on fewer
// lanes), then b -= r * (x of lane I).  The fused DPP multiply-add takes the negation as a source modifier; the lanes above I,
// whose b nothing reads any more, sit the step out.  Lane I's own b is spent by the update, which is why x is taken first.
template <int I>
__device__ __forceinline__ void backsub_step(double &b, double &x, double dinv, double r, int l16) {
#if defined(TMPC_HOST_SIM) || defined(TMPC_NO_DPP_FMAC)
    if (l16 <= I) x = b * dinv;
    const double xi = row_bcast_d<I>(x);
    if (l16 <= I) b = fma(xi, -r, b);
#else
    (void)l16;
    constexpr int LE = static_cast<int>(lanes4x16(m16_le(I)));
    if constexpr (I > 0)
        asm volatile("s_mov_b32 exec_lo, %4\n\ts_mov_b32 exec_hi, %4\n\t"
                     "v_mul_f64 %1, %0, %2\n\t"
                     "s_nop 1\n\t"
                     "v_fmac_f64_dpp %0, %1, -%3 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
                     "s_mov_b64 exec, -1"
                     : "+v"(b), "+v"(x) : "v"(dinv), "v"(r), "n"(LE), "n"(I));
    else      // (nothing below lane 0 to update)
        asm volatile("s_mov_b32 exec_lo, %3\n\ts_mov_b32 exec_hi, %3\n\t"
                     "v_mul_f64 %0, %1, %2\n\t"
                     "s_mov_b64 exec, -1"
                     : "+v"(x) : "v"(b), "v"(dinv), "n"(LE));
#endif
}

// rows16_factor_select with factor_scale at the head of every step: the same software pipeline (the next pivot's reciprocal under
// the updates), the same order of the DPP reads -- factor_scale's vector instructions now stand, volatile, between the last write
// of step k - 1 and the first DPP read of step k, where the select form had the multiplier's -- and one register less (pinv_k need
// not outlive the step: dinv takes it at the head).
template <int N>
__device__ __forceinline__ bool rows16_factor_masked(double (&row)[N], double &b, double &dinv, int lane) {
    static_assert(N <= 16, "one matrix row per lane of a 16-lane DPP row");
    const int l16 = lane & 15;
    bool ok = true;
    expect_full_exec();
    pin(b);
    // (row[0] may come straight from the caller's vector instructions -- the working-set matrix of the refinement is built by
    // selects --, and with the multiplier's selects gone nothing of this routine is left to stand in between: two wait states)
    double pkk = row_bcast_ordered<0, 2>(row[0]);
    double pinv = fast_rcp(pkk);
    double nf = -0.0;
    static_for_n<N>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        ok = ok && (pkk > 0.0);
        factor_scale<k>(nf, row[k], dinv, pinv, l16);
        constexpr int NU = N - 1 - k;
        static_for_n<(NU < 3 ? NU : 3)>([&](auto j_) {
            constexpr int j = k + 1 + decltype(j_)::value;
            fmac_bcast<k, 0>(row[j], row[j], nf);
        });
        if constexpr (NU < 3) fmac_bcast<k, 0>(b, b, nf);
        if constexpr (k + 1 < N) {
            pkk = row_bcast_ordered<k + 1, (NU == 1 ? 2 : 0)>(row[k + 1]);
            pinv = fast_rcp(pkk);
        }
        if constexpr (NU >= 3) {
            static_for_n<NU - 3>([&](auto j_) {
                constexpr int j = k + 4 + decltype(j_)::value;
                fmac_bcast<k, 0>(row[j], row[j], nf);
            });
            fmac_bcast<k, 0>(b, b, nf);
        }
    });
    return __builtin_amdgcn_readfirstlane(static_cast<int>(ok)) != 0;
}
// One chain as in the select form -- product, broadcast, update --, two vector instructions a step instead of six.  Lanes beyond
// N return 0 as there.
template <int N>
__device__ __forceinline__ double rows16_backsub_lane_masked(const double (&row)[N], double b, double dinv, int lane) {
    static_assert(N <= 16, "one matrix row per lane of a 16-lane DPP row");
    const int l16 = lane & 15;
    double xl = 0.0;
    expect_full_exec();
    static_for_n<N>([&](auto r_) {
        constexpr int i = N - 1 - decltype(r_)::value;
        backsub_step<i>(b, xl, dinv, row[i], l16);
    });
    return xl;
}
// (the forward substitution keeps its selects: its zero multipliers reach values that ARE read afterwards, so the update
// cannot be masked, and a masked copy of the multiplier costs the vector pipe what the select does)
// SELECT: the caller asks for the select forms (a kernel at the 256-register limit whose allocation the volatile statements of the
// masked forms tip into a spill: tmpc_kernels.hip names it)
// (-DTMPC_SELECT_FORMS: the select forms throughout, everything else as shipped -- csrc/Makefile builds lib/libtmpc_hip_select.so
// that way, the reference of tests/test_select_free_end_to_end_gpu.py)
#if defined(TMPC_HOST_SIM) || defined(TMPC_NO_DPP_FMAC) || defined(TMPC_SELECT_FORMS)
constexpr bool MASKED_FORMS = false;
#else
constexpr bool MASKED_FORMS = true;
#endif
template <int N, bool SELECT = false>
__device__ __forceinline__ bool rows16_factor(double (&row)[N], double &b, double &dinv, int lane) {
    if constexpr (MASKED_FORMS && !SELECT) return rows16_factor_masked<N>(row, b, dinv, lane);
    else return rows16_factor_select<N>(row, b, dinv, lane);
}
template <int N, bool SELECT = false>
__device__ __forceinline__ double rows16_backsub_lane(const double (&row)[N], double b, double dinv, int lane) {
    if constexpr (MASKED_FORMS && !SELECT) return rows16_backsub_lane_masked<N>(row, b, dinv, lane);
    else return rows16_backsub_lane_select<N>(row, b, dinv, lane);
}
// ---- 16 < N <= 32: TWO matrix rows per lane -- lane i of every 16-lane row holds rows i (`ra`) and i + 16 (`rb`) -- so that every
// pivot row sits on a lane of the SAME 16-lane row as the rows it updates and the DPP forms above apply: an update is one
// v_fmac_f64_dpp per row half (two per column while the pivot is among the first sixteen rows, one afterwards) where the
// one-row-per-lane form of round 3 needed two v_readlane_b32 and a multiply-add with a scalar operand, i.e. a scalar-register
// round trip in every link of every chain (N = 26: 1 053 instructions for the elimination against 605 fused updates).
// The matrix lives in LDS (rows of stride LDM: N entries, then 1 / d_i) before and after: `rows32_factor_solve` reads the rows,
// eliminates with the right-hand side `rhs` (LDS, [N]) carried along, leaves the factor in place of the matrix and the solution
// in `x` (LDS, [N]); `rows32_resolve` solves with the stored factor.  Lanes whose second row does not exist (i + 16 >= N) carry
// a copy of row 0 with multipliers forced to zero.
template <int N, int LDM>
__device__ __forceinline__ bool rows32_factor_solve(double *Mf, const double *rhs, double *x, int lane) {
    static_assert(N > 16 && N <= 32, "two matrix rows per lane");
    const int l16 = lane & 15;
    const bool hasb = l16 + 16 < N;
    const int ib = hasb ? l16 + 16 : 0;
    double ra[N], rb[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { ra[j] = Mf[l16 * LDM + j]; rb[j] = Mf[ib * LDM + j]; }
    double ba = rhs[l16], bb = hasb ? rhs[ib] : 0.0;
    double da = 1.0, db = 1.0;
    lds_fence();
    bool ok = true;
    pin(ba);
    pin(bb);
    static_for_n<N>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        constexpr bool inA = k < 16;
        constexpr int kl = k & 15;
        // (the pivot entry was written by the first updates of step k - 1; only the last steps have fewer than two statements behind it)
        double pkk;
        if constexpr (inA) pkk = row_bcast_ordered<kl, (k >= N - 2 ? 2 : 0)>(ra[k]);
        else pkk = row_bcast_ordered<kl, (k >= N - 2 ? 2 : 0)>(rb[k]);
        ok = ok && (pkk > 0.0);
        const double pinv = fast_rcp(pkk);
        double nfa = 0.0;
        if constexpr (inA) nfa = (l16 > k) ? -ra[k] * pinv : 0.0;
        const double nfb = (hasb && l16 + 16 > k) ? -rb[k] * pinv : 0.0;
        static_for_n<N - 1 - k>([&](auto j_) {
            constexpr int j = k + 1 + decltype(j_)::value;
            // (the lower half first: it reads the pivot row's entry of `ra` before the upper half's own update writes that register)
            if constexpr (inA) {
                fmac_bcast<kl, 0>(rb[j], ra[j], nfb);
                fmac_bcast<kl, 0>(ra[j], ra[j], nfa);
            } else {
                fmac_bcast<kl, 0>(rb[j], rb[j], nfb);
            }
        });
        if constexpr (inA) {
            fmac_bcast<kl, 0>(bb, ba, nfb);
            fmac_bcast<kl, 0>(ba, ba, nfa);
            if (l16 > k) ra[k] = -nfa;
            if (l16 == k) da = pinv;
        } else {
            fmac_bcast<kl, 0>(bb, bb, nfb);
            if (l16 == kl) db = pinv;
        }
        if (hasb && l16 + 16 > k) rb[k] = -nfb;
    });
    ok = __builtin_amdgcn_readfirstlane(static_cast<int>(ok)) != 0;
    if (!ok) return false;
    // back substitution (compiler's DPP form: one dependent chain, see rows16_backsub_lane); x_i ends on lane i & 15
    double xa = 0.0, xb = 0.0;
    static_for_n<N>([&](auto r_) {
        constexpr int i = N - 1 - decltype(r_)::value;
        constexpr int il = i & 15;
        if constexpr (i >= 16) {
            const double bi = bb * db;
            const double xi = row_bcast_d<il>(bi);
            xb = (l16 == il) ? bi : xb;
            bb = fma(-rb[i], xi, bb);
            ba = fma(-ra[i], xi, ba);
        } else {
            const double bi = ba * da;
            const double xi = row_bcast_d<il>(bi);
            xa = (l16 == il) ? bi : xa;
            ba = fma(-ra[i], xi, ba);
        }
    });
    if (lane < 16) {
        x[l16] = xa;
        if (hasb) x[ib] = xb;
        // the factor waits in LDS for the corrector's solve
#pragma unroll
        for (int j = 0; j < N; ++j) Mf[l16 * LDM + j] = ra[j];
        Mf[l16 * LDM + N] = da;
        if (hasb) {
#pragma unroll
            for (int j = 0; j < N; ++j) Mf[ib * LDM + j] = rb[j];
            Mf[ib * LDM + N] = db;
        }
    }
    lds_fence();
    return true;
}
template <int N, int LDM>
__device__ __forceinline__ void rows32_resolve(const double *Mf, const double *rhs, double *x, int lane) {
    const int l16 = lane & 15;
    const bool hasb = l16 + 16 < N;
    const int ib = hasb ? l16 + 16 : 0;
    double ra[N], rb[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { ra[j] = Mf[l16 * LDM + j]; rb[j] = Mf[ib * LDM + j]; }
    const double da = Mf[l16 * LDM + N], db = Mf[ib * LDM + N];
    double ba = rhs[l16], bb = hasb ? rhs[ib] : 0.0;
    lds_fence();
    // forward substitution with the stored multipliers
    static_for_n<N - 1>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        constexpr int kl = k & 15;
        const double fb = (hasb && l16 + 16 > k) ? rb[k] : 0.0;
        if constexpr (k < 16) {
            const double fa = (l16 > k) ? ra[k] : 0.0;
            const double xk = row_bcast_d<kl>(ba);
            ba = fma(-fa, xk, ba);
            bb = fma(-fb, xk, bb);
        } else {
            const double xk = row_bcast_d<kl>(bb);
            bb = fma(-fb, xk, bb);
        }
    });
    double xa = 0.0, xb = 0.0;
    static_for_n<N>([&](auto r_) {
        constexpr int i = N - 1 - decltype(r_)::value;
        constexpr int il = i & 15;
        if constexpr (i >= 16) {
            const double bi = bb * db;
            const double xi = row_bcast_d<il>(bi);
            xb = (l16 == il) ? bi : xb;
            bb = fma(-rb[i], xi, bb);
            ba = fma(-ra[i], xi, ba);
        } else {
            const double bi = ba * da;
            const double xi = row_bcast_d<il>(bi);
            xa = (l16 == il) ? bi : xa;
            ba = fma(-ra[i], xi, ba);
        }
    });
    if (lane < 16) {
        x[l16] = xa;
        if (hasb) x[ib] = xb;
    }
    lds_fence();
}

// dispatch: the DPP form where a matrix fits a 16-lane row, the readlane form otherwise (-DTMPC_NO_DPP64: diagnostic
// builds with the readlane form throughout)
#ifdef TMPC_NO_DPP64
constexpr int DPP_ROW = 0;
#else
constexpr int DPP_ROW = 16;
#endif
template <int N, bool SELECT = false>
__device__ __forceinline__ bool lanes_factor(double (&row)[N], double &b, double &dinv, int lane) {
    if constexpr (N <= DPP_ROW) return rows16_factor<N, SELECT>(row, b, dinv, lane);
    else return rows_factor<N>(row, b, dinv, lane);
}
template <int N>
__device__ __forceinline__ void lanes_forward(const double (&row)[N], double &b, int lane) {
    if constexpr (N <= DPP_ROW) rows16_forward<N>(row, b, lane);
    else rows_forward<N>(row, b, lane);
}
template <int N, bool SELECT = false>
__device__ __forceinline__ double lanes_backsub_lane(const double (&row)[N], double b, double dinv, int lane) {
    if constexpr (N <= DPP_ROW) return rows16_backsub_lane<N, SELECT>(row, b, dinv, lane);
    else return rows_backsub_lane<N>(row, b, dinv, lane);
}

// ---- v_mfma_f64_4x4x4_4b_f64: four INDEPENDENT 4 x 4 x 4 products D_b = A_b B_b + C_b (b = 0 .. 3) per instruction, one double per
// lane and operand.  Lane maps as probed on the device with index-coded operands (tests/wavecheck/mfmablocks.hip,
// tests/test_mfma_blocks_gpu.py; they are NOT those of the other data types): with block b = (lane >> 2) & 3 on every operand,
//   A: lane 16 k + 4 b + i holds A_b[i][k]      B: lane 16 k + 4 b + j holds B_b[k][j]      C / D: lane 16 i + 4 b + j holds D_b[i][j]
// i.e. `lane & 3` is the row of A and the column of B and D, `lane >> 4` is k on A and B and the row on C / D.  The host model sums
// k = 0 .. 3 in order by fused multiply-adds starting from C.
constexpr int mb_block(int lane) { return (lane >> 2) & 3; }
constexpr int mb_minor(int lane) { return lane & 3; }
constexpr int mb_major(int lane) { return lane >> 4; }
__device__ __forceinline__ double mfma_blocks(double a, double b, double c) {
#ifdef TMPC_HOST_SIM
    sim::Slot s{};
    s.d[0] = a;
    s.d[1] = b;
    const sim::Slot *all = sim::wave_meet(sim::OP_MFMA, s);
    const int l = sim::cur_lane(), base = 4 * mb_block(l), i = mb_major(l), j = mb_minor(l);
    double acc = c;
    for (int k = 0; k < 4; ++k) acc = std::fma(all[16 * k + base + i].d[0], all[16 * k + base + j].d[1], acc);
    return acc;
#else
    return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
#endif
}

// The product of sweep A's dense pass on those blocks:
//          [ G'DG   ]     [ (D.G)' ]
//          [ (G't)' ]  =  [  t'    ]  G         NV + 1 rows by NV columns, the NV x NV part symmetric
// needs the 4 x 4 blocks (I, J), J <= I, of its lower triangle only -- six of them for NV = 11, two instructions per k-step, where one
// v_mfma_f64_16x16x4_f64 computes the sixteen blocks of a whole tile in four times an instruction's time.
// Gt: the functionals row-major in LDS, [4 nks + 4][LDG]; column NV holds ONE in the rows of the functionals, and the four rows behind
// the last functional are zero.  dtw: (D, t) of functional f at dtw[2 f], dtw[2 f + 1], with eight more readable doubles behind the last.
// k-step ks multiplies the functionals 4 ks .. 4 ks + 3: the lane reads f = 4 ks + (lane >> 4).  Its A entry is D_f g_f[row] -- and
// t_f g_f[NV] = t_f on row NV: the lane picks D or t by the ADDRESS it reads, a multiply and no select --, its B entry g_f[column].
// Blocks to instructions: see GdgBlocks::slotq.  Two k-steps are in flight -- the operands of step ks + 1 are on their way while step ks
// multiplies; the look-ahead reads k-step nks at most and never multiplies it -- and even and odd steps accumulate into registers of
// their own, so that successive matrix instructions do not wait for each other's result.  Four k-steps per trip of the loop: the lane's
// addresses (one per operand and instruction: the rows and columns of its blocks differ from lane to lane) are bumped once per trip.
// The result goes to mt ([NV][LDM]) as BOTH triangles from the lower one (equal bit for bit), row NV to gdr[0 .. NV).
// An LDS address the compiler takes as it is: one 32-bit register, the k-steps of a trip at immediate offsets from it.  (Left to itself it
// keeps the arrays' common base and adds the array's offset in the workgroup's LDS -- a literal beyond the 64 KiB an immediate reaches --
// in front of every load: 26 additions per trip of the loop below instead of 6.)
#ifdef TMPC_HOST_SIM
typedef const double *lds_cptr;
__device__ __forceinline__ lds_cptr lds_opaque(const double *p) { return p; }
#else
typedef const __attribute__((address_space(3))) double *lds_cptr;
__device__ __forceinline__ lds_cptr lds_opaque(const double *p) {
    unsigned a = static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_cptr)p));
    asm("" : "+v"(a));
    return reinterpret_cast<lds_cptr>(static_cast<uintptr_t>(a));
}
#endif
template <int NV>
struct GdgBlocks {
    static constexpr int NBR = (NV + 1 + 3) / 4, NBC = (NV + 3) / 4;             // block rows (NV + 1 rows), block columns
    static constexpr int first(int I) { return I <= NBC ? I * (I + 1) / 2 : NBC * (NBC + 1) / 2 + (I - NBC) * NBC; }      // index of block (I, 0)
    static constexpr int NBLK = first(NBR);
    static constexpr int NI = (NBLK + 3) / 4;                                   // instructions per k-step
    static constexpr int brow(int q) { int I = 0; while (first(I + 1) <= q) ++I; return I; }
    static constexpr int bcol(int q) { return q - first(brow(q)); }
    // block of slot bs of instruction n, row-major in the lower triangle: the LAST instruction holds the last four blocks, so that the
    // blocks of the last block row -- the only ones with row NV -- share as few instructions as can be; the spare slots are the first of
    // instruction 0 (q < 0: they repeat block 0 and are not stored)
    static constexpr int slotq(int n, int bs) { return NBLK - 4 * (NI - n) + bs; }
    static constexpr int clampq(int q) { return q < 0 ? 0 : q; }
    static constexpr bool takes_t(int n) { return brow(clampq(slotq(n, 3))) == NV / 4; }
    static constexpr bool any_plain() { for (int n = 0; n < NI; ++n) if (!takes_t(n)) return true; return false; }
};
template <int NV, int LDG, int LDM>
__device__ __forceinline__ void gdg_blocks(const double *Gt, int nks, const double *dtw, double *mt, double *gdr, int lane) {
    using GB = GdgBlocks<NV>;
    constexpr int NI = GB::NI;
    static_assert(4 * GB::NBR <= LDG, "the rows of the last block row read columns of G that are staged");
    const int kq = mb_major(lane), bs = mb_block(lane), r = mb_minor(lane);
    // first row / column of the lane's block in instruction n
    int r0[NI], c0[NI];
    static_for_n<NI>([&](auto n_) {
        constexpr int n = decltype(n_)::value;
        constexpr int q0 = GB::clampq(GB::slotq(n, 0)), q1 = GB::clampq(GB::slotq(n, 1)), q2 = GB::clampq(GB::slotq(n, 2)), q3 = GB::clampq(GB::slotq(n, 3));
        r0[n] = 4 * (bs == 0 ? GB::brow(q0) : bs == 1 ? GB::brow(q1) : bs == 2 ? GB::brow(q2) : GB::brow(q3));
        c0[n] = 4 * (bs == 0 ? GB::bcol(q0) : bs == 1 ? GB::bcol(q1) : bs == 2 ? GB::bcol(q2) : GB::bcol(q3));
    });
    double acc[2][NI];
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int n = 0; n < NI; ++n) acc[h2][n] = 0.0;
    // the multiplier of the A entry (D, or t on row NV), the A entry's g and the B entry's g: one address each per instruction
    lds_cptr pd = lds_opaque(dtw + 2 * kq), px[NI], pa[NI], pb[NI];
#pragma unroll
    for (int n = 0; n < NI; ++n) {
        px[n] = GB::takes_t(n) ? lds_opaque(dtw + 2 * kq + (r0[n] + r == NV ? 1 : 0)) : pd;
        pa[n] = lds_opaque(Gt + kq * LDG + r + r0[n]);
        pb[n] = lds_opaque(Gt + kq * LDG + r + c0[n]);
    }
    struct Ops { double D, x[NI], ga[NI], gb[NI]; };
    auto fetch = [&](Ops &o, auto u_) {                 // the k-step u steps behind the addresses
        constexpr int u = decltype(u_)::value;
        if constexpr (GB::any_plain()) o.D = pd[8 * u];
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            if (GB::takes_t(n)) o.x[n] = px[n][8 * u];
            o.ga[n] = pa[n][4 * LDG * u];
            o.gb[n] = pb[n][4 * LDG * u];
        }
    };
    auto bump = [&](auto u_) {
        constexpr int u = decltype(u_)::value;
        pd += 8 * u;
#pragma unroll
        for (int n = 0; n < NI; ++n) { px[n] += 8 * u; pa[n] += 4 * LDG * u; pb[n] += 4 * LDG * u; }
    };
    auto multiply = [&](auto h_, const Ops &o) {
        constexpr int h2 = decltype(h_)::value;
        static_for_n<NI>([&](auto n_) {
            constexpr int n = decltype(n_)::value;
            const double a = (GB::takes_t(n) ? o.x[n] : o.D) * o.ga[n];
            acc[h2][n] = mfma_blocks(a, o.gb[n], acc[h2][n]);
        });
    };
    constexpr std::integral_constant<int, 0> c_0{};
    constexpr std::integral_constant<int, 1> c_1{};
    constexpr std::integral_constant<int, 2> c_2{};
    constexpr std::integral_constant<int, 3> c_3{};
    constexpr std::integral_constant<int, 4> c_4{};
    {
        Ops o0, o1;
        fetch(o0, c_0);
        int ks = 0;
        for (; ks + 3 < nks; ks += 4) {
            fetch(o1, c_1);
            multiply(c_0, o0);
            fetch(o0, c_2);
            multiply(c_1, o1);
            fetch(o1, c_3);
            multiply(c_0, o0);
            bump(c_4);
            fetch(o0, c_0);                             // (past the end: zero rows, never multiplied)
            multiply(c_1, o1);
        }
        if (ks + 1 < nks) {
            fetch(o1, c_1);
            multiply(c_0, o0);
            fetch(o0, c_2);
            multiply(c_1, o1);
            ks += 2;
        }
        if (ks < nks) multiply(c_0, o0);
    }
    // C / D: the lane holds row `lane >> 4`, column `lane & 3` of its block
    static_for_n<NI>([&](auto n_) {
        constexpr int n = decltype(n_)::value;
        const double v = acc[0][n] + acc[1][n];
        const int row = r0[n] + kq, col = c0[n] + r;
        const bool mine = GB::slotq(n, 0) + bs >= 0;        // (not a spare block)
        if (mine && row < NV && col <= row) {
            mt[row * LDM + col] = v;
            if (col < row) mt[col * LDM + row] = v;
        }
        if (mine && row == NV && col < NV) gdr[col] = v;
    });
    lds_fence();
}

}  // namespace wv
}  // namespace tmpc
