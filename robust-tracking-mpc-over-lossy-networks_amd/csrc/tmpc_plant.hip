// A plant per trajectory for the tracking loops (gfx950): one launch advances B plants by one sampling period,
//
//   x_plus[b] = f_b(x[b], u[b]) + w[b]
//
// behind the state-machine launch of a stepped session (include/tmpc.h: tmpc_mc_run_plants, tmpc_plant_step_device).  The session cuts the
// closed loop exactly at the plant -- it takes x_t after the solve and returns u_t -- so the plants of a family live here and no kernel of
// the closed-loop state machines knows about them.
//
//   plant_cartpole_kernel   one LANE per trajectory: the lane's seven parameters, the four states and the RK4 stages in registers (the
//                           work is serial and scalar, as in west_rollout_kernel).  The input is held over the period; the update is
//                           spelled as mcstep::mc_step_impl spells it, so that a nominal row rounds like the loop's own plant wherever the
//                           compiler contracts alike.  Optionally the physics-rate tracking error of the period.  No LDS, no private memory.
//   plant_linear_kernel     one lane per (trajectory, state row): the lane reads one contiguous row [A_b[i, :] | B_b[i, :]] and sums in the
//                           order of the loop's own linear plant: w_i, the A terms by ascending k, the B terms by ascending j.
//
// The disturbance is an array, the Philox stream of tmpc_mc_set_device_rng (exactly tmpc_mc_run's numbers: mcstep::mc_draws), or nothing.
// Lanes beyond the batch return before any load.
#ifdef TMPC_HOST_SIM
#include "hip_sim.hpp"      // tests/wavesim: this very source compiled for the CPU under sanitizers (never in the product)
#else
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "tmpc_device.hpp"
#include "tmpc_launch.hpp"
#include "tmpc_mc_step.hpp"
#include "tmpc_plant.hpp"

namespace tmpc {

namespace {

using ull = unsigned long long;

constexpr int PLANT_CART_THREADS = 64;       // one wave per workgroup, as the W estimate's rollout
constexpr int PLANT_LIN_THREADS = 256;

// the grid of a launch: every workgroup on the host execution model (launch_grid runs workgroup 0 alone there)
template <class... P, class... A>
hipError_t plant_launch(void (*kernel)(P...), unsigned blocks, unsigned threads, hipStream_t stream, A &&...args) {
#ifdef TMPC_HOST_SIM
    (void)stream;
    for (unsigned b = 0; b < blocks; ++b) {
        sim::Dim3 bi, gd;
        bi.x = b;
        gd.x = blocks;
        sim_rendezvous_total += sim::run_block(static_cast<int>(threads), 0, bi, gd, [&]() { kernel(static_cast<P>(args)...); });
    }
    return hipSuccess;
#else
    return launch_grid(kernel, blocks, threads, 0, stream, static_cast<A &&>(args)...);
#endif
}

// w_bound (2 u - 1) of one Philox word, the product rounded on its own as in mcstep::mc_draws
__device__ __forceinline__ double plant_w(double bound, ull word) { return bound * (2.0 * mcstep::u01(word) - 1.0); }

// x + w in one rounding of its own: w is a number of the caller's (or of the generator), not a product to be fused into the sum
__device__ __forceinline__ double plant_add(double x, double w) {
#pragma clang fp contract(off)
    return x + w;
}

__global__ __launch_bounds__(PLANT_CART_THREADS) void plant_cartpole_kernel(PlantStep a) {
    const int64_t b = static_cast<int64_t>(blockIdx.x) * PLANT_CART_THREADS + threadIdx.x;
    if (b >= a.B) return;
    double y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = a.x[b * 4 + i];
    if (a.hold != nullptr && a.hold[b]) {
        // the trajectory has stopped (McState::dead): its state stays, its physics-rate error is NaN (tmpc_mc_get_physics_error)
#pragma unroll
        for (int i = 0; i < 4; ++i) a.x_plus[b * 4 + i] = y[i];
        if (a.err2_phys) a.err2_phys[b] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    double par[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) par[i] = a.models[b * 7 + i];
    const double u0 = a.u[b];
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    if (a.w != nullptr) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = a.w[b * a.w_stride + i];
    } else if (a.rng_on) {
        // block 0 of the step holds [theta, gamma, w_0, w_1], block 1 holds w_2 .. w_5
        const ull key1 = static_cast<ull>(a.rng_first + b);
        ull r0[4], r1[4];
        mcstep::philox4x64(static_cast<ull>(a.t), 0ull, a.rng_seed, key1, r0);
        mcstep::philox4x64(static_cast<ull>(a.t), 1ull, a.rng_seed, key1, r1);
        w[0] = plant_w(a.w_bound[0], r0[2]);
        w[1] = plant_w(a.w_bound[1], r0[3]);
        w[2] = plant_w(a.w_bound[2], r1[0]);
        w[3] = plant_w(a.w_bound[3], r1[1]);
    }
    // the reference the solve of this step used: the schedule's row, or the legacy position reference
    const bool phys = a.err2_phys != nullptr, full_ref = a.ref_tab != nullptr;
    double rp[4] = {0.0, 0.0, 0.0, 0.0};
    if (phys && full_ref) {
        const double *row = a.ref_tab + (static_cast<int64_t>(a.ref_id[b]) * a.ref_T + a.t) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) rp[i] = row[i];
    }
    const double ref_t = a.ref_t;
    const double dt = par[6] / a.substeps;
    double aphys = 0.0;
    // zero-order hold of u over the sampling period, RK4 at the physics rate: the hold of mcstep::mc_step_impl, operation for operation
    for (int sstep = 0; sstep < a.substeps; ++sstep) {
        double k1[4], k2[4], k3[4], k4[4], yt[4];
        if (phys) {
            if (full_ref) {
                // (the legacy sum as the compiler contracts it, spelled out: see mc_step_impl)
                double e = (y[0] - rp[0]) * (y[0] - rp[0]);
#pragma unroll
                for (int i = 1; i < 4; ++i) e = fma(y[i] - rp[i], y[i] - rp[i], e);
                aphys += e;
            } else aphys += (y[0] - ref_t) * (y[0] - ref_t) + y[1] * y[1] + y[2] * y[2] + y[3] * y[3];
        }
        mcstep::cartpole_rhs(par, y, u0, k1);
#pragma unroll
        for (int i = 0; i < 4; ++i) yt[i] = y[i] + 0.5 * dt * k1[i];
        mcstep::cartpole_rhs(par, yt, u0, k2);
#pragma unroll
        for (int i = 0; i < 4; ++i) yt[i] = y[i] + 0.5 * dt * k2[i];
        mcstep::cartpole_rhs(par, yt, u0, k3);
#pragma unroll
        for (int i = 0; i < 4; ++i) yt[i] = y[i] + dt * k3[i];
        mcstep::cartpole_rhs(par, yt, u0, k4);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] += dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a.x_plus[b * 4 + i] = plant_add(y[i], w[i]);
    if (phys) a.err2_phys[b] += aphys;
}

__global__ __launch_bounds__(PLANT_LIN_THREADS) void plant_linear_kernel(PlantStep a) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * PLANT_LIN_THREADS + threadIdx.x;
    const int nx = a.nx, nu = a.nu;
    if (g >= a.B * nx) return;
    const int64_t b = g / nx;
    const int i = static_cast<int>(g - b * nx);
    const double *__restrict__ xb = a.x + b * nx;
    if (a.hold != nullptr && a.hold[b]) {
        a.x_plus[g] = xb[i];
        return;
    }
    double v = 0.0;
    if (a.w != nullptr) {
        v = a.w[b * a.w_stride + i];
    } else if (a.rng_on) {
        const int idx = i + 2;               // block j = 0: [theta, gamma, w_0, w_1]; block j >= 1: w_{4j-2} .. w_{4j+1}
        ull r[4];
        mcstep::philox4x64(static_cast<ull>(a.t), static_cast<ull>(idx >> 2), a.rng_seed, static_cast<ull>(a.rng_first + b), r);
        const ull rc = (idx & 3) == 0 ? r[0] : ((idx & 3) == 1 ? r[1] : ((idx & 3) == 2 ? r[2] : r[3]));
        v = plant_w(a.w_bound[i], rc);
    }
    const double *__restrict__ row = a.models + g * (nx + nu);
    const double *__restrict__ ub = a.u + b * nu;
    for (int k = 0; k < nx; ++k) v += row[k] * xb[k];
    for (int j = 0; j < nu; ++j) v += row[nx + j] * ub[j];
    a.x_plus[g] = v;
}

}  // namespace

hipError_t launch_plant_step(const PlantStep &a, hipStream_t stream) {
    if (a.B < 1 || !a.models || !a.x || !a.u || !a.x_plus || (a.rng_on && !a.w && !a.w_bound)) return hipErrorInvalidValue;
    if (a.kind == TMPC_PLANT_CARTPOLE) {
        if (a.nx != 4 || a.nu != 1 || a.substeps < 1) return hipErrorInvalidValue;
        if (a.err2_phys && a.ref_tab && (!a.ref_id || a.t < 0 || a.t >= a.ref_T)) return hipErrorInvalidValue;
        const unsigned blocks = static_cast<unsigned>((a.B + PLANT_CART_THREADS - 1) / PLANT_CART_THREADS);
        return plant_launch(plant_cartpole_kernel, blocks, PLANT_CART_THREADS, stream, a);
    }
    if (a.kind == TMPC_PLANT_LINEAR) {
        if (a.nx < 1 || a.nx > mcstep::MAXN || a.nu < 1 || a.nu > mcstep::MAXN) return hipErrorInvalidValue;
        const unsigned blocks = static_cast<unsigned>((a.B * a.nx + PLANT_LIN_THREADS - 1) / PLANT_LIN_THREADS);
        return plant_launch(plant_linear_kernel, blocks, PLANT_LIN_THREADS, stream, a);
    }
    return hipErrorInvalidValue;
}

}  // namespace tmpc
