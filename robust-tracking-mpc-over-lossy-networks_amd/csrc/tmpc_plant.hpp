// A family of plants, one per trajectory, advanced by one sampling period per launch (tmpc_plant.hip): what tmpc_loops.cpp and the host
// execution model of tests/wavesim see of it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tmpc {

// x_plus[b] = f_b(x[b], u[b]) + w[b] for B trajectories.  Every pointer is device memory; the optional ones may be nullptr.
struct PlantStep {
    int kind;                            // TMPC_PLANT_CARTPOLE (nx = 4, nu = 1) or TMPC_PLANT_LINEAR (1 <= nx, nu <= 16)
    int nx, nu;
    int substeps;                        // cart-pole: RK4 steps of Th_b / substeps per period
    int64_t B;
    const double *models;                // cart-pole [B][7] rows {M, m, b, I, g, l, Th}; linear [B][nx][nx + nu] rows [A_b[i, :] | B_b[i, :]]
    const double *x, *u;                 // [B][nx], [B][nu]
    double *x_plus;                      // [B][nx]; must not overlap x
    // the disturbance: an array (trajectory b at w + b * w_stride), else the Philox stream of tmpc_mc_set_device_rng -- key
    // (rng_seed, rng_first + b), counter (t, j, 0, 0), w_i = w_bound[i] (2 u - 1) -- else none
    const double *w;
    int64_t w_stride;
    int rng_on, t;
    unsigned long long rng_seed;
    long long rng_first;
    const double *w_bound;               // [nx]  (rng_on)
    const uint8_t *hold;                 // [B] or nullptr: a trajectory with hold[b] != 0 keeps its x (an R-MPC trajectory that has stopped)
    // cart-pole, or nullptr: += the tracking error at the start of every physics step, against the reference of step t -- row t of the
    // trajectory's schedule ref_tab[ref_id[b]] (rows of nx, ref_T per schedule), or without a table [ref_t, 0, 0, 0]; NaN where hold
    double *err2_phys;                   // [B]
    double ref_t;
    const double *ref_tab;
    const int32_t *ref_id;
    int ref_T;
};

// hipErrorInvalidValue for a kind, a shape or a missing pointer the kernels do not cover; enqueues one launch and does not synchronise
hipError_t launch_plant_step(const PlantStep &a, hipStream_t stream);

}  // namespace tmpc
