// Closed loop of the regulator MPCs on the device (include/tmpc.h: tmpc_reg_run): the loop of the reference's
// Example_of_Tube_Regulator_MPC.py, batched over B trajectories.  Per time step the host enqueues the solve launch over all
// trajectories (the wave or block kernel, as for any solve) and ONE launch of reg_step_kernel behind it, which for every
// trajectory
//   applies   u_t = u_nom_0 - K (x_t - x_nom_0)        (the reference's sign: K is the LQR gain of u = -K x; plain: u_t = u_nom_0)
//   checks    x_t in X, u_t in U, x_t - x_nom_0 in Z   (the rows of each set spread over the lanes)
//   sums      x_t'Q x_t + u_t'R u_t
//   updates   x_{t+1} = A x_t + B u_t + w_t           (w: host array, or the Philox stream of tmpc_mc_set_device_rng; A, B: the model's, or
//                                                      the trajectory's own plant of tmpc_mc_set_plant_models -- the solve keeps the model's)
// and writes x_{t+1} in place, where the next solve reads its x_k.
//
// Form as mc_step_wave (tmpc_mc_step.hpp): one wavefront per trajectory, component i of every state-sized vector on lane i,
// the vectors a matrix-vector product reads handed round through LDS (broadcast reads), wave-uniform scalars, no private memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tmpc_device.hpp"
#include "tmpc_mc_step.hpp"

namespace tmpc {

namespace {

using mcstep::MAXN;
using mcstep::mc_fence;
using mcstep::philox4x64;
using mcstep::u01;

constexpr int RWAVE = 64;
constexpr int REG_WPB = 4;           // trajectories (waves) per workgroup
enum { R_X = 0, R_E, R_U, R_COUNT };

// Row r of {H v <= h} violated by more than polytope's abs_tol, for any row of the set (rows over the lanes)
__device__ __forceinline__ bool set_violated(const double *__restrict__ H, const double *__restrict__ h, int rows, int dim,
                                             const double *v, int lane) {
    int out = 0;
    for (int r = lane; r < rows; r += RWAVE) {
        double a = -h[r];
        for (int i = 0; i < dim; ++i) a += H[r * dim + i] * v[i];
        out |= (a > 1e-7);
    }
    return __any(out);
}

__global__ __launch_bounds__(RWAVE * REG_WPB) void reg_step_kernel(const RegModel m, const RegState st, const int t, const int T,
                                                                     const int64_t B, const double *__restrict__ u_nom,
                                                                     const double *__restrict__ x_nom0,
                                                                     const int32_t *__restrict__ status, const int32_t *__restrict__ iters) {
    __shared__ double sh[REG_WPB][R_COUNT][MAXN];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = static_cast<int64_t>(blockIdx.x) * REG_WPB + wave;
    if (b >= B) return;
    double (&S)[R_COUNT][MAXN] = sh[wave];
    const int nx = m.nx, nu = m.nu, N = m.N;
    const bool lx = lane < nx, lu = lane < nu;
    const bool cap = b == st.cap_index;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const double x_l = lx ? st.x[b * nx + lane] : 0.0;
    if (st.fail_step[b] >= 0) {                  // frozen since an infeasible solve: the state stays, nothing accumulates
        if (cap) {
            if (lx) { st.cap_x[(t + 1) * nx + lane] = x_l; st.cap_xn[t * nx + lane] = nanv; }
            if (lu) st.cap_u[t * nu + lane] = nanv;
        }
        return;
    }
    const int stat = status[b];
    if (lane == 0) {
        st.iters_sum[b] += iters[b];
        if (stat != TMPC_STATUS_OPTIMAL) st.not_optimal[b] += 1;
        if (stat >= TMPC_STATUS_INFEASIBLE) st.fail_step[b] = t;
    }
    if (stat >= TMPC_STATUS_INFEASIBLE) {
        if (cap) {
            if (lx) { st.cap_x[(t + 1) * nx + lane] = x_l; st.cap_xn[t * nx + lane] = nanv; }
            if (lu) st.cap_u[t * nu + lane] = nanv;
        }
        return;
    }
    // ---- input: u_t = u_nom_0 - K (x_t - x_nom_0)
    const double xn_l = lx ? x_nom0[b * nx + lane] : 0.0;
    if (lane < MAXN) { S[R_X][lane] = x_l; S[R_E][lane] = x_l - xn_l; }
    mc_fence();
    double u_l = 0.0;
    if (lu) {
        u_l = u_nom[b * N * nu + lane];
        if (m.tube)
            for (int i = 0; i < nx; ++i) u_l -= m.K[lane * nx + i] * S[R_E][i];
    }
    if (lane < MAXN) S[R_U][lane] = u_l;
    mc_fence();
    // ---- statistics
    if (lane == 0) {
        double c = 0.0;
        for (int i = 0; i < nx; ++i) {
            double qi = 0.0;
            for (int j = 0; j < nx; ++j) qi += m.Q[i * nx + j] * S[R_X][j];
            c += S[R_X][i] * qi;
        }
        for (int i = 0; i < nu; ++i) {
            double ri = 0.0;
            for (int j = 0; j < nu; ++j) ri += m.R[i * nu + j] * S[R_U][j];
            c += S[R_U][i] * ri;
        }
        st.cost[b] += c;
    }
    if (m.rX > 0 && set_violated(m.HX, m.hX, m.rX, nx, S[R_X], lane) && lane == 0) st.x_viol[b] += 1;
    if (m.rU > 0 && set_violated(m.HU, m.hU, m.rU, nu, S[R_U], lane) && lane == 0) st.u_viol[b] += 1;
    if (m.rZ > 0 && set_violated(m.HZ, m.hZ, m.rZ, nx, S[R_E], lane) && lane == 0) st.tube_viol[b] += 1;
    // ---- disturbance: host array, or component `lane` of the Philox stream (block 0 = [theta, gamma, w_0, w_1], block j >= 1 =
    // w_{4j-2} .. w_{4j+1}: the draws of tmpc_mc_run, mcstep::mc_draws)
    double w_l = 0.0;
    if (lx) {
        if (st.w != nullptr) {
            w_l = st.w[(b * T + t) * nx + lane];
        } else if (st.rng_on) {
            unsigned long long r[4];
            const int idx = lane + 2;
            philox4x64(static_cast<unsigned long long>(t), static_cast<unsigned long long>(idx >> 2), st.rng_seed,
                       static_cast<unsigned long long>(st.rng_first + b), r);
            const unsigned long long rc = (idx & 3) == 0 ? r[0] : ((idx & 3) == 1 ? r[1] : ((idx & 3) == 2 ? r[2] : r[3]));
            w_l = st.w_bound[lane] * (2.0 * u01(rc) - 1.0);
        }
    }
    // ---- plant
    double xp_l = 0.0;
    if (lx) {
        // row `lane` of the model's (A, B), or of the trajectory's own plant [A_b | B_b] (tmpc_mc_set_plant_models): one arithmetic path
        const double *ap = m.A + lane * nx, *bp = m.B + lane * nu;
        if (st.plant_lin != nullptr) {
            ap = st.plant_lin + (b * nx + lane) * static_cast<int64_t>(nx + nu);
            bp = ap + nx;
        }
        double v = 0.0;
        for (int k = 0; k < nx; ++k) v += ap[k] * S[R_X][k];
        for (int j = 0; j < nu; ++j) v += bp[j] * S[R_U][j];
        xp_l = v + w_l;
        st.x[b * nx + lane] = xp_l;
    }
    if (cap) {
        if (lx) { st.cap_x[(t + 1) * nx + lane] = xp_l; st.cap_xn[t * nx + lane] = xn_l; }
        if (lu) st.cap_u[t * nu + lane] = u_l;
    }
}

}  // namespace

hipError_t launch_reg_step(const RegModel &m, const RegState &st, int t, int T, int64_t B, const double *u_nom, const double *x_nom0,
                           const int32_t *status, const int32_t *iters, hipStream_t stream) {
    if (m.nx > MAXN || m.nu > MAXN) return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>((B + REG_WPB - 1) / REG_WPB);
    hipLaunchKernelGGL(reg_step_kernel, dim3(blocks), dim3(RWAVE * REG_WPB), 0, stream, m, st, t, T, B, u_nom, x_nom0, status, iters);
    return hipGetLastError();
}

}  // namespace tmpc
