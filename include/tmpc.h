/*
 * tmpc.h -- C ABI of the MI355X tube-tracking-MPC solve engine (libtmpc_hip.so).
 *
 * Drop-in boundary for ONE hot path of
 * EricssonResearch/Robust-Tracking-MPC-over-Lossy-Networks: the per-timestep QP of
 * TubeTrackingMPC / ExtendedTubeTrackingMPC, batched over independent
 * Monte-Carlo trajectories.  Each entry point names the reference interface it
 * replaces (paths relative to the reference's src/LinearMPCOverNetworks/).
 *
 * Conventions
 *   - plain C, no C++/torch types; every matrix is float64, row-major, dense;
 *   - the caller owns all buffers passed in; the library owns the opaque handle,
 *     its device copies of the problem, its scratch and its HIP streams;
 *   - every function returns 0 on success and a negative TMPC_E_* code otherwise;
 *     tmpc_last_error() gives the message; no C++ exception crosses the boundary;
 *   - a handle is not thread-safe; use one handle per host thread / per GPU.
 */
#ifndef TMPC_H
#define TMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: first cut; 2: projected terminal rows of the packet-received problem (HTP, hTP, rTP); 3: tmpc_lp_batch, TMPC_STATUS_UNBOUNDED;
 * 4: terminal_equality, tmpc_kernel_name; 5: an iterate that hits the iteration cap keeps TMPC_STATUS_MAX_ITER whatever its
 * constraint violation (INFEASIBLE only with a Farkas-type certificate), host-only handles report their kernel path,
 * tmpc_debug_dump_layout (tmpc_debug_dump_lp_layout was added later without a bump: a new export, nothing else changed).
 * Added without a bump: the regulator QPs (tmpc_regulator_problem, tmpc_create_regulator, tmpc_reg_run) -- new exports; tmpc_problem
 * and every tracking handle behave as before (a regulator handle accepts ref == NULL in the solve calls, see below); the
 * disturbance-set estimation (tmpc_estimate_w, tmpc_order_statistics) -- new exports; tmpc_set_call_overlap, tmpc_debug_lane_counters,
 * tmpc_debug_calls_conflict -- new exports (what tmpc_kernel_ms_total adds up for calls that overlap is defined there);
 * tmpc_set_call_lanes / tmpc_get_call_lanes, tmpc_debug_lane_counters_n and the policy diagnostics next to them -- new exports
 * (tmpc_debug_lane_counters now counts by the parity of the lane changes: with two lanes, what it was) */
#define TMPC_ABI_VERSION 5

/* error codes (function return values) */
#define TMPC_OK            0
#define TMPC_E_INVALID    -1   /* bad argument / inconsistent problem description      */
#define TMPC_E_UNSUPPORTED -2  /* problem size outside what the compiled kernels cover */
#define TMPC_E_DEVICE     -3   /* HIP runtime error                                     */
#define TMPC_E_NOMEM      -4

/* per-instance solver status (status[] output), mirroring what the reference reads
 * from cvxpy: "optimal" / "optimal_inaccurate" / "infeasible" / failure -> None
 * (TubeTrackingMPC.py:185-194) */
#define TMPC_STATUS_OPTIMAL     0
#define TMPC_STATUS_MAX_ITER    1   /* iteration cap hit; last iterate returned          */
#define TMPC_STATUS_INFEASIBLE  2   /* no x satisfies the constraints for this (x_k)     */
#define TMPC_STATUS_NUMERICAL   3
#define TMPC_STATUS_UNBOUNDED   4   /* tmpc_lp_batch only: the objective is unbounded on the set */

/*
 * Problem description: everything `TubeTrackingMPC.generate_optimization_problem`
 * (TubeTrackingMPC.py:104-156) and, when `extended` is set,
 * `ExtendedTubeTrackingMPC.generate_optimization_problem_when_packet_received`
 * (TubeTrackingMPC.py:253-299) close over.
 *
 *   model     x+ = A x + B u                      A: nx*nx   B: nx*nu     (RegulatorMPC.py:13-14)
 *   weights   Q: nx*nx  R: nu*nu                                          (RegulatorMPC.py:24-25)
 *             P: nx*nx  terminal weight                                   (TubeRegulatorMPC.py:23)
 *             T: nx*nx  steady-state offset weight = 10 P                 (TubeTrackingMPC.py:27)
 *   gains     K: nu*nx steady-state LQR gain, K_anc: nu*nx ancillary gain (TubeTrackingMPC.py:229-240)
 *   sets      {Hx x <= hx}   rx rows, tightened state set  Xc            (TubeTrackingMPC.py:112)
 *             {Hu u <= hu}   ru rows, tightened input set  Uc            (TubeTrackingMPC.py:110)
 *             {HT [x_N; x_bar; u_bar] <= hT}  rT rows, terminal set Xf in R^(2nx+nu) (TubeTrackingMPC.py:114,149)
 *             {HZ e <= hZ}   rZ rows, mRPI set Z; used iff fixed_x0 == 0  (TubeTrackingMPC.py:130-132)
 *             {HZW e <= hZW} rZW rows, Z (-) W; used iff extended != 0    (TubeTrackingMPC.py:266-278)
 *             {HTP [x_bar; u_bar] <= hTP} rTP rows (optional, extended only): the terminal row block of the
 *                            packet-received problem (TubeTrackingMPC.py:293) with its free auxiliaries
 *                            eliminated, i.e. proj(Xf) on the steady-state subspace -- see below
 *
 * fixed_x0 : 1 -> x_0 == x_k (TubeTrackingMPC.py:127); 0 -> HZ (x_k - x_0) <= hZ (TubeTrackingMPC.py:132).
 * extended : 1 -> a second QP ("variant 1") is prepared for instances whose
 *            previous plant packet arrived (gamma_t == 1, TubeTrackingMPC.py:312).
 * literal_terminal_row : 1 (default) reproduces TubeTrackingMPC.py:293 literally: in
 *            variant 1 the terminal inequality is written on x_mpc[:,N] and u_bar of the
 *            *base* problem, i.e. on free auxiliary variables; 0 uses the variant's own
 *            x_N and u_bar instead.
 *            The auxiliaries are not priced, so line :293 only says x_bar in proj_xbar(Xf).  When the
 *            caller supplies that projection (HTP, hTP; LinearMPCOverNetworks/utils_polytope.py:
 *            eliminate_terminal_auxiliaries computes it exactly at set-up time) the auxiliaries are
 *            dropped and the QP stays strictly convex: the minimiser in (x, u, x_bar, u_bar) is the
 *            same.  Without it (rTP == 0) the auxiliaries are kept with a vanishing weight
 *            2e-6 min(diag R) |aux|^2; that problem is badly conditioned and its solution is only
 *            reliable to ~1e-5.
 * tol      : relative primal-residual / duality-gap level at which the interior-point
 *            phase hands over to the exact active-set refinement; <= 0 selects the
 *            default 1e-7 (tightened by 1e-2 and retried whenever the refinement
 *            cannot certify its active set).
 * max_iter : interior-point iteration cap; <= 0 selects the default 60.
 */
typedef struct tmpc_problem {
    int32_t nx, nu, N;
    int32_t rx, ru, rT, rZ, rZW;
    int32_t fixed_x0, extended, literal_terminal_row;
    int32_t max_iter;
    double  tol;
    const double *A, *B, *Q, *R, *P, *T, *K, *K_anc;
    const double *Hx, *hx, *Hu, *hu, *HT, *hT, *HZ, *hZ, *HZW, *hZW;
    const double *HTP, *hTP;    /* rTP x (nx+nu), rTP; may be NULL */
    int32_t rTP;
    int32_t terminal_equality;  /* 1: x_N == x_bar instead of a terminal set (TrackingMPC.py:105-107: the tracking MPC
                                 * before setup_optimization()); needs rT == 0.  The nx equalities are eliminated at set-up
                                 * like the dynamics and the steady-state equation. */
} tmpc_problem;

typedef struct tmpc_handle tmpc_handle;

/* ABI version of the loaded library (compare with TMPC_ABI_VERSION). */
int tmpc_abi_version(void);

/* Last error message of `h`, or of the last failed tmpc_create when h == NULL. */
const char *tmpc_last_error(const tmpc_handle *h);

/*
 * Replaces generate_optimization_problem(fixed_initial_state)
 * (TubeTrackingMPC.py:104-156) [+ :253-299 when p->extended]: condenses the QP(s)
 * once, uploads them to HIP device `device`, allocates scratch.
 * device < 0 builds a host-only handle: the condensed problem can be inspected
 * (tmpc_get_dims / tmpc_get_condensed) but every solve call fails with TMPC_E_DEVICE --
 * there is no CPU solve path in this library.
 */
int tmpc_create(const tmpc_problem *p, int device, tmpc_handle **out);

void tmpc_destroy(tmpc_handle *h);

/*
 * The regulator QPs -- the root of the reference's class chain: RegulatorMPC (RegulatorMPC.py:45-91, "bring the state to the
 * origin") and, with `tube` set, the tube MPC of Mayne, Seron and Rakovic 2005, TubeRegulatorMPC (TubeRegulatorMPC.py:109-143).
 *
 *   model     x+ = A x + B u                      A: nx*nx   B: nx*nu
 *   weights   Q: nx*nx  R: nu*nu  stage cost x'Qx + u'Ru, i = 0 .. N-1
 *             P: nx*nx  terminal weight x_N'P x_N  (tube only; the plain regulator has none, NULL allowed)
 *   gain      K: nu*nx  ancillary gain of u = u_nom_0 - K (x - x_nom_0) (the LQR gain, u = -K x); tmpc_reg_run applies it.
 *             Tube: required.  Plain: not read (x_nom_0 = x), NULL allowed
 *   sets      {Hx x <= hx}   rx rows on x_0 .. x_{N-1}   (tube: the tightened Xc)   rx = 0: no state constraint (X = None)
 *             {Hu u <= hu}   ru rows on u_0 .. u_{N-1}   (tube: the tightened Uc)   ru = 0: no input constraint (U = None)
 *             {Hf x <= hf}   rf rows on x_N, terminal set Xf (tube only; rf = 0: none)
 *             {HZ e <= hZ}   rZ rows, the tube cross-section Z: HZ (x_k - x_0) <= hZ (tube only, rZ > 0 required)
 *   tube      0: plain regulator, z = [u_0 .. u_{N-1}] with x_0 = x_k (the rows Hx x_0 <= hx then depend on x_k only and are
 *                checked once per instance: a state outside X is INFEASIBLE)
 *             1: tube regulator, z = [u_0 .. u_{N-1} | x_0] with x_0 free
 *   tol, max_iter: as in tmpc_problem.
 * A row count > 0 needs both of its arrays.
 */
typedef struct tmpc_regulator_problem {
    int32_t nx, nu, N;
    int32_t rx, ru, rf, rZ;
    int32_t tube;
    int32_t max_iter;
    double  tol;
    const double *A, *B, *Q, *R, *P, *K;
    const double *Hx, *hx, *Hu, *hu, *Hf, *hf, *HZ, *hZ;
} tmpc_regulator_problem;

/*
 * Replaces RegulatorMPC.generate_optimization_problem / TubeRegulatorMPC.generate_optimization_problem: condenses the QP
 * (min 1/2 z'Hz + (F1 x_k)'z  s.t.  G z <= g0 + E x_k; F2 = 0, no steady-state block) and returns an ordinary handle: the
 * solve calls, tmpc_set_kernel_path, tmpc_kernel_name, tmpc_get_dims / _condensed / _factoring and tmpc_destroy take it as
 * they take a tracking handle (device < 0: host-only, as in tmpc_create).  Same limits as tmpc_create (0 < nx <= 16).
 * In tmpc_solve_batch[_device] on a regulator handle:  ref may be NULL and is ignored; xu_ss must be NULL; variant must be
 * NULL; x_nom0 receives x_0 (the decision variable of the tube regulator, x_k for the plain one); x_nom the predicted
 * trajectory x_0 .. x_N.  tmpc_mc_run / tmpc_mc_replay refuse a regulator handle (its loop is tmpc_reg_run).
 */
int tmpc_create_regulator(const tmpc_regulator_problem *p, int device, tmpc_handle **out);

/*
 * Device-resident closed loop of a regulator handle -- the loop of the reference's Example_of_Tube_Regulator_MPC.py (and of
 * Example_of_Regulator_MPC.py with K = 0, w = 0) -- for B independent trajectories and T time steps.  Per step, on the
 * handle's stream: one solve launch over all trajectories, then one launch of the step kernel (csrc/tmpc_reg.hip), which per
 * trajectory applies  u_t = u_nom_0 - K (x_t - x_nom_0)  (plain: u_t = u_nom_0), updates  x_{t+1} = A x_t + B u_t + w_t,
 * accumulates the statistics and writes the next solve's x_k in place.  Nothing returns to the host until the statistics.
 *
 *   in   x0     B*nx
 *        w      B*T*nx disturbances, or NULL: drawn on the device as set by tmpc_mc_set_device_rng (w_t of trajectory b is
 *               the w of tmpc_mc_run's stream for (seed, first_trajectory + b, t); montecarlo.draw_realisations_philox is the
 *               host twin); NULL without the device generator: no disturbance
 *        HX,hX  rX x nx, rX   check set for x_t (normally the un-tightened X); rX = 0: no check
 *        HU,hU  rU x nu, rU   check set for u_t (normally the un-tightened U); rU = 0: no check
 *        HZ,hZ  rZ x nx, rZ   tube cross-section for x_t - x_nom_0,t; rZ = 0: no check
 *        capture index of the trajectory whose x (T+1)*nx, x_nom0 T*nx, u T*nu are copied to cap_x / cap_xn / cap_u
 *               (-1 or any NULL pointer: none)
 *   out  (any may be NULL), per trajectory:
 *        cost        sum_t x_t'Q x_t + u_t'R u_t
 *        x_viol      steps with x_t outside {HX x <= hX} (by more than 1e-7, polytope's abs_tol)
 *        u_viol      steps with u_t outside {HU u <= hU}
 *        tube_viol   steps with x_t - x_nom0_t outside Z
 *        not_optimal solves with status != TMPC_STATUS_OPTIMAL
 *        fail_step   first step whose solve has status >= TMPC_STATUS_INFEASIBLE, -1 if none; from that step on the
 *                    trajectory is frozen (x stays, nothing accumulates)
 *        x_final     B*nx
 *        iters_sum   interior-point iterations of the trajectory's solves
 * All pointers are HOST pointers; the call returns when the results are in place.
 */
int tmpc_reg_run(tmpc_handle *h, int64_t B, int32_t T, const double *x0, const double *w,
                 const double *HX, const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU,
                 const double *HZ, const double *hZ, int32_t rZ,
                 double *cost, int32_t *x_viol, int32_t *u_viol, int32_t *tube_viol, int32_t *not_optimal, int32_t *fail_step,
                 double *x_final, int32_t *iters_sum, int64_t capture, double *cap_x, double *cap_xn, double *cap_u);

/*
 * Replaces solve_optimization_problem(x_init, ref[, gamma_t])
 * (TubeTrackingMPC.py:170-194, :307-349) for B independent instances.
 *
 *   in   x_k     B*nx     state estimate handed to the controller (x_init)
 *        ref     B*nx     reference state                          (ref)
 *        variant B or NULL  0 = base problem, 1 = packet-received problem (gamma_t)
 *   out  u_nom   B*N*nu   nominal inputs u_0..u_{N-1}   (reference returns its transpose, nu*N)
 *        x_nom0  B*nx     x_nom[:,0]                     (TubeTrackingMPC.py:364)
 *        xu_ss   B*(nx+nu) [x_bar | u_bar]               (TubeTrackingMPC.py:191-192)
 *        x_nom   B*(N+1)*nx or NULL  full nominal state trajectory
 *        status  B        TMPC_STATUS_*
 *        iters   B        interior-point iterations used
 *
 * All pointers are HOST pointers; the call copies in, launches, copies out and
 * returns when the results are in place.  Outputs of instances with
 * status >= TMPC_STATUS_INFEASIBLE are NaN (the reference returns None).
 */
int tmpc_solve_batch(tmpc_handle *h, int64_t B,
                     const double *x_k, const double *ref, const uint8_t *variant,
                     double *u_nom, double *x_nom0, double *xu_ss, double *x_nom,
                     int32_t *status, int32_t *iters);

/*
 * Same, with every pointer a DEVICE pointer on the handle's device (e.g. a torch
 * tensor's data_ptr()).  The kernels are enqueued on one of the handle's streams and the
 * call returns without synchronising; use tmpc_synchronize() or
 * tmpc_last_kernel_ms().
 *
 * Ordering contract: calls on a handle take effect as if executed in call order.  Independent calls may run concurrently: the
 * handle keeps up to TMPC_MAX_LANES launch lanes (a non-blocking stream each, with its own launch scratch; tmpc_set_call_lanes), and a
 * call goes to the next lane in rotation when none of its arrays overlaps -- read after write, write after write or write after
 * read, by byte range: x_k, ref, variant are read; u_nom, x_nom0, xu_ss, x_nom, status, iters written -- an array of the
 * unfinished calls of the handle.  A call that does overlap stays on a lane behind a call it depends on, and that lane waits for the
 * other lanes as well where it depends on several.  The tail of one launch (a launch ends with its slowest instances while most of
 * the card idles) then runs under the head of the next ones: a server that streams independent batches through one handle needs no
 * second handle.  A lane is taken into use by the first call that finds unfinished, independent work on every lane in use to run
 * beside (the lanes' streams are created by tmpc_create, together, so that they land on different hardware queues);
 * every other entry point (tmpc_solve_batch, tmpc_mc_run / _replay, tmpc_reg_run, the getters) joins the lanes before it runs.
 * tmpc_set_call_overlap turns all lanes but the first off.
 * The handle's streams are its own: they are NOT ordered against the stream that produced the inputs or will consume the
 * outputs (e.g. torch's current stream).  The caller synchronises on both sides: the producers of x_k / ref / variant must have
 * completed before this call (torch.cuda.synchronize() or an event wait), and the outputs may be read only after
 * tmpc_synchronize(), as before.  Instances whose variant id is >= the handle's number of problems get status TMPC_STATUS_NUMERICAL
 * and NaN outputs.
 */
int tmpc_solve_batch_device(tmpc_handle *h, int64_t B,
                            const double *x_k, const double *ref, const uint8_t *variant,
                            double *u_nom, double *x_nom0, double *xu_ss, double *x_nom,
                            int32_t *status, int32_t *iters);

/*
 * Which kernel solves a variant.  TMPC_PATH_AUTO (default): the one-wave-per-QP kernel
 * (csrc/tmpc_kernels.hip) when one of its compiled shapes covers the condensed problem, otherwise
 * the workgroup-per-QP kernel (csrc/tmpc_block.hip: nv <= 128, any number of rows, G'DG on the
 * FP64 matrix cores).  TMPC_PATH_WAVE / TMPC_PATH_BLOCK force one of them (TMPC_E_UNSUPPORTED if
 * it cannot take the problem).  Results agree to the refinement's accuracy either way
 * (tests/test_hip_parity.py).  tmpc_get_kernel_path reports the path a variant currently takes.
 * Environment (developer knob, read by tmpc_create): TMPC_BLOCK_PAIRS=0 makes the workgroup-per-QP
 * kernel keep one row of G per constraint row instead of one per pair of mirrored rows
 * (DESIGN.md section 4); the answers agree (tests/test_block_layout.py).
 */
#define TMPC_PATH_AUTO  0
#define TMPC_PATH_WAVE  1
#define TMPC_PATH_BLOCK 2
int tmpc_set_kernel_path(tmpc_handle *h, int path);
int tmpc_get_kernel_path(const tmpc_handle *h, int variant);

/*
 * Name of the kernel instantiation that solves a variant on the current path, as it appears (up to the
 * anonymous-namespace qualifier) in a rocprofv3 kernel trace: "tmpc::solve_kernel<NV,DP,DS,KC,CP,CS,WPB>" (one wavefront
 * per QP; shape = padded variables, dense paired / single slots, factored width and paired / single slots, waves per
 * workgroup) or "tmpc::solve_block_kernel<T>" (one workgroup per QP).  The string belongs to the library.
 */
const char *tmpc_kernel_name(const tmpc_handle *h, int variant);

/*
 * Diagnostics (tests/wavesim: the kernel sources compiled for the CPU under sanitizers): writes to `path` everything the
 * wave-per-QP kernel receives for `variant` -- two int32 words {tag "TMPC" = 0x43504d54, dump format = tmpc::DUMP_FORMAT of
 * csrc/tmpc_device.hpp, bumped with every change of the records below: a reader built against another format must reject the
 * file}, the compiled shape (NVP, DP, DS, KC, CP, CS; int32 x 6), the size of tmpc::DeviceQP (csrc/tmpc_device.hpp; uint64)
 * and the structure itself, then, for each of its arrays in field order (Gt, Hct, Psi, Hs, Hinv, F1s, F2s, g0p, Esp, vmask,
 * row_of, gp0, Ep, Dv, Tzs, Txf, Mth, A, B, cip), a uint64 byte count and the bytes.  Host-only handles (device < 0) only:
 * TMPC_E_UNSUPPORTED otherwise, or when no wave shape covers the variant.  Not part of the solve path.
 */
int tmpc_debug_dump_layout(const tmpc_handle *h, int variant, const char *path);
/* The same for the workgroup-per-QP kernel: the two format words, tiles and workspace rows (int32 x 2), the sizes of
 * tmpc::DeviceQP and tmpc::BlockQP (uint64 x 2), the two structures (BlockQP as of format 2: ncp, nz4, zx0, znx, mir, ng, ngp, the
 * array pointers, row_start[9]), then 20 records, each a uint64 byte count and the bytes: Hs, Hinv, F1s, F2s, gp0, Ep, Dv, Tzs,
 * Txf, Mth, A, B of the first structure; Grm ([ngp + NVP][NVP]: the rows of G, then the NVP rows of Hs), Gcm, GHrm, g0, Es,
 * ncols of the second; Gw ([ncp][NVP], G by constraint row) -- zero bytes when Gw is Grm (mir == 0); and ci ([ncp], format 3). */
int tmpc_debug_dump_block_layout(const tmpc_handle *h, int variant, const char *path);
/* The same for the batched LP kernel (tmpc_lp_batch): the polytope (H, h) in kernel units -- int32 d, nr, nrp, DP (padded
 * dimension), max_iter; double tol, relax_by, hm; then H transposed [DP][nrp], h [nrp] and the row scale [nrp].  No device
 * is touched.  TMPC_E_INVALID when the batch would be decided on the host (no normal at all, or a row 0 <= h_r < 0). */
int tmpc_debug_dump_lp_layout(int32_t d, int32_t nr, const double *H, const double *h, double relax_by, const char *path);

/*
 * Device-resident closed loop over a lossy network for B independent trajectories and T time steps: the body
 * of the reference's Monte-Carlo loop (Results/results_linear_system.py:209-259,291; with extended != 0
 * results_linear_system_with_extendedMPC.py:247-378) -- controller packet, packet losses in both directions,
 * consistent actuator with nominal model and ancillary feedback (SmartActuator.py:125-231), plant update,
 * estimator / robust estimator (Estimator.py:9-161) -- run as per-trajectory state machines, one wavefront per trajectory,
 * on the handle's stream: INSIDE the solve kernel, between two solves of the trajectory, where the controller has one
 * QP (one launch for the whole sweep; tmpc_mc_set_fused below), else in ONE launch per time step next to the solve's.
 * Only the statistics return to the host.
 *
 *   in   p_loss B        loss probability of the trajectory (both directions)
 *        ref    T        position reference; the solve gets ref_t = [ref[t], 0, ...]   (:240)
 *        th_u   B*T      uniforms: controller->plant packet of step t is lost iff t > 0 and th_u < p_loss
 *        ga_u   B*T      same for the plant->controller packet
 *        w      B*T*nx   disturbance realisations
 *        x0     B*nx or NULL (zeros)
 *        HZ,hZ  rZ x nx, rZ   the tube cross-section Z for the membership check (:258); rZ = 0 skips it
 *   out  (any may be NULL)
 *        err2        B   sum_t (x_t[0]-ref_t)^2 + |x_t[1:]|^2   (tracking error of :291 = sqrt(err2)/T)
 *        tube_viol   B   steps with x_t - x_nom_t outside Z
 *        not_optimal B   solves with status != 0 (a solve with status >= 2 sends no packet)
 *        x_final     B*nx
 *        consistent  B   max |x_hat - x_nom| over the steps with Theta_t = gamma_t = 1 (0 by Proposition 1; not for extended)
 *        iters_sum   B   interior-point iterations spent on the trajectory (the solve effort the reference's scripts report
 *                        as times, results_linear_system.py:305-315)
 * All pointers are HOST pointers; the call returns when the results are in place.
 *
 * With a reference table set (tmpc_mc_set_reference_table below, "full-reference mode") `ref` is not read and may be NULL: the
 * solve of step t of trajectory b gets the full state table[ref_id[b]][t][0..nx), and err2 is sum_t sum_i (x_t[i] - r_t[i])^2
 * (the physics-rate error of a nonlinear plant likewise, r_t held over the sampling period).  B must be the table's B and
 * T <= T_tab, else TMPC_E_INVALID.  Everything else is unchanged.
 */
int tmpc_mc_run(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref,
                const double *th_u, const double *ga_u, const double *w, const double *x0, const double *HZ, const double *hZ,
                int32_t rZ, double *err2, int32_t *tube_viol, int32_t *not_optimal, double *x_final, double *consistent,
                int32_t *iters_sum);

/*
 * The state machines of tmpc_mc_run driven by GIVEN controller packets instead of solved ones -- the test entry that pins the
 * device-side Estimator / RobustEstimator (Estimator.py:43-161) and SmartActuator / ConsistentActuator (SmartActuator.py:57-231)
 * directly against trajectories recorded from the reference's classes (tests/golden/glue_golden.npz, glue_smart_golden.npz).
 * Step t of trajectory b runs exactly the kernel tmpc_mc_run launches after its solve, with the packet
 * U_pkt[b][t] = [u_0 .. u_{N-1} | terminal column] ((N+1) x nu, row per column of the reference's U_t) and, for the extended
 * controller, x_nom_0 = xn0_pkt[b][t]; theta / gamma are the ARRIVAL flags of the two links (1 = arrives; step 0 always
 * arrives, results_linear_system.py:211-214), w the disturbances, x0 the initial state (NULL: zeros).  No QP is solved.
 *   out  trace_f  B*T*(3 nx + nu)   per step: x_{t+1}, x_hat_{t+1}, the nominal state in the plant's packet, u_t
 *        trace_i  B*T*3             per step: s_t, Theta_t, and q_t as the controller's packet of step t carried it
 * Actuator kind, plant and gains are the handle's (tmpc_mc_set_actuator, tmpc_mc_set_plant, K / K_anc of tmpc_problem).
 * All pointers are HOST pointers.  Added without an ABI bump: a new export, nothing else changed.
 */
int tmpc_mc_replay(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *U_pkt, const double *xn0_pkt,
                   const uint8_t *theta, const uint8_t *gamma, const double *w, const double *x0, double *trace_f, int32_t *trace_i);

/*
 * Warm start inside tmpc_mc_run (off by default).  Consecutive QPs of a trajectory share most of their active set: with
 * on != 0 every solve first hands the working set certified by the trajectory's previous solve (of the same problem
 * variant) to the active-set refinement.  The refinement accepts a point only if it is primal feasible on ALL rows with
 * non-negative multipliers, i.e. only the exact minimiser; otherwise the solve falls back to the cold interior-point
 * start.  Results are therefore the same with and without (tests/test_closed_loop.py); only the iteration counts drop.
 * One-wave-per-QP kernel only; the workgroup-per-QP kernel ignores the setting.
 */
int tmpc_mc_set_warm_start(tmpc_handle *h, int on);

/*
 * How tmpc_mc_run steps its trajectories.  TMPC_MC_FUSED_ON: ONE launch for the whole sweep -- a wavefront keeps its
 * trajectory for all T time steps and alternates between the QP solve and the trajectory's state machines inside the
 * kernel (the reference's loop body, Results/results_linear_system.py:209-259, with nothing between two of its
 * iterations).  TMPC_MC_FUSED_OFF: per time step one solve launch (per problem variant) and one
 * launch of the state machines.  The two give the same numbers bit for bit: a trajectory's arithmetic does not depend on
 * which wavefront runs it or when.  TMPC_MC_FUSED_AUTO (default): fused when the trajectories fill their rounds on the
 * card's resident wavefronts to at least 85 % (or fit in one round), else per step -- a fused work item is T solves
 * long, a per-step one a single solve.  Fusing needs ONE problem on the one-wave-per-QP kernel: the extended controller
 * (two problems, chosen per step by the arrival flag) takes ONE launch per problem and time step with the state machines
 * of the problem's trajectories inside (two launches per step instead of three: _ON, and _AUTO from one round of resident
 * wavefronts on -- a smaller batch is bound by the latency of its launches, which the state machines inside lengthen);
 * the workgroup-per-QP kernel and tmpc_mc_replay always take a solve launch per problem and a state-machine launch per
 * step.  tmpc_mc_last_fused: what the last tmpc_mc_run of the handle did -- 1: one launch for the sweep; 2: one launch
 * per problem and step, state machines inside; 0: solve launches + a state-machine launch per step.
 */
#define TMPC_MC_FUSED_OFF 0
#define TMPC_MC_FUSED_ON 1
#define TMPC_MC_FUSED_AUTO 2
int tmpc_mc_set_fused(tmpc_handle *h, int mode);
int tmpc_mc_last_fused(const tmpc_handle *h);

/*
 * Per-solve computation times -- what the reference's controllers keep in _computational_times and the scripts print as
 * max / quantiles / median (TubeTrackingMPC.py:205, 242-243; results_linear_system.py:305-315).  On the device an MPC solve
 * is one instance of a batched launch; with tmpc_set_solve_timing(on) every instance records the time from the moment its
 * wavefront / workgroup picks it up to the moment its outputs are written, in ticks of the GPU's constant 100 MHz counter
 * (s_memrealtime: 1 tick = 10 ns).  tmpc_get_solve_ticks copies out the B tick counts of the last tmpc_solve_batch /
 * tmpc_solve_batch_device call (instances a variant selector skipped: 0); after a tmpc_mc_run, tmpc_mc_get_solve_ticks
 * gives per trajectory the sum and the maximum over its T solves (either pointer may be NULL).  Off by default.
 */
int tmpc_set_solve_timing(tmpc_handle *h, int on);
int tmpc_get_solve_ticks(tmpc_handle *h, int64_t B, int64_t *ticks);
int tmpc_mc_get_solve_ticks(tmpc_handle *h, int64_t B, int64_t *ticks_sum, int64_t *ticks_max);

/*
 * Sample trajectory of tmpc_mc_run -- what the scripts keep for their plots (x_traj, x_nom_traj of one run per loss rate,
 * results_linear_system.py:298-301).  tmpc_mc_set_capture(index >= 0) makes the following runs record trajectory `index`
 * (-1: off); after a run tmpc_mc_get_capture copies out, for t = 0 .. T-1, the plant state x_t, the nominal state the tube
 * check of step t uses, and the applied input u_t (row-major T x nx, T x nx, T x nu; any pointer may be NULL).  Dead
 * trajectories of the R-MPC loop leave zeros from their last step on.
 */
int tmpc_mc_set_capture(tmpc_handle *h, int64_t index);
int tmpc_mc_get_capture(tmpc_handle *h, int32_t T, double *x_traj, double *x_nom_traj, double *u_traj);

/*
 * Realisations drawn on the device (throughput runs: the host arrays of a 10 x 1000 x 250 sweep are 120 MB and their
 * generation takes longer than the closed loop).  With tmpc_mc_set_device_rng(on = 1, seed, first_trajectory, w_bound)
 * the following tmpc_mc_run calls ignore th_u, ga_u and w (NULL allowed) and draw, for trajectory b of the call and step t,
 * from Philox4x64-10 with key (seed, first_trajectory + b) and counter (t, j, 0, 0): block j = 0 gives the theta and gamma
 * uniforms and w_0, w_1, block j >= 1 gives w_{4j-2} .. w_{4j+1}; a uniform is (x >> 11) * 2^-53, a disturbance component
 * w_bound[i] * (2 u - 1) (the reference draws rng_w.uniform(-w_bound, w_bound), results_linear_system.py:229-233).
 * A trajectory's stream depends on (seed, its global index, t) only -- not on the batch it is solved in nor on the rank.
 * LinearMPCOverNetworks.montecarlo.draw_realisations_philox is the numpy twin (tests: identical closed loops).
 * w_bound: nx half-widths, NULL = no disturbance.  on = 0 returns to host arrays.
 */
int tmpc_mc_set_device_rng(tmpc_handle *h, int on, uint64_t seed, int64_t first_trajectory, const double *w_bound);

/*
 * Plant simulated by tmpc_mc_run.  TMPC_PLANT_LINEAR (default): x+ = A x + B u + w (results_linear_system.py:248).
 * TMPC_PLANT_CARTPOLE: the nonlinear cart-pole the linear model was derived from (results_linear_system.py:26-47;
 * the reference integrates it with PyBullet at 500 Hz, results_nonlinear_system.py:30-37), zero-order hold of the
 * input over the sampling period, classical RK4 with `substeps` steps; w is added to the result (pass zeros).
 * par = {M, m, b, I, g, l, Th}.  Needs nx = 4, nu = 1.
 */
#define TMPC_PLANT_LINEAR   0
#define TMPC_PLANT_CARTPOLE 1
#define TMPC_PLANT_EXTERNAL 2   /* the caller's plant: set by a stepped session (tmpc_mc_open) only, refused by tmpc_mc_set_plant */
int tmpc_mc_set_plant(tmpc_handle *h, int kind, const double *par7, int substeps);
/*
 * A plant model per trajectory for the regulator loop (tmpc_reg_run): the plant of trajectory b differs from the controller's model,
 * which is the point -- the gain and the QP stay the handle's (A, B).
 *   kind    TMPC_PLANT_LINEAR.  models is B x nx x (nx + nu), row-major: row i of trajectory b is [A_b[i, :] | B_b[i, :]], its plant
 *           x+ = A_b x + B_b u + w.  substeps is ignored.
 * B == 0 clears the models.  models is HOST memory, copied; the copy lives on the host (the setter works on a host-only handle) and
 * is uploaded with each loop.  While models are set, tmpc_reg_run needs its B equal to the models' B (TMPC_E_INVALID otherwise, before
 * anything is launched).  TMPC_E_INVALID, the message naming trajectory and entry: B < 0, models == NULL with B > 0, another kind, a
 * non-finite entry.  A refused call changes nothing.  Tracking handles: TMPC_E_UNSUPPORTED -- tmpc_mc_run, tmpc_mc_replay and the
 * stepped sessions simulate the handle's one plant (tmpc_mc_set_plant).  Added without an ABI bump: a new export.
 */
int tmpc_mc_set_plant_models(tmpc_handle *h, int kind, int64_t B, const double *models, int substeps);
/*
 * A plant per trajectory in the TRACKING loop: the stepped session (tmpc_mc_open / tmpc_mc_step_device, below) driven for T steps around a
 * family of plants that one more kernel advances (tmpc_plant.hip), with nothing returning to the host in between.  The resident kernels
 * of tmpc_mc_run are not involved: they keep their one plant.
 *
 * tmpc_plant_step_device(device, kind, nx, nu, B, models, substeps, x, u, w, x_plus, stream): ONE launch, x_plus[b] = f_b(x[b], u[b]) + w[b].
 *   kind    TMPC_PLANT_CARTPOLE (nx = 4, nu = 1): models is B x 7 rows {M, m, b, I, g, l, Th}; u held over the period, classical RK4 with
 *           `substeps` >= 1 steps of Th_b / substeps -- the plant of tmpc_mc_set_plant with the row's numbers.
 *           TMPC_PLANT_LINEAR (1 <= nx <= 16, 1 <= nu <= 16): models is B x nx x (nx + nu), the layout of tmpc_mc_set_plant_models;
 *           x_plus_i = w_i + sum_k A_b[i, k] x_k + sum_j B_b[i, j] u_j, summed in this order.  substeps is ignored.
 *   Every array is a DEVICE pointer: models, x (B*nx), u (B*nu), x_plus (B*nx), w (B*nx, or NULL: no disturbance).  stream: a hipStream_t
 *   or NULL.  Enqueues the kernel and returns without synchronising.  x_plus must not overlap x (the lanes of one trajectory would
 *   race): TMPC_E_INVALID, as for B < 1, another kind, a shape the kind does not take and a NULL pointer -- all found before anything
 *   touches the device, the message through tmpc_last_error(NULL).  With tmpc_mc_step_device it makes a caller's own loop around the
 *   library's plants.
 *
 * tmpc_mc_run_plants(h, B, T, extended, kind, models, substeps, p_loss, ref, th_u, ga_u, w, x0, HZ, hZ, rZ, HX, hX, rX, HU, hU, rU, err2,
 *                    tube_viol, x_viol, u_viol, not_optimal, x_final, consistent, iters_sum, err2_phys): HOST pointers, the semantics of
 *   tmpc_mc_run plus the session's check sets X and U (x_viol, u_viol) and the family: trajectory b runs on plant b of `models` (copied;
 *   kind, layout and substeps as above, with the handle's nx and nu).  err2_phys (B, or NULL; cart-pole only, not written for a linear
 *   family): the physics-rate error of tmpc_mc_get_physics_error, which works afterwards too.  Any output may be NULL.
 *   Per step (number of problems + 2) launches on the handle's stream -- the solve(s), the state machines, the plants -- and between the
 *   uploads and the copy-back no synchronisation and no copy.  Honoured as set on the handle: tmpc_mc_set_actuator, _set_warm_start,
 *   _set_capture, tmpc_set_solve_timing, tmpc_set_kernel_path, the reference table, the loss channel and the device generator -- with it
 *   th_u, ga_u and w may be NULL: the session draws the loss uniforms, the plant kernel the disturbance, exactly tmpc_mc_run's numbers.
 *   Ignored: tmpc_mc_set_plant and tmpc_mc_set_fused (tmpc_mc_last_fused: 0).  An R-MPC trajectory that has stopped keeps its state.
 *   Afterwards tmpc_mc_get_link_stats, _get_capture and _get_solve_ticks work as after tmpc_mc_close.
 *   Refused before anything is launched, the handle left as it was: TMPC_E_INVALID for a regulator handle, an open session, B or T < 1,
 *   a B that does not match a reference table or channel that is set, a cart-pole family on a handle with nx != 4 or nu != 1, a row that
 *   is no plant (the rule of tmpc_estimate_w_models; a linear entry that is not finite) with the message naming trajectory and field or
 *   entry, a NULL input; TMPC_E_DEVICE for a host-only handle, after these.  A device error in a step ends the loop: TMPC_E_DEVICE.
 * Added without an ABI bump: new exports, nothing else changed.
 */
int tmpc_plant_step_device(int device, int kind, int32_t nx, int32_t nu, int64_t B, const double *models, int substeps, const double *x,
                           const double *u, const double *w, double *x_plus, void *stream);
int tmpc_mc_run_plants(tmpc_handle *h, int64_t B, int32_t T, int extended, int kind, const double *models, int substeps, const double *p_loss,
                       const double *ref, const double *th_u, const double *ga_u, const double *w, const double *x0, const double *HZ,
                       const double *hZ, int32_t rZ, const double *HX, const double *hX, int32_t rX, const double *HU, const double *hU,
                       int32_t rU, double *err2, int32_t *tube_viol, int32_t *x_viol, int32_t *u_viol, int32_t *not_optimal, double *x_final,
                       double *consistent, int32_t *iters_sum, double *err2_phys);

/*
 * Stepped closed loop around a plant the CALLER owns: the per-trajectory state machines and the solve kernels of tmpc_mc_run,
 * opened once, advanced ONE time step per call with the plant state given by the caller, and closed for the statistics.  For a
 * plant that is neither the handle's linear model nor the closed-form cart-pole -- another mechanism, saturation or friction, a
 * batched simulator on the device, a physics engine or hardware on the host.
 *
 * The cut: in the loop body the plant appears once, x_{t+1} = f(x_t, u_t) + w_t.  The estimator predicts from x_t / x_nom_t and
 * u_t, the solve of step t reads x_hat_t, which step t-1 produced; so a step needs the caller's x_t only AFTER its solve (actuator,
 * statistics, checks, estimator) and gives back u_t only.
 *
 * tmpc_mc_open(h, B, T, extended, p_loss, ref, th_u, ga_u, x0, HZ, hZ, rZ, HX, hX, rX, HU, hU, rU): HOST pointers, copied.
 *        B, T          trajectories; the number of steps the session MAY take (ref, th_u, ga_u are sized by it)
 *        p_loss, ref, th_u, ga_u, x0, HZ / hZ / rZ     as tmpc_mc_run; x, x_hat and x_nom start at x0 (NULL: zeros), the first
 *                      packet always arrives.  With tmpc_mc_set_device_rng on, th_u / ga_u may be NULL: the loss uniforms are
 *                      those of Philox block 0, exactly tmpc_mc_run's.
 *        HX,hX  rX x nx, rX     optional check set for the caller's x_t   (rX = 0: none)
 *        HU,hU  rU x nu, rU     optional check set for the applied u_t    (rU = 0: none); a step counts when a row is exceeded
 *                      by more than 1e-7 (tmpc_reg_run's convention).
 *   NO disturbance is ever drawn or added: w belongs to the caller's plant (draw_realisations_philox of the Python package
 *   reproduces the library's w for a caller who wants it).  The session honours tmpc_mc_set_actuator, _set_warm_start,
 *   _set_capture, tmpc_set_solve_timing and tmpc_set_kernel_path as set at open (no setter succeeds before close); it
 *   ignores tmpc_mc_set_plant (and leaves that setting alone) and tmpc_mc_set_fused: every step is the solve launch(es) of tmpc_solve_batch -- one per problem -- and ONE launch of the state
 *   machines, on the wave and on the block kernel path alike (the results do not depend on the launch form, see above).
 *
 * tmpc_mc_step_device(h, x_t, u_t, caller_stream): step t = the number of steps taken so far.  x_t (B*nx, read) and u_t (B*nu,
 *   written: the applied input, 0 for an R-MPC trajectory that has stopped) are DEVICE pointers and may differ from call to call.
 *   Returns without synchronising: no host synchronisation, no host<->device transfer, (number of problems + 1) kernel launches,
 *   no copy.  caller_stream != NULL (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream): the step's state machines are
 *   ordered behind the work already enqueued on that stream and the work enqueued on it afterwards is ordered behind the step,
 *   by an event each way (hipEventRecord / hipStreamWaitEvent); the launches stay on the handle's stream.  The step's SOLVE does
 *   not read x_t and is not ordered behind the caller's stream.  caller_stream == NULL: the caller synchronises on both sides
 *   (x_t complete before the call, tmpc_synchronize before u_t is read) -- the contract of tmpc_solve_batch_device.
 * tmpc_mc_step(h, x_t, u_t): the same with HOST pointers, one DMA each way through a pinned block; returns when u_t is in place
 *   (a plant that lives on the host).
 * tmpc_mc_close(h, err2, tube_viol, x_viol, u_viol, not_optimal, consistent, iters_sum, steps_done): synchronises and copies
 *   out the per-trajectory statistics over the steps taken (semantics of tmpc_mc_run; x_viol / u_viol: steps with x_t outside X /
 *   u_t outside U; steps_done: one int32); any pointer may be NULL.  There is no x_final: the caller has it.  After close
 *   tmpc_mc_get_capture (with the T of open; rows of steps not taken are zero) and tmpc_mc_get_solve_ticks work as after a run.
 *
 * One session per handle.  tmpc_mc_open: TMPC_E_INVALID on a regulator handle or while a session is open, TMPC_E_DEVICE on a
 * host-only handle.  While a session is open tmpc_solve_batch, tmpc_solve_batch_device, tmpc_mc_run, tmpc_mc_replay and
 * tmpc_reg_run return TMPC_E_INVALID and leave the session intact (they would re-carve the memory it lives in); so does EVERY
 * setter of the handle (tmpc_set_solve_timing, tmpc_set_kernel_path, tmpc_set_call_overlap, tmpc_mc_set_actuator, _set_plant,
 * _set_capture, _set_device_rng, _set_warm_start, _set_fused): the session's arrays are carved for the settings of its open, and
 * none changes under it -- choose them before tmpc_mc_open.  A step beyond T,
 * and a step or a close without a session, return TMPC_E_INVALID.  A step that fails on the device ends the session: further
 * steps return TMPC_E_INVALID, close is still allowed.  tmpc_destroy closes an open session; after close the handle behaves as
 * before open.  R-MPC (TMPC_ACTUATOR_SMART): a trajectory whose solve is infeasible stops as in tmpc_mc_run (err2 NaN, counted
 * once in not_optimal) and its u_t is 0 from that step on.  Added without an ABI bump: new exports, nothing else changed.
 */
int tmpc_mc_open(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref, const double *th_u,
                 const double *ga_u, const double *x0, const double *HZ, const double *hZ, int32_t rZ, const double *HX,
                 const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU);
int tmpc_mc_step_device(tmpc_handle *h, const double *x_t, double *u_t, void *caller_stream);
int tmpc_mc_step(tmpc_handle *h, const double *x_t, double *u_t);
int tmpc_mc_close(tmpc_handle *h, double *err2, int32_t *tube_viol, int32_t *x_viol, int32_t *u_viol, int32_t *not_optimal,
                  double *consistent, int32_t *iters_sum, int32_t *steps_done);
/*
 * Full-state reference schedules of the closed loops, per trajectory ("full-reference mode" of tmpc_mc_run and tmpc_mc_open).
 *   table   K x T_tab x nx, row-major, HOST memory, copied: K >= 1 schedules of full-state references
 *   ref_id  B, in [0, K): the schedule of trajectory b of the next loops.  NULL: schedule 0 for everybody when K == 1,
 *           schedule b when K == B, TMPC_E_INVALID otherwise.
 *   K == 0  clears the setting (table, T_tab, B and ref_id are then ignored).
 * The copy lives on the host (the setter works on a host-only handle) and is uploaded with each loop.  While a table is set,
 * tmpc_mc_run and tmpc_mc_open need their B equal to the table's B and their T <= T_tab (TMPC_E_INVALID otherwise) and do not
 * read their `ref` (NULL allowed): the solve of step t of trajectory b gets table[ref_id[b]][t], and the tracking error of step t
 * is sum_i (x_t[i] - r_t[i])^2 against the reference the solve of step t used.  tmpc_mc_replay and tmpc_reg_run ignore the
 * setting.  TMPC_E_INVALID: K < 0, T_tab < 1, B < 1, table == NULL with K > 0, an id out of range, a regulator handle, an open
 * session.  Without a table every loop runs as before.
 *
 * tmpc_mc_step_device_ref / tmpc_mc_step_ref: tmpc_mc_step_device / tmpc_mc_step with ref_next (B*nx; a DEVICE pointer for the
 * former, read by the state-machine launch behind caller_stream like x_t; a HOST pointer for the latter), the reference of the
 * solve of step t + 1.  NULL: row t + 1 of the schedule, i.e. the plain call.  Only in a session opened in full-reference mode
 * (TMPC_E_INVALID otherwise; the session stays usable): the table gives the reference of step 0 and the default of every later
 * step -- a caller with online references only passes a constant table.  Added without an ABI bump.
 */
int tmpc_mc_set_reference_table(tmpc_handle *h, int32_t K, int32_t T_tab, const double *table, int64_t B, const int32_t *ref_id);
int tmpc_mc_step_device_ref(tmpc_handle *h, const double *x_t, double *u_t, const double *ref_next, void *caller_stream);
int tmpc_mc_step_ref(tmpc_handle *h, const double *x_t, double *u_t, const double *ref_next);
/*
 * Bursty packet loss: a two-state Markov (Gilbert-Elliott) channel per link, and per-trajectory link statistics.
 *
 * The model.  Each of the two links of a trajectory (controller -> plant, plant -> controller) has a state in {G, B}.  Trajectory b
 * has four parameters, shared by its two links as p_loss is:
 *   p_gb = P(B at t | G at t-1),  p_bg = P(G at t | B at t-1),  e_g / e_b = loss probability in state G / B.
 * One uniform u per link and step decides the transition and the loss -- the step's th_u / ga_u entry, or its Philox block-0 words
 * (tmpc_mc_set_device_rng): the draw layout and every stream are those of the Bernoulli model.  With a = P(B | previous state),
 * i.e. p_gb after G and 1 - p_bg after B:
 *   u < a e_b                 (B, lost)
 *   else u < a                (B, arrives)
 *   else u < a + (1 - a) e_g  (G, lost)
 *   else                      (G, arrives)
 * The comparisons are strict, like the Bernoulli model's u < p_loss.  Both links start in G.  At t = 0 the packet arrives and the
 * state does not move (the draw of t = 0 is ignored, as ever).  A failed solve (status >= 2) still sends nothing (theta = 0), but
 * the channel's state follows the draw alone.  The three thresholds per previous state -- thr[b][prev][0..3) = a e_b, a,
 * a + (1 - a) e_g with prev = 0 (G), 1 (B) -- are computed once per trajectory on the host, every product and sum rounded on its
 * own (no fused multiply-add); the device only compares.  Hence p_gb = 0, e_g = p gives (0, 0, p) after G: the Bernoulli flags of
 * p_loss = p, bit for bit; and p_gb = 1, p_bg = 0, e_b = 1 loses every packet after step 0.
 *
 * tmpc_mc_set_channel: p_gb, p_bg, e_g, e_b are HOST arrays of B entries, copied.  B == 0 clears the setting (the arrays are then
 * ignored).  Works on a host-only handle.  While a channel is set, tmpc_mc_run and tmpc_mc_open need their B equal to the channel's
 * (TMPC_E_INVALID otherwise) and do not read p_loss, which may be NULL; a session honours the channel as set when it was opened.
 * tmpc_mc_replay takes its arrival flags as given and ignores the channel; regulator handles have no network.
 * TMPC_E_INVALID: a regulator handle, an open session, B < 0, a NULL array with B > 0, a probability outside [0, 1] or NaN.
 *
 * tmpc_mc_get_channel: the thresholds as they are uploaded, thr[B][2][3] (B * 6 doubles); TMPC_E_INVALID unless B is the channel's.
 *
 * tmpc_mc_get_link_stats: per trajectory of the last tmpc_mc_run, or of the session tmpc_mc_close just ended -- kept with either
 * loss model, any pointer may be NULL:
 *   lost_up    steps t > 0 whose controller -> plant packet the CHANNEL dropped (a packet withheld after a failed solve is not counted)
 *   lost_down  the same for the plant -> controller packet
 *   max_gap    max_t (t - s_t): the largest age of the sequence the actuator played
 *   overrun    steps with t - s_t >= N: the buffered sequence was exhausted and the terminal law Ub[N] - K x_nom applied
 * A trajectory of the smart actuator that has stopped counts nothing from the step of its infeasible solve on.
 * TMPC_E_INVALID: no such run, or another B.  Added without an ABI bump.
 */
int tmpc_mc_set_channel(tmpc_handle *h, int64_t B, const double *p_gb, const double *p_bg, const double *e_g, const double *e_b);
int tmpc_mc_get_channel(tmpc_handle *h, int64_t B, double *thr);
int tmpc_mc_get_link_stats(tmpc_handle *h, int64_t B, int32_t *lost_up, int32_t *lost_down, int32_t *max_gap, int32_t *overrun);
/*
 * Time-resolved records of the tracking loops, and their statistics over the ensemble per time step.
 *
 * The record.  With tmpc_mc_set_series(h, 1) a loop keeps two values per step t and trajectory b, TIME-major ([T][B]: row t holds the
 * B trajectories of step t):
 *   e[t][b]     the step's tracking-error term -- exactly the value the step adds to err2[b], |x_t - [ref_t, 0, ..]|^2 or, under a reference
 *               table, |x_t - r_t|^2 -- so that the sum of e[0..T)[b] in this order is err2[b], bit for bit
 *   word[t][b]  bit 0  TMPC_SER_ALIVE        the trajectory took step t
 *               bit 1  TMPC_SER_LOST_UP      the channel dropped the controller -> plant packet (as lost_up of tmpc_mc_get_link_stats: a
 *                                            packet withheld after a failed solve is not counted)
 *               bit 2  TMPC_SER_LOST_DOWN    the same for the plant -> controller packet
 *               bit 3  TMPC_SER_ADOPTED      Theta_t = 1: the actuator adopted the packet of this step
 *               bit 4  TMPC_SER_TUBE         x_t - x_nom_t is outside Z (what tube_viol counts; 0 when rZ = 0)
 *               bit 5  TMPC_SER_NOT_OPTIMAL  status != 0 (what not_optimal counts)
 *               bit 6  TMPC_SER_OVERRUN      t - s_t >= N: the terminal law (what overrun counts)
 *               bit 7  zero
 *               bits 8-19   iterations of the step's solve, saturating at TMPC_SER_SATURATE = 4095
 *               bits 20-31  age t - s_t of the sequence played, saturating at 4095
 * A trajectory that does not take the step writes nothing, and the buffers start as zeros: a stopped R-MPC trajectory has word 0 ("not
 * alive") and e = 0 from the step of its infeasible solve on, and so has every trajectory in the steps a session did not take.
 *
 * tmpc_mc_set_series: on != 0 switches the record on for the following tmpc_mc_run, tmpc_mc_run_plants and tmpc_mc_open (a session honours
 * it as set at open); works on a host-only handle; TMPC_E_INVALID on a regulator handle and while a session is open.  tmpc_mc_replay and
 * tmpc_reg_run ignore it.  A recording tmpc_mc_run runs its state machines in the per-step kernels (tmpc_mc_last_fused: 0, whatever
 * tmpc_mc_set_fused says): the fused kernels carry no recording code.  With the record off every loop is what it was.
 *
 * tmpc_mc_get_series: the record of the last such loop, or of the session tmpc_mc_close just ended, as e[T][B] and word[T][B] (either may
 * be NULL).  TMPC_E_INVALID: no such loop, the record was off, or another B or T.
 *
 * tmpc_mc_series_stats: the statistics below of the record where it lies on the device; tmpc_series_stats: the same reduction of HOST
 * arrays e[T][B], word[T][B] on `device`, without a handle (its errors through tmpc_last_error(NULL)).
 *   group     [B] group of every trajectory in [0, G), or -1: in no group; NULL: everybody is in group 0.  Groups need not be contiguous.
 *   q         [n_q] quantiles in [0, 1], 0 <= n_q <= 16
 * Column (t, g) is the entries [t][b] of the members b of group g.  An entry takes part iff its ALIVE bit is set; an alive entry whose e
 * is NaN (the loops produce none) is left out of the e statistics and counted in n_nan.  Outputs, [T][G] each, any may be NULL:
 *   n_alive, n_nan                                          int32  entries that take part; those of them with e = NaN
 *   lost_up, lost_down, adopted, tube, not_optimal, overrun int32  entries with the bit set
 *   age_max, iters_max   int32    age_sum, iters_sum   int64      of the saturated fields of the word
 *   e_sum     double  sum of the n = n_alive - n_nan values, in a fixed order that is not the host's: equal bytes from call to call, the
 *                     last bits differ from a sequential sum (0 for n = 0)
 *   e_max     double  their maximum (NaN for n = 0)
 *   e_q       [T][G][n_q] double: quantile q is the element of rank floor(q (n - 1)) -- one multiplication and one floor in double -- of
 *                     the sorted values: exact order statistics, no interpolation (NaN for n = 0).  Of -0.0 and 0.0 either may come back.
 *   kernel_ms the reduction's device time (HIP events), or NULL
 * TMPC_E_INVALID, before anything touches the device: B, T or G < 1, a NULL input, group[b] >= G or < -1, n_q outside [0, 16], q NULL with
 * n_q > 0, a q[i] outside [0, 1] or NaN; tmpc_mc_series_stats also where tmpc_mc_get_series would refuse.  Added without an ABI bump.
 */
#define TMPC_SER_ALIVE       0x01u
#define TMPC_SER_LOST_UP     0x02u
#define TMPC_SER_LOST_DOWN   0x04u
#define TMPC_SER_ADOPTED     0x08u
#define TMPC_SER_TUBE        0x10u
#define TMPC_SER_NOT_OPTIMAL 0x20u
#define TMPC_SER_OVERRUN     0x40u
#define TMPC_SER_ITERS_SHIFT 8
#define TMPC_SER_AGE_SHIFT   20
#define TMPC_SER_SATURATE    4095
#define TMPC_SER_MAX_Q       16
int tmpc_mc_set_series(tmpc_handle *h, int on);
int tmpc_mc_get_series(tmpc_handle *h, int64_t B, int32_t T, double *e, uint32_t *word);
int tmpc_mc_series_stats(tmpc_handle *h, int64_t B, int32_t T, int32_t G, const int32_t *group, int32_t n_q, const double *q,
                         int32_t *n_alive, int32_t *n_nan, int32_t *lost_up, int32_t *lost_down, int32_t *adopted, int32_t *tube,
                         int32_t *not_optimal, int32_t *overrun, int32_t *age_max, int64_t *age_sum, int32_t *iters_max, int64_t *iters_sum,
                         double *e_sum, double *e_max, double *e_q, float *kernel_ms);
int tmpc_series_stats(int device, int64_t B, int32_t T, const double *e, const uint32_t *word, int32_t G, const int32_t *group, int32_t n_q,
                      const double *q, int32_t *n_alive, int32_t *n_nan, int32_t *lost_up, int32_t *lost_down, int32_t *adopted, int32_t *tube,
                      int32_t *not_optimal, int32_t *overrun, int32_t *age_max, int64_t *age_sum, int32_t *iters_max, int64_t *iters_sum,
                      double *e_sum, double *e_max, double *e_q, float *kernel_ms);
/*
 * With a nonlinear plant tmpc_mc_run also sums |x - ref|^2 over the T * substeps physics steps (the state at the start of
 * every physics step, i.e. x_traj[:, 0:-1] of results_nonlinear_system.py:361, whose tracking error is taken at 500 Hz);
 * copied out per trajectory by tmpc_mc_get_physics_error (NaN for an R-MPC trajectory that stopped).
 */
int tmpc_mc_get_physics_error(tmpc_handle *h, int64_t B, double *err2_phys);

/*
 * Plant-side actuator simulated by tmpc_mc_run.  TMPC_ACTUATOR_CONSISTENT (default): ConsistentActuator with nominal
 * model and ancillary feedback (SmartActuator.py:125-231), the remote tube MPC's actuator.  TMPC_ACTUATOR_SMART: the plain
 * SmartActuator (SmartActuator.py:11-123) the reference pairs with the non-robust TrackingMPC (results_linear_system.py:
 * 198-205, 262-287): no nominal model, terminal law on the measured state, the plant packet carries the measured state.
 * With it a trajectory whose solve is infeasible stops (the reference sets track_feasible = False, :268-270): its err2
 * becomes NaN, its x_final the last state reached, and not_optimal counts the one failed solve.
 */
#define TMPC_ACTUATOR_CONSISTENT 0
#define TMPC_ACTUATOR_SMART      1
int tmpc_mc_set_actuator(tmpc_handle *h, int kind);

/* Block until everything enqueued on the handle, on every launch lane, has finished. */
int tmpc_synchronize(tmpc_handle *h);

/*
 * Successive independent tmpc_solve_batch_device calls of the handle on several launch lanes (on != 0, the default; see the
 * ordering contract there) or every call on the handle's first stream (on = 0: calls run one after the other, and the
 * other streams stay idle).  Results do not depend on the setting.  Turning it off orders the first
 * lane behind what the others still hold; turning it on waits for the calls enqueued while it was off.
 */
int tmpc_set_call_overlap(tmpc_handle *h, int on);
/*
 * The number of launch lanes the independent calls of the handle rotate over while the overlap is on: n = 1 ... TMPC_MAX_LANES
 * (1: as with the overlap off).  A new handle takes the environment's TMPC_CALL_LANES, else the library's default (DESIGN.md 5.1
 * "Between launches" has the measurements behind it); two lanes schedule exactly as the two-lane handle did.  A handle with a
 * variant on the workgroup-per-QP kernel uses at most two, whatever is set here (that kernel's workspace is per lane).  The
 * ordering contract of tmpc_solve_batch_device holds for every n, and results do not depend on it.  Changing the number waits
 * for the handle's calls.  tmpc_get_call_lanes: the lanes in use now.
 */
#define TMPC_MAX_LANES 4
int tmpc_set_call_lanes(tmpc_handle *h, int n);
int tmpc_get_call_lanes(const tmpc_handle *h);
/*
 * Diagnostics: calls_per_lane[2] = the tmpc_solve_batch_device calls by the parity of the lane changes since the lanes were last
 * joined (a call that goes to another lane than the call before it changes the parity) -- with two lanes, the calls enqueued on the
 * first / second lane, as before; for every lane count, independent calls in rotation alternate between the two entries.
 * *cross_lane_waits = the calls among them that depended on unfinished calls of several lanes and made their lane wait for the
 * others -- since the handle was created or the counters were last reset (reset != 0 clears them after reading).  Either
 * pointer may be NULL.  tmpc_debug_lane_counters_n: the same with calls_per_lane[TMPC_MAX_LANES], one count per lane.
 */
int tmpc_debug_lane_counters(tmpc_handle *h, int64_t *calls_per_lane, int64_t *cross_lane_waits, int reset);
int tmpc_debug_lane_counters_n(tmpc_handle *h, int64_t *calls_per_lane, int64_t *cross_lane_waits, int reset);
/*
 * Diagnostics (tests/test_elastic_policy.py): the lane policy, and the policy of an elastic launch grid that is not in use yet (DESIGN.md
 * 5.1 "Between launches"), themselves (csrc/tmpc_hazard.hpp); none of them touches a device, and all work on a host-only handle or without one.
 * tmpc_debug_elastic_grid: *core = the core workgroups of an elastic launch on n_cu CUs with `lanes` lanes set (a handle with a
 *   block-kernel variant: at most two), *eligible = whether a launch over B instances with wpb waves per workgroup would be elastic.
 * tmpc_debug_surplus_yields: the decision of a surplus workgroup that reads `followers`, 0 | 1.
 * tmpc_debug_plan_lanes: the lanes of a script of n_calls tmpc_solve_batch_device calls none of which finishes, on a fresh handle
 *   with `lanes` lanes; ptrs = [n_calls][9] pointer arguments as in tmpc_debug_calls_conflict, B = [n_calls].  lane_out[i] = the
 *   call's lane, waited_out[i] = bit l set: its lane waited for lane l, followers_out[i] = what call i's followers word ends at.
 * tmpc_debug_busy_union: tmpc_kernel_ms_total's arithmetic on n calls given in call order by lane, start and end time.
 */
int tmpc_debug_elastic_grid(const tmpc_handle *h, int32_t n_cu, int32_t lanes, int32_t wpb, int64_t B, int32_t *core, int32_t *eligible);
int tmpc_debug_surplus_yields(uint32_t followers, int32_t lanes);
int tmpc_debug_plan_lanes(int32_t nx, int32_t nu, int32_t N, int32_t lanes, int32_t n_calls, const int64_t *B, const void *const *ptrs,
                          int32_t *lane_out, int32_t *waited_out, int32_t *followers_out);
double tmpc_debug_busy_union(int32_t n, const int32_t *lane, const double *start, const double *end);
/*
 * Diagnostics (tests/test_call_hazards.py): the overlap rule itself, no device and no handle involved.  a and b are the nine
 * pointer arguments of two tmpc_solve_batch_device calls over B_a / B_b instances of a problem with nx, nu, N, in the order
 * of that function (x_k, ref, variant, u_nom, x_nom0, xu_ss, x_nom, status, iters; NULL: not given); nothing is
 * dereferenced.  Returns 1 when the later call must stay behind the earlier one, 0 when they may overlap, TMPC_E_INVALID.
 */
int tmpc_debug_calls_conflict(int32_t nx, int32_t nu, int32_t N, int64_t B_a, const void *const *a, int64_t B_b, const void *const *b);

/*
 * Device time of the solve kernel(s) of the most recent tmpc_solve_batch[_device]
 * call: from its own start to its own end, HIP events recorded on the call's stream
 * around its launches (waits for the call).  A call that overlapped with its neighbours
 * shows a longer time here than it would alone.
 */
int tmpc_last_kernel_ms(tmpc_handle *h, float *ms);

/*
 * Device time the handle was busy with the solve calls since the last reset, and their count (at most 4096 calls are
 * tracked between resets).  Every call adds the time by which it extended the handle's busy period: from the later of
 * {its own start event, the end event of the call that ended last among those before it} to its own end event.  For calls
 * that do not overlap -- one lane, tmpc_set_call_overlap(0), the closed loops -- that is each call's own start-to-end time,
 * the sum of what tmpc_last_kernel_ms reports; where calls overlap, the overlapped part counts once.
 * Synchronises the handle.  bench.py divides the two for the average device time per call.
 */
int tmpc_kernel_ms_total(tmpc_handle *h, float *total_ms, int32_t *launches, int reset);

/*
 * Introspection for DESIGN.md / bench.py's roofline accounting: dimensions of the
 * condensed QP of `variant` as the kernels see it.
 *   nv   decision variables after condensing
 *   nc   inequality rows kept (rows that cannot bind for any x_k are dropped)
 *   npar rows that depend on x_k only (checked once per instance, not iterated on)
 */
int tmpc_get_dims(const tmpc_handle *h, int variant, int32_t *nv, int32_t *nc, int32_t *npar);
/*
 * How the nc rows are stored: nd general ("dense") rows of width nv and one block of ncc rows of rank kc kept in factored
 * form Hc * Psi (the terminal set acts on [x_N; theta] only, TubeTrackingMPC.py:149; the initial-state set of the
 * packet-received problem on x_0 only, :278); nc = nd + ncc, ncc = kc = 0 when nothing is factored.  The figures are those of
 * the layout the variant's kernel reads: the wave kernel's lane packing moves the rows of a partly filled last slot of the
 * block to the dense class (cart-pole N = 10: 120 / 384 / 5; 92 / 412 / 5 with TMPC_NO_LANE_PACKING=1 in the environment of
 * tmpc_create), the workgroup-per-QP kernel keeps every row dense.  bench.py prices the
 * factored block at its rank in `roofline_factored`.  Added without an ABI bump: a new export, nothing else changed.
 */
int tmpc_get_factoring(const tmpc_handle *h, int variant, int32_t *nd, int32_t *ncc, int32_t *kc);

/*
 * Copies the condensed, unscaled QP data of `variant` to caller buffers (any may be
 * NULL): the QP is  min 1/2 z'Hz + (F1 x_k + F2 ref)'z  s.t.  G z <= g0 + E x_k.
 *   H nv*nv, F1 nv*nx, F2 nv*nx, G nc*nv, g0 nc, E nc*nx.   Used by the tests.
 */
int tmpc_get_condensed(const tmpc_handle *h, int variant,
                       double *H, double *F1, double *F2, double *G, double *g0, double *E);

/*
 * Offline stage: a batch of support-function linear programs over ONE polytope,
 *
 *        val[b] = max  C[b,:] . x   s.t.  H x <= h   (row relax[b] of h raised by relax_by)
 *
 * Replaces the one-at-a-time scipy.optimize.linprog calls of the reference's set
 * computations (reference src/LinearMPCOverNetworks/utils_polytope.py:12-23 `support`,
 * :19 the linprog call; used by the Gilbert-Tan recursion :247-268, the Pontryagin
 * difference :25-38, and the redundancy removal of polytope.reduce,
 * TubeRegulatorMPC.py:74).  One wavefront per LP: interior-point iterations handed over
 * to primal active-set steps, so that the value is the vertex value (csrc/tmpc_lp.hip).
 *
 *   d       dimension, 1 <= d <= 32           nr  rows of H (row-major nr x d), nr >= 1
 *   B       number of objectives              C   B x d, row-major
 *   relax   B row indices or NULL; relax[b] = -1 leaves h alone.  Row relax[b] is raised
 *           by relax_by IN THE UNITS OF h AS PASSED (the redundancy test of row i is
 *           "maximise H[i,:] x with h[i] + 1", polytope.reduce)
 *   val     B        x   B x d maximiser or NULL
 *   status  B  TMPC_STATUS_* (OPTIMAL: x feasible to 1e-11 max(|h_r|, 1), with multipliers
 *           y >= -1e-10 max(y) on active rows and |c - H'y|_inf <= 1e-11 |c| -- a point of
 *           the optimal face, or the interior-point iterate at gap 1e-12 and the same dual
 *           residual; MAX_ITER: last iterate without that certificate, accurate to about
 *           1e-8; INFEASIBLE; UNBOUNDED: val = +inf)
 *   iters   B  interior-point iterations
 * All pointers are HOST pointers (this is a set-up step; the data is small).  Errors:
 * negative TMPC_E_* code, text through tmpc_last_error(NULL).
 */
int tmpc_lp_batch(int device, int32_t d, int32_t nr, const double *H, const double *h,
                  int64_t B, const double *C, const int32_t *relax, double relax_by,
                  double *val, double *x, int32_t *status, int32_t *iters);

/*
 * Exact order statistics of columns of doubles, selected on the device (csrc/tmpc_west.hip: most-significant-digit radix
 * select on an order-preserving 64-bit key, six passes of 11 + 11 + 11 + 11 + 11 + 9 bits; ties need no care).
 *
 *   n, ncol   data is ncol columns of n values, column-major (column c at data + c n), HOST memory
 *   ranks     n_rank ranks in [0, n), the same for every column: rank r is element r of the sorted column (numpy.partition(col, r)[r])
 *   out       ncol x n_rank, row-major.  -0 and +0 compare equal and may come back with either sign.
 *   n_nonfinite  ncol counts (or NULL) of the values that are NaN or +-inf.  NaN have no order: they are left out, the ranks
 *             count through the other values, and a rank beyond them comes back as NaN.  +-inf are ordered and keep their place.
 * Errors: TMPC_E_INVALID (sizes, a rank out of range), TMPC_E_NOMEM (8 n ncol bytes of device memory), TMPC_E_DEVICE; text
 * through tmpc_last_error(NULL).  Added without an ABI bump: a new export, nothing else changed.
 */
int tmpc_order_statistics(int device, int64_t n, int32_t ncol, const double *data, int32_t n_rank, const int64_t *ranks,
                          double *out, int64_t *n_nonfinite);

/*
 * The disturbance set W of the linear model (A, B), estimated on the plant the model was derived from -- the procedure of the
 * reference's Results/estimate_W_for_Cartpole.py on the plant of tmpc_mc_set_plant (the closed-form cart-pole, RK4, `substeps`
 * steps per sampling period par7[6]; NOT the reference's PyBullet model): n_traj closed loops u = -K x of T sampling periods,
 * the force held over a period, and at every period boundary k = 1 .. T - 1 the one-step prediction error
 *
 *        w_k = x_k - (A - B K) x_{k-1}                                        (estimate_W_for_Cartpole.py:94-107)
 *
 * i.e. T - 1 samples per trajectory and component (the state after the last period is not sampled; the reference's leading
 * all-zero sample, :77, is not added).  One lane per trajectory; the samples stay on the device, where order statistics
 * of each component are selected as by tmpc_order_statistics (the reference's quantiles, :117-120).
 *
 *   nx, nu, plant   only TMPC_PLANT_CARTPOLE with nx = 4, nu = 1; anything else: TMPC_E_UNSUPPORTED
 *   A nx*nx, B nx*nu, K nu*nx (u = -K x), par7 = M, m, b, I, g, l, Th, substeps >= 1
 *   n_traj >= 1, T >= 2
 *   x0        n_traj x nx initial states, or NULL: trajectory b starts at x0_lo + (x0_hi - x0_lo) u (two roundings), u_i = (word_i >> 11) 2^-53
 *             of the four words of Philox4x64-10 with key (seed, first_trajectory + b), counter 0 -- a trajectory does not
 *             depend on how a sweep is split into calls
 *   ranks     n_rank ranks in [0, n_traj (T - 1)), the same for every component
 *   settle_tol  a trajectory with |x_T|_2 > settle_tol (or NaN) counts as not settled (the reference's check uses 1e-3, :110)
 * Outputs (host memory; any may be NULL):
 *   order_stats nx x n_rank      w_min, w_max  nx each: extremes of the finite samples (NaN without any)
 *   n_samples   n_traj (T - 1)   n_nonfinite   nx counts of NaN / +-inf samples (see tmpc_order_statistics)
 *   not_settled, x_final_norm_max (max |x_T|_2)      x0_used  n_traj x nx
 *   samples     nx x (T - 1) x n_traj: sample k of trajectory b, component i, at [i][k - 1][b] (for tests and small runs)
 *   kernel_ms   2 floats: device time of the rollout launch and of the selection launches (HIP events)
 * Errors: TMPC_E_INVALID (sizes, ranks), TMPC_E_NOMEM when the sample buffer of 8 nx (T - 1) n_traj bytes cannot be allocated
 * on the device, TMPC_E_DEVICE.  Nothing is launched after an argument error.  Added without an ABI bump: a new export.
 */
int tmpc_estimate_w(int device, int32_t nx, int32_t nu, const double *A, const double *B, const double *K,
                    int plant, const double *par7, int32_t substeps, int64_t n_traj, int32_t T,
                    const double *x0, const double *x0_lo, const double *x0_hi, uint64_t seed, int64_t first_trajectory,
                    int32_t n_rank, const int64_t *ranks, double settle_tol,
                    double *order_stats, double *w_min, double *w_max, int64_t *n_samples, int64_t *n_nonfinite,
                    int64_t *not_settled, double *x_final_norm_max, double *x0_used, double *samples, float *kernel_ms);

/*
 * tmpc_estimate_w with a plant per trajectory: par_traj is n_traj x 7 (HOST memory), row b the cart-pole of trajectory b; NULL: par7 for
 * every trajectory (tmpc_estimate_w is this call with NULL; par7 may be NULL when par_traj is given).  A, B and K stay nominal, so
 * w_k = x_k - (A - B K) x_{k-1} contains the parametric mismatch of the family: a box estimated this way covers it.  The rows are
 * validated (TMPC_E_INVALID naming trajectory and field: a non-finite entry, M, m, l or Th <= 0, I or b < 0).  Added without an ABI bump: a new export.
 */
int tmpc_estimate_w_models(int device, int32_t nx, int32_t nu, const double *A, const double *B, const double *K,
                           int plant, const double *par7, const double *par_traj, int32_t substeps, int64_t n_traj, int32_t T,
                           const double *x0, const double *x0_lo, const double *x0_hi, uint64_t seed, int64_t first_trajectory,
                           int32_t n_rank, const int64_t *ranks, double settle_tol,
                           double *order_stats, double *w_min, double *w_max, int64_t *n_samples, int64_t *n_nonfinite,
                           int64_t *not_settled, double *x_final_norm_max, double *x0_used, double *samples, float *kernel_ms);

/*
 * Sensitivity of the solution to its inputs: the Jacobian of y = [u_nom (N nu) | x_nom0 (nx) | xu_ss (nx + nu)] with respect to
 * p = [x_k | ref], and its transpose applied to a vector (the backward pass of a differentiable layer around tmpc_solve_batch_device).
 *
 * The minimiser of the condensed QP (tmpc_get_condensed; F = [F1 F2], Ebar = [E 0]) is piecewise affine in p.  On the critical region
 * of a given solution the law follows from one KKT solve on its working set A -- the rows with slack g0_i + E_i x_k - G_i z <= act_tol,
 * taken in ascending row order (act_tol <= 0 selects 1e-7, on unscaled rows):  M = G_A H^-1 G_A',
 *   lambda_A = -M^-1 (G_A H^-1 F p + g0_A + Ebar_A p),   dlambda/dp = -M^-1 (G_A H^-1 F + Ebar_A),   dz/dp = -H^-1 (F + G_A' dlambda/dp),
 * and J = Y dz/dp + Yp with the affine output map y = Y z + Yp p of the condensing (ny x 2 nx, ny = N nu + 2 nx + nu).
 * NOTHING IS SOLVED HERE: u_nom, x_nom0, xu_ss and status are the outputs of a preceding solve (or of any other solver of the same
 * problem), from which z is rebuilt.  One kernel launch per problem variant (csrc/tmpc_sens.hip).
 *
 * tmpc_sens_jacobian(h, B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, J, flag, n_active, active): HOST pointers.
 *   in   x_k, ref, variant (or NULL), u_nom, x_nom0, xu_ss, status (or NULL: every instance counts as solved): as tmpc_solve_batch
 *   out  J         B*ny*2nx   [B][ny][2 nx], row-major
 *        flag      B int32    TMPC_SENS_* bits, below
 *        n_active  B int32    rows of the working set after the rank test
 *        active    B*ceil(nc_max/32) uint32 or NULL: bit i (word i / 32, bit i % 32) is set when row i, in tmpc_get_condensed order of
 *                  the instance's variant, is in the working set after the rank test; nc_max = the largest nc of the handle's variants.
 *                  The words are the identity of the critical region.
 * tmpc_sens_vjp(h, B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, ybar, pbar, flag, n_active): pbar[b] = J_b' ybar[b],
 *   ybar [B][ny], pbar [B][2 nx], one right-hand side through the same system; J is not formed.
 * tmpc_sens_jacobian_device / tmpc_sens_vjp_device: the same with DEVICE pointers, under the ordering contract of tmpc_solve_batch_device:
 *   calls on a handle take effect as if executed in call order, and a call goes to the other launch lane than the call before it when none
 *   of its arrays -- read: x_k, ref, variant, u_nom, x_nom0, xu_ss, status, ybar; written: J / pbar, flag, n_active, active; by byte range --
 *   overlaps an array of the unfinished calls of that call's lane (solve calls and sensitivity calls alike).  Independent calls run side by
 *   side; a call that overlaps stays behind the call it depends on.  Returns without synchronising (tmpc_synchronize); as there, the
 *   handle's streams are not ordered against the caller's.  The calls count in tmpc_debug_lane_counters.
 * tmpc_last_kernel_ms after any of the four: the device time of the call's launches (they count as calls in tmpc_kernel_ms_total).
 *
 * Flags:
 *   TMPC_SENS_SKIPPED    status >= TMPC_STATUS_INFEASIBLE, a variant id out of range, or a non-finite input: the outputs are NaN,
 *                        n_active 0, no other bit
 *   TMPC_SENS_DEPENDENT  rows were dropped by the rank test: a row whose pivot in the row-by-row Cholesky factorisation of M falls to
 *                        rank_tol = 1e-10 times its own diagonal entry of M (and every candidate after nv rows are kept) is left out; the
 *                        derivative is that on the reduced set
 *   TMPC_SENS_WEAK       a working row's multiplier is <= mult_tol max(1, |lambda|_inf), mult_tol = 1e-9: the point lies on the boundary of
 *                        its region; the derivative written is the one-sided one with the row held active
 *   TMPC_SENS_NOT_KKT    the given point is not a KKT point of its working set: |H z + F p + G_A' lambda_A|_inf > kkt_tol (1 + |F p|_inf),
 *                        kkt_tol = 1e-6, or a multiplier below minus that; values are still written
 * The three tolerances are compile-time constants (csrc/tmpc_sens.hpp); LinearMPCOverNetworks/sensitivity.py is the numpy twin.
 *
 * Refused before anything touches the device: NULL arguments or B < 0 (TMPC_E_INVALID); an open stepped session (TMPC_E_INVALID); a
 * regulator handle (TMPC_E_UNSUPPORTED); a variant that keeps unpriced auxiliaries (extended, literal_terminal_row without HTP: the
 * outputs do not determine z; TMPC_E_UNSUPPORTED); a host-only handle (TMPC_E_DEVICE).  The model part (H^-1, G H^-1, H^-1 F, Y, Yp)
 * is computed and uploaded by the first sensitivity call of a handle; a handle that never asks allocates nothing.
 *
 * tmpc_qp_sensitivity(device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, B, P, Z, status, act_tol, mode, ybar, out, flag, n_active,
 *   active): the same launcher on raw condensed data, without a handle (errors through tmpc_last_error(NULL)); HOST pointers.
 *   H nv*nv (symmetric positive definite), F nv*np, G nc*nv, g0 nc, Ebar nc*np, Y ny*nv, Yp ny*np; P [B][np], Z [B][nv] the minimisers,
 *   status [B] or NULL; mode TMPC_SENS_JACOBIAN (out [B][ny][np]) or TMPC_SENS_VJP (ybar [B][ny], out [B][np]); active
 *   [B][ceil(nc/32)] or NULL.  Limits: 1 <= nv <= 128, 0 <= nc <= 2^20, 1 <= np <= 32, 1 <= ny <= 4096 (TMPC_E_INVALID beyond them, as
 *   for NULL arguments, B < 0 and an H that is not positive definite; device < 0: TMPC_E_DEVICE).
 * tmpc_sens_get_model(h, variant, F, Ebar, Y, Yp, Rec): what the handle entries hand the kernel beyond tmpc_get_condensed, for a caller
 *   who drives tmpc_qp_sensitivity or a host implementation with a handle's problem (any pointer may be NULL; works on a host-only handle):
 *   F nv*2nx = [F1 F2], Ebar nc*2nx = [E 0], Y ny*nv and Yp ny*2nx (y = Y z + Yp [x_k | ref]), Rec nv*(ny + 2nx): z = Rec [y | x_k | ref],
 *   the map back from a solve's outputs (theta by least squares from xu_ss).  Refusals as above.
 * Added without an ABI bump: new exports, nothing else changed.
 *
 * Gradients with respect to the weights Q, R, P, T of tmpc_problem, summed over the batch (K, K_anc and all sets held fixed; the four
 * count as independent symmetric parameters of the QP -- a caller who ties P to (Q, R) chains through their own Riccati code).  With
 * v = Y' ybar_b the reverse mode solves [H G_A'; G_A 0] [a_b; q_b] = [v; 0] on the working set; for a loss l(y)
 *   dl = -a' dH z - a' dF p   =>   Hbar = -1/2 sum_b (a_b z_b' + z_b a_b'),   Fbar = -sum_b a_b p_b'
 * (dH symmetric), and H, F are linear in the weights: H = 2 sum L'W L, F1 = 2 sum L'W Dx, F2 = 2 sum L'W Dr over the error signals
 * e = L z + Dx x_k + Dr ref priced with W, so  Wbar = sym(2 sum (L Hbar L' + L F1bar Dx' + L F2bar Dr')).  SKIPPED instances add nothing.
 * The sums over b run in a fixed order (chunks of 256 instances, then the chunks in order; no atomics): two calls give equal bytes.
 *
 * tmpc_sens_vjp_weights(h, B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, ybar, pbar, Qbar, Rbar, Pbar, Tbar, flag, n_active):
 *   HOST pointers.  pbar, flag, n_active: the bytes tmpc_sens_vjp writes for the same inputs.  Qbar nx*nx, Rbar nu*nu, Pbar nx*nx,
 *   Tbar nx*nx: symmetric, any of the four may be NULL; on an extended handle the contributions of both variants are added.
 * tmpc_sens_vjp_weights_device: the per-instance arrays (x_k .. n_active) are DEVICE pointers under the ordering contract of
 *   tmpc_sens_vjp_device (same ranges read and written; the call counts in tmpc_debug_lane_counters).  Qbar, Rbar, Pbar, Tbar are HOST
 *   pointers: the call returns once they are in place, after it has synchronised ITS OWN launch lane (the map from Hbar, Fbar to the
 *   weights is a few MFLOP on an nv x (nv + 2 nx) block and runs on the host).  pbar, flag, n_active are complete then as well.
 *   Workspace per lane: 2 B nv + ceil(B / 256) nv (nv + 2 nx) doubles.
 * Refusals: those of tmpc_sens_vjp / tmpc_sens_vjp_device.
 * tmpc_sens_weight_map(h, variant, Hbar, Fbar, Qbar, Rbar, Pbar, Tbar): the map alone, on the host (works on a host-only handle):
 *   Hbar nv*nv, Fbar nv*2nx = [F1bar F2bar] in; symmetric matrices out, any may be NULL.  Under a terminal equality the terminal error
 *   x_N - x_bar is zero, so Pbar = 0.  Refused: NULL handle, Hbar or Fbar, a variant out of range (TMPC_E_INVALID); a regulator handle, a
 *   variant that keeps unpriced auxiliaries (TMPC_E_UNSUPPORTED).
 * tmpc_qp_sensitivity_data(device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, B, P, Z, status, act_tol, ybar, pbar, Hbar, Fbar, adj, flag,
 *   n_active): the handle-free entry on raw condensed data, beside tmpc_qp_sensitivity (same limits and refusals; HOST pointers):
 *   pbar [B][np] (or NULL) as tmpc_qp_sensitivity(mode = VJP) writes it, Hbar nv*nv (symmetric), Fbar nv*np, adj [B][nv] (or NULL) the a_b.
 *   The a_b behind Hbar, Fbar and adj take one step of refinement on the constraint rows, a = a0 - W_A' M^-1 (G_A a0) with a0 the a_b behind
 *   pbar (the exact a_b has G_A a_b = 0; with |A| = nv it is zero); pbar is that of tmpc_sens_vjp, untouched.
 */
#define TMPC_SENS_SKIPPED   0x1
#define TMPC_SENS_DEPENDENT 0x2
#define TMPC_SENS_WEAK      0x4
#define TMPC_SENS_NOT_KKT   0x8
#define TMPC_SENS_JACOBIAN  0
#define TMPC_SENS_VJP       1
int tmpc_sens_jacobian(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                       const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, double *J, int32_t *flag,
                       int32_t *n_active, uint32_t *active);
int tmpc_sens_jacobian_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                              const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, double *J, int32_t *flag,
                              int32_t *n_active, uint32_t *active);
int tmpc_sens_vjp(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                  const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                  int32_t *flag, int32_t *n_active);
int tmpc_sens_vjp_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                         const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                         int32_t *flag, int32_t *n_active);
int tmpc_sens_get_model(tmpc_handle *h, int variant, double *F, double *Ebar, double *Y, double *Yp, double *Rec);
int tmpc_sens_vjp_weights(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                          const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                          double *Qbar, double *Rbar, double *Pbar, double *Tbar, int32_t *flag, int32_t *n_active);
int tmpc_sens_vjp_weights_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                                 const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                                 double *Qbar, double *Rbar, double *Pbar, double *Tbar, int32_t *flag, int32_t *n_active);
int tmpc_sens_weight_map(tmpc_handle *h, int variant, const double *Hbar, const double *Fbar, double *Qbar, double *Rbar, double *Pbar, double *Tbar);
int tmpc_qp_sensitivity_data(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
                             const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t B, const double *P, const double *Z,
                             const int32_t *status, double act_tol, const double *ybar, double *pbar, double *Hbar, double *Fbar, double *adj,
                             int32_t *flag, int32_t *n_active);
int tmpc_qp_sensitivity(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
                        const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t B, const double *P, const double *Z,
                        const int32_t *status, double act_tol, int mode, const double *ybar, double *out, int32_t *flag, int32_t *n_active,
                        uint32_t *active);

/*
 * The explicit control law: a table of critical regions per problem variant, evaluated on the device (csrc/tmpc_law.hip), with the
 * handle's ordinary solve as the fallback for the instances no stored region holds.
 *
 * On the critical region of a working set A (rows of tmpc_get_condensed; the bit words `active` of tmpc_sens_jacobian) the minimiser
 * is affine in p = [x_k | ref]: with M = G_A H^-1 G_A' and W = G H^-1,
 *   lambda_A(p) = Kl p + kl,  Kl = -M^-1 (W_A F + Ebar_A),  kl = -M^-1 g0_A;   z(p) = Kz p + kz,  Kz = -H^-1 (F + G_A' Kl),  kz = -H^-1 G_A' kl;
 *   y(p) = Ky p + ky,  Ky = Y Kz + Yp,  ky = Y kz          (y = [u_nom | x_nom0 | xu_ss], the output map of tmpc_sens_get_model).
 * The region's polyhedron S p + s >= 0 has nrow = nc + npar rows, in this order: row i < nc outside A is the primal slack
 * g0_i + Ebar_i p - G_i z(p) + TMPC_LAW_FEAS_TOL; row i < nc inside A is its multiplier lambda_i(p) + TMPC_LAW_MULT_TOL; row nc + j is the
 * parameter-only row gp0_j + Ep_j x_k + TMPC_LAW_FEAS_TOL (tmpc_get_param_rows).  Acceptance of p by a region is the KKT test of the
 * strictly convex QP, so an accepted instance gets THE minimiser: a table that is incomplete, badly ordered or built from doubtful
 * working sets costs speed, never correctness.  The two thresholds are compile-time constants (csrc/tmpc_law.hpp), absolute, on the
 * unscaled rows; LinearMPCOverNetworks/explicit_law.py is the numpy twin.  A region is built in double on the host with a Cholesky
 * factorisation of M; a set whose M is not positive definite is refused (id -1).  The empty set is a valid region.
 *
 * Per handle and variant the table keeps stable region ids 0 .. R-1 (insertion order; a set already stored keeps its id), a hit
 * counter per region in device memory, and a search order (a permutation of the ids, insertion order until tmpc_law_reorder).  The
 * first tmpc_law_* call allocates; a handle that never asks allocates nothing.  Growth beyond the device's memory: TMPC_E_NOMEM, the
 * table as it was.
 *
 * tmpc_law_add(h, variant, n_sets, words, ids): HOST pointers; words [n_sets][ceil(nc/32)] of that variant, ids [n_sets] or NULL.  Waits
 *   for the handle's launch lanes first.  Works on a host-only handle (for tmpc_law_get_region).
 * tmpc_law_learn(h, B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, ids, n_new): HOST pointers, the inputs and outputs of a
 *   preceding solve.  Runs the sensitivity kernel for the signatures and adds every one whose flag has neither TMPC_SENS_SKIPPED nor
 *   TMPC_SENS_NOT_KKT (WEAK and DEPENDENT sets are admissible: acceptance certifies).  ids [B] or NULL: the region of each instance, -1
 *   where none was added; n_new or NULL: regions that were new.
 * tmpc_law_eval(h, B, x_k, ref, variant, hint, max_tries, u_nom, x_nom0, xu_ss, x_nom, status, iters, region, tries): HOST pointers, the law
 *   kernel alone.  Inputs and outputs as tmpc_solve_batch, and
 *     hint      B int32 or NULL   the region tried first where it is a valid id (last step's region of a closed loop)
 *     max_tries                   candidates tested per instance at most, the hint included; <= 0: all
 *     region    B int32           the id of the region that holds the instance, -1: none (a miss)
 *     tries     B int32 or NULL   candidates tested
 *   A hit has status TMPC_STATUS_OPTIMAL and iters 0; x_nom is the rollout x_{i+1} = A x_i + B u_i from x_nom0.  A miss has NaN outputs and
 *   status TMPC_STATUS_NUMERICAL; so has an instance with a non-finite input or a variant id out of range (tries 0).  x_nom, iters,
 *   hint and tries may be NULL.  An empty table is no error: everything misses.
 * tmpc_law_solve: the same arguments (iters is required); the misses, and only they, go through the handle's solve kernels in the same
 *   call -- the law kernel writes a selector byte per instance, and the solve launches that follow on the same launch lane skip every
 *   instance it has answered.  No host synchronisation, no gather or scatter, no copy.  Every instance is answered as by
 *   tmpc_solve_batch; region tells which came from the table.
 * tmpc_law_eval_device / tmpc_law_solve_device: the same with DEVICE pointers, under the ordering contract of tmpc_solve_batch_device (read:
 *   x_k, ref, variant, hint; written: u_nom, x_nom0, xu_ss, x_nom, status, iters, region, tries).  They return without synchronising and
 *   count in tmpc_debug_lane_counters, tmpc_last_kernel_ms and tmpc_kernel_ms_total.
 * tmpc_law_get_stats(h, variant, R, hits): the number of regions and (hits [R] or NULL) the hit counters; waits for the lanes.
 * tmpc_law_reorder(h, variant): sorts the search order by descending hits, ties by id; the ids stay.  Waits for the lanes.
 * tmpc_law_clear(h, variant): empties the table and its counters.
 * tmpc_law_get_region(h, variant, id, words, Ky, ky, S, s): the region as uploaded -- words [ceil(nc/32)], Ky [ny][2 nx], ky [ny],
 *   S [nrow][2 nx], s [nrow] (tolerances folded in); any pointer may be NULL.  tmpc_get_param_rows(h, variant, gp0, Ep): the npar rows
 *   0 <= gp0 + Ep x_k (npar from tmpc_get_dims; Ep [npar][nx]).  Both work on a host-only handle.
 * tmpc_qp_law_eval(device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, n_sets, words, n_order, order, B, P, hint, max_tries, out_y, region,
 *   tries): the same kernel on raw condensed data without a handle (errors through tmpc_last_error(NULL)); HOST pointers.  The model as
 *   for tmpc_qp_sensitivity, no parameter-only rows; words [n_sets][ceil(nc/32)], set i is region i (a refused set stays in the table as
 *   a region that holds no p); order [n_order] ids; P [B][np]; out_y [B][ny] (NaN for a miss); hint and tries may be NULL.  Limits:
 *   1 <= nv <= 128, 0 <= nc <= 2^20, 1 <= np <= 32, 1 <= ny <= 4096, n_sets and n_order <= 2^20.
 *
 * Hops.  A candidate that fails tells where to look next: row i < nc of its polyhedron is the slack (i outside the working set) or the
 * multiplier (i inside) of constraint i, so the region across the facet of a failing row i has the working set with bit i flipped.
 *   The key of a working set A is the XOR over i in A of z(i), z = splitmix64 of i + 1:
 *     x = (i + 1) * 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *   (64-bit, wrapping); the empty set has key 0, and the neighbour across row i has key(A) ^ z(i) whichever side i is on.  Per table the
 *   device holds key [R] and an open-addressed table slot [n_slot] of int32 ids, -1 for empty: n_slot is the power of two >= max(64, 2 R),
 *   ids are inserted in increasing order at key & (n_slot - 1) with linear probing, a key already present keeps the earlier id, a lookup
 *   compares key[slot[j]] and stops at an empty slot.  A 64-bit collision costs one wasted test, never an answer.  The host builds both
 *   wherever the table changes (tmpc_law_add, tmpc_law_learn, tmpc_law_clear; tmpc_law_reorder leaves them alone).
 * tmpc_law_set_hops(h, max_hops) / tmpc_law_get_hops(h, &max_hops): a handle-wide setting, 0 by default, read by tmpc_law_eval[_device],
 *   tmpc_law_solve[_device] and the loops of tmpc_mc_set_law (at the start of a run; a session at its open).  With max_hops > 0 the search
 *   of an instance is a CHAIN, then the walk:
 *     the chain starts at the hint where it is a valid id, otherwise at order[0], otherwise there is none.  The current region r is tested
 *     (it counts in tries); if it accepts, it is the answer.  Otherwise, with i the LOWEST failing row (a NaN row fails), the chain ends
 *     if -- looked at in this order -- i >= nc (a parameter-only row); r has no key (a refused set of tmpc_qp_law_eval_hops); the
 *     neighbour's key is absent from the hash; the neighbour is the region tested immediately before r (a two-cycle); max_hops hops have
 *     been made; max_tries > 0 candidates have been tested.  Otherwise r becomes the neighbour.
 *     The walk is the search order without the chain's start, under the same max_tries; regions the chain visited may be tested again.
 *   Acceptance is the KKT test, so whatever the chain finds is the minimiser, and nothing that hits without hops can miss with them.
 *   max_hops = 0 is the search described above, unchanged.  The setter waits for the launch lanes; max_hops < 0 and an open session:
 *   TMPC_E_INVALID; a regulator handle: TMPC_E_UNSUPPORTED; on a host-only handle it only stores the value.
 * tmpc_law_get_hop_stats(h, variant, stats) / tmpc_law_clear_hop_stats(h, variant): six counters per variant in device memory, added to
 *   with max_hops > 0 only -- stats[0] chains that hit (the start's own hit included), [1] regions the chains tested, chains ended [2] by an
 *   absent neighbour, [3] by max_hops, [4] by a two-cycle, [5] by a parameter-only row; a chain ended by max_tries or at a region without
 *   a key counts in none of [2..5].  Both wait for the lanes; tmpc_law_clear clears the variant's counters too; zeros on a host-only handle.
 * tmpc_law_find_key(h, variant, key, &id): the id the host's hash holds under a key, -1: none.  Works on a host-only handle.
 * tmpc_qp_law_eval_hops: the arguments of tmpc_qp_law_eval, then max_hops >= 0 and stats (int64 [6] or NULL); tmpc_qp_law_eval is this
 *   entry at max_hops = 0.
 *
 * Refused before anything touches the device: NULL arguments or B < 0 (TMPC_E_INVALID); an open stepped session (TMPC_E_INVALID); a
 * regulator handle (TMPC_E_UNSUPPORTED); a variant that keeps unpriced auxiliaries (TMPC_E_UNSUPPORTED); for the evaluating entries and
 * tmpc_law_learn a host-only handle (TMPC_E_DEVICE).  Added without an ABI bump: new exports, nothing else changed.
 */
#define TMPC_LAW_FEAS_TOL 1e-10
#define TMPC_LAW_MULT_TOL 1e-10
int tmpc_law_add(tmpc_handle *h, int variant, int64_t n_sets, const uint32_t *words, int32_t *ids);
int tmpc_law_learn(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom, const double *x_nom0,
                   const double *xu_ss, const int32_t *status, double act_tol, int32_t *ids, int64_t *n_new);
int tmpc_law_eval(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries, double *u_nom,
                  double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries);
int tmpc_law_eval_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries,
                         double *u_nom, double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries);
int tmpc_law_solve(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries, double *u_nom,
                   double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries);
int tmpc_law_solve_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries,
                          double *u_nom, double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries);
int tmpc_law_get_stats(tmpc_handle *h, int variant, int32_t *R, int64_t *hits);
int tmpc_law_reorder(tmpc_handle *h, int variant);
int tmpc_law_clear(tmpc_handle *h, int variant);
int tmpc_law_get_region(tmpc_handle *h, int variant, int32_t id, uint32_t *words, double *Ky, double *ky, double *S, double *s);
int tmpc_get_param_rows(tmpc_handle *h, int variant, double *gp0, double *Ep);
int tmpc_qp_law_eval(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G, const double *g0,
                     const double *Ebar, const double *Y, const double *Yp, int64_t n_sets, const uint32_t *words, int64_t n_order, const int32_t *order,
                     int64_t B, const double *P, const int32_t *hint, int max_tries, double *out_y, int32_t *region, int32_t *tries);
int tmpc_law_set_hops(tmpc_handle *h, int max_hops);
int tmpc_law_get_hops(tmpc_handle *h, int *max_hops);
int tmpc_law_get_hop_stats(tmpc_handle *h, int variant, int64_t *stats);
int tmpc_law_clear_hop_stats(tmpc_handle *h, int variant);
int tmpc_law_find_key(tmpc_handle *h, int variant, uint64_t key, int32_t *id);
int tmpc_qp_law_eval_hops(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G, const double *g0,
                          const double *Ebar, const double *Y, const double *Yp, int64_t n_sets, const uint32_t *words, int64_t n_order, const int32_t *order,
                          int64_t B, const double *P, const int32_t *hint, int max_tries, double *out_y, int32_t *region, int32_t *tries, int max_hops,
                          int64_t *stats);

/*
 * The closed loops through the explicit law.  A trajectory returns to the same few regions step after step, and inside a loop the law has
 * the hint that makes it cheap: the region of the step before.
 *
 * tmpc_mc_set_law: with on != 0 the following tmpc_mc_run, tmpc_mc_run_plants and tmpc_mc_open look [x_hat | ref_k] of every trajectory up
 * in the handle's table (of the problem the step would solve) before each solve, and solve the misses only.  The hint of trajectory b at
 * step t is its region at step t-1; -1 at t = 0 and after a miss (with tmpc_law_set_hops > 0 such a step chains from order[0]; tries
 * include the chains' tests).  At most max_tries candidates are tried per step, the hint included
 * (<= 0: all).  The table is the handle's at the start of the run; a session honours the setting as it was at open.  A hit writes what
 * tmpc_law_eval writes -- u_nom, x_nom0, xu_ss, status TMPC_STATUS_OPTIMAL, iters 0 -- which the state machines read as after a solve,
 * counts in the region's hit counter (tmpc_law_get_stats), and with warm start on leaves the trajectory's working-set record as it is.
 * A trajectory that has stopped is passed over.  tmpc_mc_run with one problem on the one-wave-per-QP kernel still takes one launch for the
 * sweep by the TMPC_MC_FUSED_* rule (tmpc_mc_last_fused: 1) where the problem's kernel shape has a factored block (the cart-pole's
 * shapes); every other loop takes per step the law's launch, the solve launches of the misses and the state-machine launch -- the extended
 * controller too (tmpc_mc_last_fused: 0).  Both forms give the same bytes.
 * miss_capacity >= 0: the rows of the miss log.  Works on a host-only handle, where it only stores the setting.  TMPC_E_INVALID while a
 * session is open and for miss_capacity < 0; TMPC_E_UNSUPPORTED on a regulator handle -- and, reported by the run, for a problem that
 * keeps the unpriced auxiliaries of the literal terminal row.  tmpc_mc_replay and tmpc_reg_run ignore the setting.  With the law off
 * every loop is what it was.
 *
 * tmpc_mc_get_law_stats: per trajectory of the last such loop, or of the session tmpc_mc_close just ended: the steps answered from the
 * table, the candidates tested in total, and the region of the last step taken (-1: a miss).  Any of the three may be NULL.
 * TMPC_E_INVALID where there is no such loop, the law was off, or B differs.
 *
 * tmpc_mc_get_law_misses: the log of the same loop -- [x_hat | ref_k] (x_k [.][nx], ref [.][nx]) and problem id of the steps that missed,
 * exactly as the law read them, appended on the device through one counter.  The log keeps the first miss_capacity entries drawn and the
 * counter goes on counting: *n_total is the number of misses of the run, and min(n_total, miss_capacity, capacity) rows come back.  The
 * order of the rows is not defined.  Solved and handed to tmpc_law_learn, the log of a pilot sweep is the table of the sweep that follows.
 */
int tmpc_mc_set_law(tmpc_handle *h, int on, int max_tries, int64_t miss_capacity);
int tmpc_mc_get_law_stats(tmpc_handle *h, int64_t B, int32_t *hits, int64_t *tries, int32_t *region_last);
int tmpc_mc_get_law_misses(tmpc_handle *h, int64_t capacity, int64_t *n_total, double *x_k, double *ref, uint8_t *variant);

#ifdef __cplusplus
}
#endif
#endif /* TMPC_H */
