"""From the disturbance set to the closed loop, every stage on the device: estimate W for the cart-pole the loop really runs
(montecarlo.estimate_disturbance_box: the reference's Results/estimate_W_for_Cartpole.py on the RK4 plant), build the controller's
sets with that W (setup_optimization on the batched LP kernel), run the remote tube MPC on the nonlinear plant, and count the steps at
which x - x_nom left the tube Z -- next to the same count with the constants of workloads.cartpole(), which were calibrated on the
reference's PyBullet plant.

    python examples/estimate_w_for_cartpole.py [--n-traj 4096] [--mc 64] [--steps 200]

The counts are reported, not promised: a box that discards 2.5 % of the samples guarantees nothing, and the estimate comes from
regulation to the origin while the loop below tracks a reference over a lossy network."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "robust-tracking-mpc-over-lossy-networks_amd"))
from LinearMPCOverNetworks import control_lite, montecarlo, polytope_lite, workloads     # noqa: E402
from LinearMPCOverNetworks.TubeTrackingMPC import TubeTrackingMPC                        # noqa: E402
from LinearMPCOverNetworks.polytope_lite import box2poly                                 # noqa: E402


def closed_loop(model, w_bound, n_mc, T, N=10):
    mpc = TubeTrackingMPC(model["A"], model["B"], model["Q"], model["R"], N)
    mpc.set_input_constraints(model["U"])
    mpc.set_state_constraints(model["X"])
    old = polytope_lite.set_lp_backend("hip")
    try:
        with contextlib.redirect_stdout(io.StringIO()):                                  # the reference's progress prints
            mpc.setup_optimization(box2poly(np.c_[-w_bound, w_bound]), fixed_initial_state=True, rpi_method=1)
    finally:
        polytope_lite.set_lp_backend(old)
    p_loss = np.tile([0.0, 0.3, 0.6, 0.9], n_mc // 4)
    th, ga, dist = montecarlo.draw_realisations(len(p_loss), T, w_bound, seed=31)
    # the mismatch between the linear model and the plant is the disturbance: nothing is added to it
    return mpc.run_closed_loop(p_loss, 0.5 * np.ones(T), th, ga, 0.0 * dist, plant="cartpole")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-traj", type=int, default=4096)
    ap.add_argument("--mc", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    model = workloads.cartpole()
    K, _, _ = control_lite.dlqr(model["A"], model["B"], model["Q"], model["R"])
    est = montecarlo.estimate_disturbance_box(model["A"], model["B"], K, T=400, x0_box=montecarlo.W_REFERENCE_X0_BOX, n_traj=args.n_traj, seed=456)
    print(f"W estimated from {args.n_traj} x 400 periods on the device ({est['rollout_ms']:.2f} + {est['selection_ms']:.2f} ms):")
    print(f"  w_bound = {est['w_bound']}  (extremes {np.maximum(-est['min'], est['max'])}; not settled: {est['not_settled']})")
    print(f"  workloads.cartpole(): {model['w_bound']}")
    for name, wb in (("estimated W", est["w_bound"]), ("hard-coded W", model["w_bound"])):
        out = closed_loop(model, np.asarray(wb, dtype=np.float64), args.mc, args.steps)
        print(f"{name}: tube violations {int(out['tube_violations'].sum())} in {args.mc} x {args.steps} steps "
              f"({int((out['tube_violations'] > 0).sum())} trajectories), solves that were not optimal {int(out['not_optimal'].sum())}, "
              f"mean tracking error {out['tracking_error'].mean():.4f}")


if __name__ == "__main__":
    main()
