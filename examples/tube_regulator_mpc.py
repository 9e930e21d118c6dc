"""Tube regulator MPC (Mayne, Seron and Rakovic 2005) on the disturbed double integrator -- the scenario of the reference's
"Examples of Model Predictive Controllers/Example_of_Tube_Regulator_MPC.py" (figure 2 of the paper) run through this
package: same class, same calls, the QP of every time step solved on the MI355X.

    python examples/tube_regulator_mpc.py [--mc 4096] [--T 30]

A = [[1, 1], [0, 1]], B = [0.5, 1]', Q = I, R = 0.01, N = 9, U = [-1, 1], X = {|x_1| <= 10, -10 <= x_2 <= 2}, W = 0.1-box,
x0 = (-5, -2).  The 10 steps of the reference script, then a Monte Carlo of the tube guarantee: trajectories from random
feasible initial states, disturbances drawn on the device uniformly in W, every step checked against X, U and the tube
x_nom + Z."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "robust-tracking-mpc-over-lossy-networks_amd"))
from LinearMPCOverNetworks.TubeRegulatorMPC import TubeRegulatorMPC         # noqa: E402
from LinearMPCOverNetworks.polytope_lite import Polytope                   # noqa: E402  (stands in for polytope.Polytope)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mc", type=int, default=4096)
    ap.add_argument("--T", type=int, default=30)
    args = ap.parse_args()
    rng_w = np.random.default_rng(1)
    A = np.array([[1.0, 1.0], [0.0, 1.0]])
    B = np.array([[0.5], [1.0]])
    nx, nu, N, T = 2, 1, 9, 10
    W = Polytope(np.r_[np.eye(nx), -np.eye(nx)], 0.1 * np.ones(2 * nx))
    U = Polytope(np.array([[1.0], [-1.0]]), np.ones(2))
    X = Polytope(np.r_[np.eye(nx), -np.eye(nx)], np.array([10.0, 2.0, 10.0, 10.0]))
    mpc = TubeRegulatorMPC(A, B, np.eye(nx), 0.01 * np.eye(nu), N)
    mpc.set_input_constraints(U)
    mpc.set_state_constraints(X)
    mpc.setup_optimization(W)
    K = mpc.get_controller_gain()
    Z = mpc.get_minimum_robust_positively_invariant_set()
    print(f"tube regulator MPC: Z has {Z.A.shape[0]} rows, Xf {mpc._Xf.A.shape[0]} rows, K = {np.round(K, 4).tolist()}")

    x = np.array([-5.0, -2.0])
    in_tube = in_X = in_U = 0
    for _ in range(T):
        x_mpc, u_mpc = mpc.solve_optimization_problem(x)
        x_nom = x_mpc[:, 0]
        u = u_mpc[:, 0] - K @ (x - x_nom)
        in_tube += Z.contains(x - x_nom)
        in_X += X.contains(x)
        in_U += U.contains(u)
        x = A @ x + B @ u + rng_w.uniform(-0.1, 0.1, nx)
    print(f"tube regulator MPC: {T} steps from x0 = (-5, -2): x - x_nom in Z at {in_tube} of {T} steps, x in X at {in_X}, "
          f"u in U at {in_U}; |x_T| = {np.linalg.norm(x):.3f}")

    # Monte Carlo of the tube guarantee on the device: initial states the controller accepts, w uniform in W
    rng = np.random.default_rng(3)
    cand = np.c_[rng.uniform(-8.0, 4.0, 4 * args.mc), rng.uniform(-3.0, 2.0, 4 * args.mc)]
    x_mpc, _ = mpc.solve_optimization_problem(cand)
    x0 = cand[~np.isnan(x_mpc[:, 0, 0])][:args.mc]
    out = mpc.run_closed_loop(x0, args.T, seed=2005)
    print(f"tube regulator MPC Monte Carlo: {x0.shape[0]} trajectories x {args.T} steps: tube violations "
          f"{int(out['tube_viol'].sum())}, X violations {int(out['x_viol'].sum())}, U violations {int(out['u_viol'].sum())}, "
          f"infeasible solves {int((out['fail_step'] >= 0).sum())}, mean cost {out['cost'].mean():.2f}")


if __name__ == "__main__":
    main()
