"""Regulator MPC on the double integrator -- the scenario of the reference's
"Examples of Model Predictive Controllers/Example_of_Regulator_MPC.py" run through this package: same class, same calls,
the QP of every time step solved on the MI355X.

    python examples/regulator_mpc.py

Drives x0 = (1, 3) to the origin with |u| <= 1 in 20 steps (horizon N = 10, Q = I, R = 1, no state constraint), one solve
per step as the reference does, then runs the same loop for a batch of initial states on the device (run_closed_loop) and
checks it against the step-by-step loop.  Prints what the reference script plots: the input range against U and the final
state."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "robust-tracking-mpc-over-lossy-networks_amd"))
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC                 # noqa: E402
from LinearMPCOverNetworks.polytope_lite import Polytope                   # noqa: E402  (stands in for polytope.Polytope)


def main():
    A = np.array([[1.0, 1.0], [0.0, 1.0]])
    B = np.array([[0.0], [1.0]])
    nx, nu, N, T = 2, 1, 10, 20
    U = Polytope(np.array([[1.0], [-1.0]]), np.ones(2))
    mpc = RegulatorMPC(A, B, np.eye(nx), np.eye(nu), N)
    mpc.set_input_constraints(U)
    mpc.generate_optimization_problem()

    x = np.array([1.0, 3.0])
    x_traj, u_traj = [x], []
    for _ in range(T):
        _, u_mpc = mpc.solve_optimization_problem(x)
        u = u_mpc[:, 0]
        x = A @ x + B @ u
        x_traj.append(x)
        u_traj.append(u)
    x_traj, u_traj = np.array(x_traj), np.array(u_traj)
    print(f"regulator MPC: {T} steps from x0 = (1, 3): max |u_t| = {np.abs(u_traj).max():.4f} (U = [-1, 1]), "
          f"|x_T| = {np.linalg.norm(x_traj[-1]):.2e}")
    if np.abs(u_traj).max() > 1.0 + 1e-7:
        print("Input constraints violated")

    # the same loop for 256 initial states at once, resident on the device; trajectory 0 starts at (1, 3)
    rng = np.random.default_rng(0)
    x0 = np.r_[[[1.0, 3.0]], rng.uniform(-4.0, 4.0, (255, nx))]
    out = mpc.run_closed_loop(x0, T, capture=0)
    dev = float(np.max(np.abs(out["x_traj"] - x_traj)))
    print(f"regulator MPC device loop: 256 trajectories x {T} steps, input constraint violations {int(out['u_viol'].sum())}, "
          f"infeasible solves {int((out['fail_step'] >= 0).sum())}, max |x_t - step-by-step loop| = {dev:.1e}")


if __name__ == "__main__":
    main()
