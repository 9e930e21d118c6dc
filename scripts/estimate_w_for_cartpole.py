#!/usr/bin/env python3
"""The reference's Results/estimate_W_for_Cartpole.py on the plant of the device closed loop: closed loops u = -K x on the nonlinear
cart-pole from random initial states, the one-step prediction error w_k = x_k - (A - B K) x_{k-1} of the linearised model, and the
interval each component lies in once the `--discard` fraction of its largest absolute values is dropped.

    python scripts/estimate_w_for_cartpole.py [--n-traj 100] [--periods 400] [--discard 0.025] [--seed 456] [--host] [--device-draws]
                                           [--plant-spread S]

Defaults: the reference's scenario -- seed 456, its box of initial states, 100 trajectories of 400 sampling periods (its 4000 physics
steps), initial states drawn like its four scalar draws per trajectory.  --host: the numpy twin instead of the device.
--device-draws: the initial states come from the device's Philox streams (sweeps too large to draw on the host).
--plant-spread S: every trajectory on its own cart-pole (montecarlo.sample_cartpole: M, m, l within +-S of nominal, cart friction
up to S; tmpc_estimate_w_models) while A, B and K stay nominal -- the box then covers the parametric mismatch of that family.

The plant is the closed-form cart-pole integrated with RK4 at 500 Hz (workloads.cartpole_step, TMPC_PLANT_CARTPOLE), not the
reference's PyBullet model: the numbers are this plant's, no replication of the constants in workloads.cartpole().  Unlike the
reference, no all-zero sample is put in front of the samples."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "robust-tracking-mpc-over-lossy-networks_amd"))
from LinearMPCOverNetworks import control_lite, montecarlo, workloads          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-traj", type=int, default=100)
    ap.add_argument("--periods", type=int, default=400)
    ap.add_argument("--discard", type=float, default=0.025)
    ap.add_argument("--seed", type=int, default=456)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device-draws", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--plant-spread", type=float, default=None, metavar="S")
    args = ap.parse_args()
    model = workloads.cartpole()
    A, B = model["A"], model["B"]
    K, _, _ = control_lite.dlqr(A, B, model["Q"], model["R"])                 # estimate_W_for_Cartpole.py:55-58
    box = montecarlo.W_REFERENCE_X0_BOX
    par = None if args.plant_spread is None else montecarlo.sample_cartpole(args.n_traj, args.plant_spread, args.seed)
    t0 = time.perf_counter()
    if args.host:
        x0 = (montecarlo.draw_initial_states_philox(args.n_traj, *box, seed=args.seed) if args.device_draws
              else montecarlo.reference_initial_states(args.n_traj, args.seed))
        out = montecarlo.estimate_disturbance_box_host(A, B, K, x0, args.periods, discard=args.discard, par=par)
    elif args.device_draws:
        out = montecarlo.estimate_disturbance_box(A, B, K, T=args.periods, discard=args.discard, x0_box=box, n_traj=args.n_traj,
                                                  seed=args.seed, device=args.device, par=par)
    else:
        out = montecarlo.estimate_disturbance_box(A, B, K, x0=montecarlo.reference_initial_states(args.n_traj, args.seed), T=args.periods,
                                                  discard=args.discard, device=args.device, par=par)
    wall = time.perf_counter() - t0
    if out["not_settled"]:
        print(f"System not stabilized in {out['not_settled']} of {args.n_traj} simulations (max |x_T| = {out['x_final_norm_max']:.3e})")
    if np.any(out["n_nonfinite"]):
        print(f"non-finite samples per component: {out['n_nonfinite']}")
    for c in range(4):
        print(f"w_{c + 1} in [{out['lo'][c]}, {out['hi'][c]}]")
    print(f"extremes: min {out['min']}, max {out['max']}")
    print(f"w_bound = {np.array2string(out['w_bound'], precision=4)}   (workloads.cartpole(): {model['w_bound']}, calibrated on the reference's PyBullet plant)")
    where = "host twin" if args.host else f"device: rollout {out['rollout_ms']:.2f} ms, selection {out['selection_ms']:.2f} ms"
    print(f"{out['n_samples']} samples per component from {args.n_traj} trajectories x {args.periods} periods, {wall:.2f} s ({where})")


if __name__ == "__main__":
    main()
