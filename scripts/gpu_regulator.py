"""Throughput of the regulator QPs on one MI355X (reported in DESIGN.md, not gated): batch solves of the Mayne tube regulator
(Example_of_Tube_Regulator_MPC.py) at B = 4096 and 65536, and its device-resident closed loop (tmpc_reg_run) at 4096
trajectories x 100 steps as MPC steps per second.

    python scripts/gpu_regulator.py [--reps 10]

Solve times are the device time of the launch (HIP events around it on the handle's stream, tmpc_last_kernel_ms), after two
warm-up calls; the closed loop is timed on the host around the whole call, which synchronises before it returns (uploads,
T solve + step launches, statistics back), after one warm-up run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "robust-tracking-mpc-over-lossy-networks_amd")]
import regulator_problems as rp                         # noqa: E402
from LinearMPCOverNetworks import _native, polytope_lite  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    polytope_lite.set_lp_backend("scipy")
    m = rp.mayne_tube(device=0)
    res = {"kernel": _native.kernel_name(m._handle), "dims": _native.get_dims(m._handle)}
    rng = np.random.default_rng(0)
    cand = np.c_[rng.uniform(-8.0, 4.0, 4 * 65536), rng.uniform(-3.0, 2.0, 4 * 65536)]
    st = m._solve_regulator(cand)["status"]
    feas = cand[st == 0]
    for B in (4096, 65536):
        x = np.ascontiguousarray(feas[:B])
        for _ in range(2):
            _native.solve_regulator_batch(m._handle, x, want_traj=False)
        ms = []
        for _ in range(args.reps):
            out = _native.solve_regulator_batch(m._handle, x, want_traj=False)
            ms.append(_native.last_kernel_ms(m._handle))
        res[f"solve_B{B}_ms_median"] = float(np.median(ms))
        res[f"solve_B{B}_ms_min"] = float(np.min(ms))
        res[f"solve_B{B}_qps"] = B / (np.median(ms) * 1e-3)
        res[f"solve_B{B}_iters_mean"] = float(out["iters"].mean())
    B, T = 4096, 100
    x0 = feas[:B]
    m.run_closed_loop(x0, T, seed=1)
    secs = []
    for _ in range(max(3, args.reps // 3)):
        t0 = time.perf_counter()
        out = m.run_closed_loop(x0, T, seed=1)
        secs.append(time.perf_counter() - t0)
    res["loop_4096x100_s_median"] = float(np.median(secs))
    res["loop_mpc_steps_per_s"] = B * T / float(np.median(secs))
    res["loop_tube_viol"] = int(out["tube_viol"].sum())
    res["loop_fail"] = int((out["fail_step"] >= 0).sum())
    print(json.dumps(res))
    m._close()


if __name__ == "__main__":
    main()
