"""Whole solves through the wave kernels whose triangular solves tests/test_select_free_end_to_end_gpu.py compares between two builds of
the library; run as a program in a process of its own, because the library is chosen when the package is imported (TMPC_LIB):

    python tests/select_free_end_to_end.py out.npz

Four shapes, chosen for the paths of csrc/tmpc_wave.hpp they compile: <11,1,0,5,4,0,8> (the bench shape: NV = 11, refinement with working
sets of 12 and of the full capacity), <12,1,0,5,4,0,8> (NV = 12), <8,0,2,0,0,0,8> and <16,0,4,0,0,0,4> (dense rows only; NV = 16 is the
size at which the pattern above the last lane is empty).  The cart-pole shapes solve the 600 fixture states and the two rows the parity
tests append (an infeasible one and one that needs no iteration); the double-integrator shapes 256 states of tests/shape_cases.py --
interior, boundary, outside -- and the same two kinds of row.  The bench shape then runs a warm-started closed loop of 64 trajectories x
8 steps with a step in the reference, as one fused launch and as a launch pair per step: its solves start in the refinement."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import common  # noqa: E402  (puts the repository and the package on sys.path)

KERNELS = {"cartpole-N10": "tmpc::solve_kernel<11,1,0,5,4,0,8>", "cartpole-N11": "tmpc::solve_kernel<12,1,0,5,4,0,8>",
           "double_integrator-N5": "tmpc::solve_kernel<8,0,2,0,0,0,8>", "double_integrator-N13": "tmpc::solve_kernel<16,0,4,0,0,0,4>"}
SOLVE_KEYS = ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")
LOOP_KEYS = ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum", "x_traj", "x_nom_traj", "u_traj")


def run_all():
    from LinearMPCOverNetworks import _native, montecarlo, polytope_lite
    import shape_cases
    polytope_lite.set_lp_backend("scipy")          # (as tests/conftest.py)
    out = {}
    S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
    Xc = np.r_[S[:, :4], [[0.0, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0]]]
    Rc = np.r_[S[:, 4:], [[0.5, 0, 0, 0.0], [0.5, 0, 0, 0.0]]]
    bench = None
    for name, N, fixed in (("cartpole", 10, True), ("cartpole", 11, True), ("double_integrator", 5, False), ("double_integrator", 13, False)):
        tag = f"{name}-N{N}"
        mpc, w = common.make_mpc(name, N, fixed, create=True)
        out[tag + "/kernel"] = np.array(_native.kernel_name(mpc._handle))
        if name == "cartpole":
            X, R = Xc, Rc
        else:
            X, R = shape_cases.tracking_states(mpc, np.random.default_rng(1000 * N), 256)
            X = np.r_[X, [[0.0, 0.0], [30.0, 0.0]]]
            R = np.r_[R, np.zeros((2, R.shape[1]))]
        sol = mpc._solve(np.ascontiguousarray(X), np.ascontiguousarray(R))
        for k in SOLVE_KEYS:
            out[f"{tag}/{k}"] = np.asarray(sol[k])
        if tag == "cartpole-N10":
            bench = (mpc, w)
    mpc, w = bench
    nb, T = 64, 8
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=17)
    ref = np.where(np.arange(T) < 4, 0.5, -0.3)
    for fused in ("on", "off"):
        loop = mpc.run_closed_loop(np.full(nb, 0.3), ref, th, ga, dist, warm_start=True, capture=5, fused=fused)
        assert bool(loop["fused"]) == (fused == "on")
        for k in LOOP_KEYS:
            out[f"loop-{fused}/{k}"] = np.asarray(loop[k])
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_all())
